"""Shapes and seeded inputs of the normalisation, gradient-penalty and GAN-loss kernel tests: tests/test_gpu_norm_gan.py runs the kernels on them,
tests/test_blocked_ref.py shows on a machine without a GPU that stock fp32 arithmetic meets the bounds on exactly these inputs and that the listed
wrong variants do not.  Everything a backward-type kernel reads as `saved` state (a, stats) is made here with stock torch in fp32: no kernel output
is an input of another kernel's test."""
import functools

import torch
import torch.nn.functional as F

from oracle import blocked_ref as R

SLOPE, EPS = R.f32(0.2), R.f32(1e-5)
# norm kernels: 64 pixel lanes per workgroup: fewer pixels than lanes, exactly one pass, one full pass + a ragged one, three full passes + a ragged one
NORM_HW = [(1, 3), (8, 8), (7, 10), (13, 19)]
# a quad that is one quarter real, an exact plane, two planes with a half-real quad in the last
NORM_C = [5, 16, 22]
IN_N = 3
# (N, group): two full groups, a ragged last group (one image), group == N, group == 1
BN_NG = [(4, 2), (3, 2), (3, 3), (2, 1)]
# per-pixel kernels: N H W = 70: one partial workgroup; 494: a full one and a partial one (the grid sum crosses workgroups)
PIX_N, PIX_HW, PIX_C = 2, [(5, 7), (13, 19)], [1, 3, 16]
RAGAN_HW = PIX_HW + [(17, 19)]             # dasr_ragan runs one thread per PIXEL: 323 pixels are what takes its grid sum across two workgroups
LOW, CONST = 1, 2                         # channel with low variance and a large mean; constant channel (forward kernels only)
N_GLOB = 6                                # ragan: 2 local + 4 remote samples


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(base, *dims):
    s = base
    for d in dims:
        s = s * 31 + d
    return s


def norm_x(N, C, H, W, seed, const=False):
    """randn * 1.5 + 0.3; channel LOW 3 + 0.01 randn (eps is visible, the two-pass variance cancels); channel CONST constant (var == 0)"""
    g = gen(seed)
    x = torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3
    x[:, LOW] = 3.0 + 0.01 * torch.randn(N, H, W, generator=g)
    if const:
        x[:, CONST] = 0.7
    return x


@functools.lru_cache(maxsize=None)
def in_fwd(C, H, W):
    return norm_x(IN_N, C, H, W, _seed(300, C, H, W), const=True)


@functools.lru_cache(maxsize=None)
def in_saved(C, H, W):
    """what inorm_lrelu_bwd / _jvp / _second read: the saved output a (with +0 and -0 planted) and rstd of a stock fp32 forward, upstream ga, tangent t,
    a previous `out`"""
    g = gen(_seed(301, C, H, W))
    x = norm_x(IN_N, C, H, W, _seed(302, C, H, W))
    var, mean = torch.var_mean(x, (2, 3), unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    a = F.leaky_relu(F.instance_norm(x, eps=EPS), SLOPE)
    a[0, 0, 0, 0], a[1, C - 1, H - 1, W - 1], a[2, 3, 0, W - 1] = 0.0, -0.0, -0.0
    if H * W > 64:
        a[0, 2, H - 1, W - 1] = 0.0       # in the ragged last pass
    ga, t, out0 = (torch.randn(IN_N, C, H, W, generator=g) for _ in range(3))
    return dict(a=a, mean=mean, rstd=rstd, ga=ga, t=t, out0=out0)


def bn_params(C, g):
    """gamma of both signs away from zero, beta; channel LOW gets beta = 6: its z stays positive (the bound of its xhat is wide, see bn_saved)"""
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    beta = torch.randn(C, generator=g) * 0.3
    beta[LOW] = 6.0
    return gamma, beta


@functools.lru_cache(maxsize=None)
def bn_fwd(N, group, C, H, W):
    g = gen(_seed(310, N, group, C, H, W))
    gamma, beta = bn_params(C, g)
    beta[LOW] = 0.1                       # the forward kernels take both branches in this channel too
    return dict(x=norm_x(N, C, H, W, _seed(311, N, group, C, H, W), const=True), gamma=gamma, beta=beta)


def bn_stats32(x, group):
    """(mean, rstd, var) [G][C] of a stock fp32 evaluation"""
    rows = [torch.var_mean(x[n0:n1], (0, 2, 3), unbiased=False) for n0, n1 in R.groups(x.shape[0], group)]
    var, mean = torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])
    return mean, 1.0 / torch.sqrt(var + EPS), var


@functools.lru_cache(maxsize=None)
def bn_saved(N, group, C, H, W):
    """what bnorm_lrelu_bwd / _jvp / _second read.  These kernels recompute z = gamma xhat + beta in fp32 and branch on its sign, the reference
    branches on the fp64 z: the inputs are conditioned so that no |z| comes near its rounding bound -- elements of x whose z lies within 400 x the
    FORWARD bound of z are moved by 0.05 away from the branch (a handful; a condition on the inputs, no element is left out of any comparison).
    z_margin = min |z| / (100 x bound) over the real channels, which the tests assert to exceed 1."""
    g = gen(_seed(320, N, group, C, H, W))
    gamma, beta = bn_params(C, g)
    x = norm_x(N, C, H, W, _seed(321, N, group, C, H, W))
    for _ in range(8):
        with R.fp64_arithmetic():
            z = R.bnorm_lrelu_fwd(x, group, EPS, SLOPE, gamma, beta)[1]
        near = z.v.abs() <= 400.0 * z.tol()
        if not bool(near.any()):
            break
        push = torch.where(z.v >= 0, 1.0, -1.0) * torch.sign(gamma.double()).view(1, C, 1, 1) * 0.05
        x = torch.where(near, x.double() + push, x.double()).float()
    with R.fp64_arithmetic():
        z = R.bnorm_lrelu_fwd(x, group, EPS, SLOPE, gamma, beta)[1]
    mean, rstd, var = bn_stats32(x, group)
    ga, t, out0 = (torch.randn(N, C, H, W, generator=g) for _ in range(3))
    return dict(x=x, gamma=gamma, beta=beta, mean=mean, rstd=rstd, var=var, ga=ga, t=t, out0=out0, dgamma0=torch.randn(C, generator=g),
                z_margin=float((z.v.abs() / (100.0 * z.tol())).min()))


PLANTED = [20.0, -20.0, 100.0, -100.0]


@functools.lru_cache(maxsize=None)
def logits(C, H, W, seed=330, planted=True):
    """randn * 3 with +-20 and +-100 planted (saturation)"""
    x = torch.randn(PIX_N, C, H, W, generator=gen(_seed(seed, C, H, W))) * 3.0
    for i, v in enumerate(PLANTED if planted else []):
        x[i % PIX_N, (i // 2) % C, i % H, (2 * i + 1) % W] = v
    return x


@functools.lru_cache(maxsize=None)
def ragan_inputs(H, W, planted=True):
    """(a, b) of this rank [2][1][H][W] and of the four remote samples [4][1][H][W]"""
    g = gen(_seed(340, H, W))
    a, b = logits(1, H, W, 341, planted), logits(1, H, W, 342, planted)
    return a, b, torch.randn(N_GLOB - PIX_N, 1, H, W, generator=g) * 3.0, torch.randn(N_GLOB - PIX_N, 1, H, W, generator=g) * 3.0


def ragan_allreduce(local32, remote):
    """the SUM all-reduce of a per-pixel fp32 buffer as the test plays it: the local fp32 word plus the remote samples' fp32 contributions, in fp32"""
    out = local32.float().clone()
    for r in remote:
        out = out + r.float()
    return out


@functools.lru_cache(maxsize=None)
def gp_inputs(C, H, W):
    return torch.randn(PIX_N, C, H, W, generator=gen(_seed(350, C, H, W))) * 0.05


# ---- the operations on these inputs: (inputs, {name: Ev}) --------------------------------------------------------------------------------------
# One function per kernel and mode; the GPU tests upload `inputs`, compare with the Ev values and apply Ev.tol(); test_blocked_ref evaluates the same
# call in fp32 and with every `wrong` the entry lists.
def ref_in_fwd(C, H, W, wrong=None):
    x = in_fwd(C, H, W)
    y, mean, rstd = R.inorm_lrelu_fwd(x, EPS, SLOPE, wrong)
    return dict(x=x), dict(y=y, mean=mean, rstd=rstd)


def ref_in_bwd(C, H, W, wrong=None):
    i = in_saved(C, H, W)
    return i, dict(gx=R.inorm_lrelu_bwd(i['a'], i['ga'], i['rstd'], SLOPE, wrong))


def ref_in_jvp(C, H, W, wrong=None):
    i = in_saved(C, H, W)
    return i, dict(out=R.inorm_lrelu_jvp(i['a'], i['t'], i['rstd'], SLOPE, wrong))


def ref_in_second(C, H, W, acc, wrong=None):
    i = in_saved(C, H, W)
    return i, dict(out=R.inorm_second(i['a'], i['t'], i['ga'], i['rstd'], SLOPE, i['out0'] if acc else None, wrong))


def ref_bn_fwd(N, group, C, H, W, wrong=None):
    i = bn_fwd(N, group, C, H, W)
    y, z, mean, rstd, var = R.bnorm_lrelu_fwd(i['x'], group, EPS, SLOPE, i['gamma'], i['beta'], wrong)
    return i, dict(y=y, mean=mean, rstd=rstd, var=var)


PSCALE = R.f32(0.37)


def ref_bn_bwd(N, group, C, H, W, wrong=None):
    i = bn_saved(N, group, C, H, W)
    gx, dg, db, z = R.bnorm_lrelu_bwd(i['x'], i['ga'], group, SLOPE, i['gamma'], i['beta'], i['mean'], i['rstd'], PSCALE, wrong)
    return i, dict(gx=gx, dgamma=dg, dbeta=db)


def ref_bn_jvp(N, group, C, H, W, wrong=None):
    i = bn_saved(N, group, C, H, W)
    return i, dict(out=R.bnorm_lrelu_jvp(i['x'], i['t'], group, SLOPE, i['gamma'], i['beta'], i['mean'], i['rstd'], wrong)[0])


def ref_bn_second(N, group, C, H, W, acc, wrong=None):
    i = bn_saved(N, group, C, H, W)
    out, dg, z = R.bnorm_second(i['x'], i['t'], i['ga'], group, SLOPE, i['gamma'], i['beta'], i['mean'], i['rstd'], i['out0'] if acc else None,
                                i['dgamma0'] if acc else None, PSCALE, wrong)
    return i, dict(out=out, dgamma=dg)


MOMENTUM = R.f32(0.1)
RUNNING = [(5, 2, 70, 1), (22, 1, 1, 0), (16, 3, 494, 2)]      # (C, rows of stats, count, g): count == 1 keeps the biased variance


def ref_bn_running(C, G, count, g, wrong=None):
    q = gen(_seed(360, C, count))
    i = dict(mean=torch.randn(G, C, generator=q), var=torch.rand(G, C, generator=q) + 0.1, rmean0=torch.randn(C, generator=q),
             rvar0=torch.rand(C, generator=q) + 0.5)
    rm, rv = R.bnorm_running(i['mean'][g], i['var'][g], count, MOMENTUM, i['rmean0'], i['rvar0'], wrong)
    return i, dict(running_mean=rm, running_var=rv)


TARGETS = [1.0, 0.0, R.f32(0.9)]


def gan_coefs(C, H, W):
    cnt = PIX_N * C * H * W
    return R.f32(1.0 / cnt), R.f32(0.3 / cnt), R.f32(0.7 / cnt)      # coef, gcoef, score_coef


def ref_gan_loss(gan_type, target, C, H, W, wrong=None):
    x = logits(C, H, W)
    l, g = R.gan_loss(x, gan_type, target, gan_coefs(C, H, W)[1], wrong)
    return dict(x=x), dict(l=l, grad=g)


RAGAN_T = {0: [(1.0, 0.0), (R.f32(0.9), 0.0)], 1: [(1.0, 0.0), (0.0, 1.0), (0.0, -1.0)], 2: [(1.0, 0.0)], 3: [(1.0, 0.0), (0.0, 1.0)]}
RAGAN_EPS = R.f32(1e-8)


@functools.lru_cache(maxsize=None)
def ragan_state(form, ta, tb, H, W):
    """the inputs of the three stages: sums_* / part_* are the GLOBAL per-pixel buffers as stages 1 / 2 read them, made here once -- this rank's
    sums (the fp64 reference's, rounded to fp32) plus the fp32 words of the four remote samples, added in fp32.  The GPU test checks the kernel's own
    local words against the reference and then UPLOADS these buffers in their place: what a later stage reads is an input of its reference, bit for bit.
    Form 1 takes the logits without the planted +-20 / +-100: -log(1 - sigmoid(z) + eps) at a saturated sigmoid is ill-conditioned (the fp32 argument
    may lie anywhere in [eps, eps + 2e-7]: the term is only known to about +-3), which would leave the loss accumulator with a bound of per cents;
    tests/test_gpu_norm_gan.py::test_ragan_form1_saturated_logits_stay_finite holds the saturated case on its own."""
    a, b, ra, rb = ragan_inputs(H, W, form != 1)
    with R.fp64_arithmetic():
        sa, sb = R.ragan_sums(a, b)
        i = dict(a=a, b=b, ra=ra, rb=rb, sums_a=ragan_allreduce(sa.v, ra), sums_b=ragan_allreduce(sb.v, rb))
        (_, da, _), (_, db, _) = R.ragan_terms(a, b, i['sums_a'], i['sums_b'], N_GLOB, form, ta, tb, RAGAN_EPS)
        (_, rda, _), (_, rdb, _) = R.ragan_terms(ra, rb, i['sums_a'], i['sums_b'], N_GLOB, form, ta, tb, RAGAN_EPS)
        i.update(rda=rda.v.float(), rdb=rdb.v.float(), part_a=ragan_allreduce(da.v.sum(0, keepdim=True), rda.v),
                 part_b=ragan_allreduce(db.v.sum(0, keepdim=True), rdb.v))
    return i


def ref_ragan(form, ta, tb, H, W, wrong=None):
    i = ragan_state(form, ta, tb, H, W)
    a, b = i['a'], i['b']
    gcoef = gan_coefs(1, H, W)[1]
    sa, sb = R.ragan_sums(a, b)
    (la, da, s_a), (lb, db, s_b) = R.ragan_terms(a, b, i['sums_a'], i['sums_b'], N_GLOB, form, ta, tb, RAGAN_EPS, wrong)
    qa, qb = da.sum((0,), PIX_N), db.sum((0,), PIX_N)
    ga, gb = R.ragan_grads(da, db, i['part_a'], i['part_b'], N_GLOB, gcoef, wrong)
    score_a, score_b = (s_a, s_b) if form == 1 else (R.Ev(a), R.Ev(b))
    return i, dict(sums_a=sa, sums_b=sb, la=la, lb=lb, qa=qa, qb=qb, score_a=score_a, score_b=score_b, ga=ga, gb=gb)


ACC0 = dict(loss=0.25, score=-1.5, score_b=0.75)                   # what the accumulators hold before the launch


def gan_accs(gan_type, target, C, H, W):
    """{name: (value, bound)} of the accumulators of dasr_gan_loss: a thread adds its C terms, then the workgroup and grid chain (R.acc_sum)"""
    i, ref = ref_gan_loss(gan_type, target, C, H, W)
    coef, _, scoef = gan_coefs(C, H, W)
    nb = (PIX_N * H * W + 255) // 256
    return dict(loss=R.acc_sum(ref['l'], coef, ACC0['loss'], C, nb), score=R.acc_sum(R.Ev(i['x']), scoef, ACC0['score'], C, nb))


def ragan_accs(form, ta, tb, H, W):
    """the accumulators of dasr_ragan stage 1: a thread (one per PIXEL) adds la + lb over its N samples (2 N terms; N for a score)"""
    i, ref = ref_ragan(form, ta, tb, H, W)
    coef, _, scoef = gan_coefs(1, H, W)
    nb = (H * W + 255) // 256
    return dict(loss=R.acc_sum(R.ev_cat([ref['la'], ref['lb']]), coef, ACC0['loss'], 2 * PIX_N, nb),
                score_a=R.acc_sum(ref['score_a'], scoef, ACC0['score'], PIX_N, nb), score_b=R.acc_sum(ref['score_b'], scoef, ACC0['score_b'], PIX_N, nb))


GP_WEIGHT = 10.0


def ref_gp(C, H, W, zero=False, wrong=None):
    """stage 0; and stage 1 -> a second rank's word added in fp32 -> stage 2 with world 2"""
    g = gp_inputs(C, H, W) * (0.0 if zero else 1.0)
    with R.fp64_arithmetic():
        s64 = R.grad_penalty_sumsq(g).v
    other = R.f32(float(s64) * 1.3 + 0.01)
    s2 = float(s64.float() + torch.tensor(other))                  # out3[3] after the host's add, as stage 2 reads it
    s = R.grad_penalty_sumsq(g)
    nrm, pen, fac = R.grad_penalty_finish(s, GP_WEIGHT)
    nrm2, pen2, fac2 = R.grad_penalty_finish(R.Ev(s2), GP_WEIGHT, 2, wrong)
    return dict(g=g, other=other), dict(s=s, nrm=nrm, pen=pen, fac=fac, nrm2=nrm2, pen2=pen2, fac2=fac2)


def evals():
    """(id, fn, args, the `wrong` variants that must leave the bound on these inputs)"""
    fwd_wrong = ['mean_count-1', 'unbiased', 'no_eps']
    for C in NORM_C:
        for H, W in NORM_HW:
            s = 'C%d-%dx%d' % (C, H, W)
            yield 'in_fwd-' + s, ref_in_fwd, (C, H, W), fwd_wrong
            yield 'in_bwd-' + s, ref_in_bwd, (C, H, W), ['lrelu1_at0']
            yield 'in_jvp-' + s, ref_in_jvp, (C, H, W), ['lrelu1_at0']
            for acc in (0, 1):
                yield 'in_second-acc%d-%s' % (acc, s), ref_in_second, (C, H, W, acc), ['lrelu1_at0', 'factor2']
            for N, group in BN_NG:
                sb = 'N%dg%d-%s' % (N, group, s)
                many, ragged = N > group, N % group != 0
                yield 'bn_fwd-' + sb, ref_bn_fwd, (N, group, C, H, W), fwd_wrong + (['ragged_drop'] if ragged else [])
                yield 'bn_bwd-' + sb, ref_bn_bwd, (N, group, C, H, W), ['other_row', 'dgamma_first'] if many else []
                yield 'bn_jvp-' + sb, ref_bn_jvp, (N, group, C, H, W), ['other_row'] if many else []
                for acc in (0, 1):
                    yield 'bn_second-acc%d-%s' % (acc, sb), ref_bn_second, (N, group, C, H, W, acc), ['factor2'] + (['other_row', 'dgamma_first'] if many else [])
    for r in RUNNING:
        yield 'bn_running-C%d-count%d' % (r[0], r[2]), ref_bn_running, r, ['biased'] if r[2] > 1 else []
    for C in PIX_C:
        for H, W in PIX_HW:
            s = 'C%d-%dx%d' % (C, H, W)
            for gt in (0, 1, 2):
                for t in TARGETS:
                    yield 'gan_loss-type%d-t%g-%s' % (gt, t, s), ref_gan_loss, (gt, t, C, H, W), ['wgan_sign'] if gt == 2 and t <= 0.5 else []
            yield 'gp-' + s, ref_gp, (C, H, W), ['no_world2']
    for H, W in RAGAN_HW:
        for form, ts in RAGAN_T.items():
            for ta, tb in ts:
                yield 'ragan-form%d-ta%g-tb%g-%dx%d' % (form, ta, tb, H, W), ref_ragan, (form, ta, tb, H, W), ['means_N', 'swap_part']
