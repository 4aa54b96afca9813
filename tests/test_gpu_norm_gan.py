"""GPU parity tests of the first half of csrc/gan.hip -- InstanceNorm / BatchNorm + LeakyReLU forward, backward, tangent and second-order adjoint,
the BatchNorm running statistics, the gradient penalty and its scaled fill, GANLoss and the relativistic average GAN loss -- in every mode
include/dasr_hip.h documents, against the fp64 references of oracle/blocked_ref.py (themselves held to stock torch by tests/test_blocked_ref.py).

Set-up as in tests/test_gpu_elementwise.py, whose machinery this file shares: every blocked tensor is plane(s) p0 > 0 of a wider sentinel-filled slab
(n_stride != K * cb_stride) and everything outside the written view must hold the sentinel bit for bit afterwards; flat buffers (stats, gamma, dgamma,
accumulators, ...) have sentinel words in front and behind; every case through the ctypes entry point (via = abi) and as a recorded op through
dasr_run_ops (via = op).  Shapes and seeded inputs come from oracle/norm_gan_cases.py: tests/test_blocked_ref.py shows on the same inputs that stock
fp32 arithmetic meets every bound applied here and that a list of wrong variants does not.

What is asserted: |got - ref| <= bound ELEMENTWISE.  The bound is Ev.tol() of the reference: u32 = 2^-24 times the magnitude of every intermediate
result times the roundings behind it, carried along the kernel's own expression (oracle/blocked_ref.py, class Ev: one rounding per operation, a
fused multiply-add counted as two, expf / logf / log1pf 1 ulp = 2 u as in tests/test_gpu_filters.py); a reduction is counted along the kernel's
chain (lane_chain: the lane's ceil(count / 64) terms, four butterfly steps, three cross-wave adds; then the multiply by the rounded 1 / count), and
the propagation goes mean -> variance -> rstd -> output.  The comment beside each comparison says which chain it is.  Exact results are asserted bit
for bit.  No tolerance here is tuned to a GPU run: the margins log records the measured slack."""
import pytest
import torch

from oracle import blocked_ref as R
from oracle import norm_gan_cases as K
from test_gpu_elementwise import EINVAL, G, SENT, VIA, Buf, Slab, _gpu, _grid_chain, biteq, bounded, call, ev_ok, gpu

assert _grid_chain(3) == R.grid_chain(3)  # the accumulators are bounded with test_l1_diff's chain


def slab(dev, x, pad=0.0, lead=1):
    """the NCHW tensor x as planes of a sentinel-filled slab, its padding channels holding `pad`"""
    N, C, H, W = x.shape
    return Slab(dev, 'f32', N, R.planes(C), H, W, R.pack(x, 'f32', pad), lead=lead)


def out_slab(dev, N, C, H, W, lead=2):
    return Slab(dev, 'f32', N, R.planes(C), H, W, None, lead=lead)


def zeros_from(t, C):
    return biteq(t[:, C:], torch.zeros_like(t[:, C:]))


def cpad(C):
    return R.planes(C) * 16


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# InstanceNorm2d + LeakyReLU.  Contract (dasr_hip.h): whole 16-channel planes are processed, the padding channels like real ones -- zero in, zero out.
def in_stats(i, C):
    """stats [N][Cpad][2] = (mean, rstd) as a stock fp32 forward leaves them; the (all-zero) padding channels: mean 0, rstd 1 / sqrt(eps)"""
    N = i['rstd'].shape[0]
    st = torch.zeros(N, cpad(C), 2)
    st[:, :, 1] = 1.0 / torch.sqrt(torch.tensor(K.EPS))
    st[:, :C, 0], st[:, :C, 1] = i['mean'][:, :, 0, 0], i['rstd'][:, :, 0, 0]
    return st


@gpu
@VIA
@pytest.mark.parametrize('C', K.NORM_C)
def test_inorm_lrelu_fwd(C, via, margins):
    dev = _gpu()
    N = K.IN_N
    for H, W in K.NORM_HW:
        i, ref = K.ref_in_fwd(C, H, W)
        xs = slab(dev, i['x'])
        for with_stats in (True, False):
            ys, st = out_slab(dev, N, C, H, W), Buf(dev, n=N * cpad(C) * 2)
            assert call(via, 'inorm_lrelu_fwd', x=xs.view(), N=N, C=C, H=H, W=W, eps=K.EPS, slope=K.SLOPE, y=ys.view(),
                        stats=st.ptr if with_stats else None) == 0
            tag = 'C%d %dx%d stats %d %s' % (C, H, W, with_stats, via)
            got = ys.nchw()
            # mean: lane_chain(ceil(HW / 64)) and the product with the rounded 1 / HW; variance: x - mean (1), its square (1), the same chain, plus the
            # square of the mean's own bound; rstd: var + eps (1), sqrtf (1), the division (1); y: (x - mean) (1) * rstd (1), * slope (1).  The constant
            # channel: x - mean is the error of the mean alone, y lies within rstd * that of zero
            ev_ok('inorm_fwd y ' + tag, got[:, :C], ref['y'], margins)
            assert zeros_from(got, C) and ys.outside_untouched() and xs.untouched()
            if not with_stats:
                assert st.untouched()
                continue
            s = st.get().view(N, cpad(C), 2)
            bounded('inorm_fwd mean ' + tag, s[:, :C, 0], ref['mean'].v[:, :, 0, 0], ref['mean'].tol()[:, :, 0, 0], margins)
            bounded('inorm_fwd rstd ' + tag, s[:, :C, 1], ref['rstd'].v[:, :, 0, 0], ref['rstd'].tol()[:, :, 0, 0], margins)
            # the padding channels' statistics are those of an all-zero channel: mean 0, rstd 1 / sqrt(0 + eps) (sqrtf and the division: 2 roundings)
            assert bool((s[:, C:, 0] == 0).all())
            assert bool(((s[:, C:, 1].double() - K.EPS ** -0.5).abs() <= 2 * R.U32 * K.EPS ** -0.5).all()) and st.guards_ok()


IN_BACK = [('inorm_lrelu_bwd', K.ref_in_bwd, 'gx', ()), ('inorm_lrelu_jvp', K.ref_in_jvp, 'out', ()), ('inorm_second', K.ref_in_second, 'out', (0,)),
           ('inorm_second', K.ref_in_second, 'out', (1,))]


@gpu
@VIA
@pytest.mark.parametrize('C', K.NORM_C)
@pytest.mark.parametrize('kern', IN_BACK, ids=['bwd', 'jvp', 'second_acc0', 'second_acc1'])
def test_inorm_backward_tangent_second(kern, C, via, margins):
    """the kernels that read the saved output a: xhat = a > 0 ? a : a / slope and LeakyReLU' = a > 0 ? 1 : slope, so at the planted a == +0 and -0 the
    slope branch with xhat = 0 -- decided from the same bits on both sides"""
    dev = _gpu()
    name, reffn, outname, extra = kern
    N = K.IN_N
    for H, W in K.NORM_HW:
        i, ref = reffn(C, H, W, *extra)
        assert bool((i['a'] == 0).any()) and bool((i['ga'][i['a'] == 0] != 0).all())
        as_, gs, ts = slab(dev, i['a']), slab(dev, i['ga'], lead=2), slab(dev, i['t'], lead=3)
        st = Buf(dev, in_stats(i, C))
        acc = bool(extra and extra[0])
        os_ = slab(dev, i['out0'], lead=2) if acc else out_slab(dev, N, C, H, W)
        kw = dict(a=as_.view(), N=N, C=C, H=H, W=W, slope=K.SLOPE, stats=st.ptr)
        kw[outname] = os_.view()
        if name != 'inorm_lrelu_jvp':
            kw['ga'] = gs.view()
        if name != 'inorm_lrelu_bwd':
            kw['t'] = ts.view()
        if name == 'inorm_second':
            kw['accumulate'] = int(acc)
        assert call(via, name, **kw) == 0
        got = os_.nchw()
        # xhat: 1 / slope (1) and the product (1); gy = ga * slope (1); every mean: its products, lane_chain(ceil(HW / 64)), * the rounded 1 / HW;
        # then the kernel's expression term by term -- bwd / jvp: rstd * (g - m1 - xhat * m2); second: the five means (sum |term| each), k0, and
        # out0 - rstd^2 * (xhat * k0 + pz * (w - mw) + pw * (t - mz))
        ev_ok('%s acc %d C%d %dx%d %s' % (name, acc, C, H, W, via), got[:, :C], ref[outname], margins)
        assert zeros_from(got, C) and os_.outside_untouched()
        assert as_.untouched() and gs.untouched() and ts.untouched() and st.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm2d (training mode, groups) + LeakyReLU.  Contract (dasr_hip.h): gamma / beta are read below C only and taken as 0 from C on, so the padding
# channels of every output are zero whatever the padding channels of the inputs hold (finite); stats has ceil(N / group) rows of Cpad entries.
JUNK = 55.5


def bn_params(dev, i, C):
    """gamma, beta: C values, then finite junk the kernels must not read"""
    return (Buf(dev, torch.cat([i[k], torch.full((cpad(C) - C + 8,), JUNK)])) for k in ('gamma', 'beta'))


def bn_stats(i, C, rows_behind=1):
    """stats [G][Cpad][3] = (mean, rstd, biased variance) of a stock fp32 forward (junk in the padding entries), and sentinel rows behind"""
    Gn = i['mean'].shape[0]
    st = torch.full((Gn + rows_behind, cpad(C), 3), JUNK)
    st[Gn:] = SENT
    st[:Gn, :C, 0], st[:Gn, :C, 1], st[:Gn, :C, 2] = i['mean'], i['rstd'], i['var']
    return st


@gpu
@VIA
@pytest.mark.parametrize('C', K.NORM_C)
@pytest.mark.parametrize('ng', K.BN_NG, ids=['N%dg%d' % ng for ng in K.BN_NG])
def test_bnorm_lrelu_fwd(ng, C, via, margins):
    dev = _gpu()
    N, group = ng
    Gn = len(R.groups(N, group))
    for H, W in K.NORM_HW:
        i, ref = K.ref_bn_fwd(N, group, C, H, W)
        xs, ys = slab(dev, i['x'], pad=77.0), out_slab(dev, N, C, H, W)
        gm, bt = bn_params(dev, i, C)
        st = Buf(dev, n=(Gn + 1) * cpad(C) * 3)                      # one row more than ceil(N / group): it must stay as it is
        assert call(via, 'bnorm_lrelu_fwd', x=xs.view(), N=N, C=C, H=H, W=W, group=group, eps=K.EPS, slope=K.SLOPE, gamma=gm.ptr, beta=bt.ptr, y=ys.view(),
                    stats=st.ptr) == 0
        tag = 'N%d g%d C%d %dx%d %s' % (N, group, C, H, W, via)
        got = ys.nchw()
        # as inorm_fwd with count = (images of the group) * HW and lane_chain(images * ceil(HW / 64)) per group (the ragged last group has its own
        # count), then xhat * gamma (1) + beta (1) before the LeakyReLU
        ev_ok('bnorm_fwd y ' + tag, got[:, :C], ref['y'], margins)
        assert zeros_from(got, C) and ys.outside_untouched() and xs.untouched() and gm.untouched() and bt.untouched()
        s = st.get().view(Gn + 1, cpad(C), 3)
        for k, nm in enumerate(('mean', 'rstd', 'var')):
            ev_ok('bnorm_fwd %s %s' % (nm, tag), s[:Gn, :C, k], ref[nm], margins)
        assert bool(torch.isfinite(s[:Gn]).all()) and biteq(s[Gn], torch.full_like(s[Gn], SENT)) and st.guards_ok()


BN_BACK = [('bnorm_lrelu_bwd', K.ref_bn_bwd, 'gx', ()), ('bnorm_lrelu_bwd', K.ref_bn_bwd, 'gx', ('no_dgamma',)), ('bnorm_lrelu_jvp', K.ref_bn_jvp, 'out', ()),
           ('bnorm_second', K.ref_bn_second, 'out', (0,)), ('bnorm_second', K.ref_bn_second, 'out', (1,)),
           ('bnorm_second', K.ref_bn_second, 'out', (1, 'no_dgamma'))]


@gpu
@VIA
@pytest.mark.parametrize('C', K.NORM_C)
@pytest.mark.parametrize('ng', K.BN_NG, ids=['N%dg%d' % ng for ng in K.BN_NG])
@pytest.mark.parametrize('kern', BN_BACK, ids=['bwd', 'bwd_no_dgamma', 'jvp', 'second_acc0', 'second_acc1', 'second_acc1_no_dgamma'])
def test_bnorm_backward_tangent_second(kern, ng, C, via, margins):
    """the kernels that recompute z = gamma xhat + beta from the saved x and the statistics rows and branch on z > 0: the inputs keep every |z| more
    than 100 x the forward bound of z away from the branch (z_margin, oracle/norm_gan_cases.py::bn_saved)"""
    dev = _gpu()
    name, reffn, outname, extra = kern
    N, group = ng
    no_dg = 'no_dgamma' in extra
    acc = bool(extra and extra[0] == 1)
    for H, W in K.NORM_HW:
        i, ref = reffn(N, group, C, H, W, *[e for e in extra if e != 'no_dgamma'])
        assert i['z_margin'] > 1.0
        xs, gs, ts = slab(dev, i['x'], pad=77.0), slab(dev, i['ga'], pad=5.0, lead=2), slab(dev, i['t'], pad=-3.0, lead=3)
        gm, bt = bn_params(dev, i, C)
        st = Buf(dev, bn_stats(i, C))
        os_ = slab(dev, i['out0'], pad=3.25, lead=2) if acc else out_slab(dev, N, C, H, W)
        dg = Buf(dev, torch.cat([i['dgamma0'], torch.full((cpad(C) - C + 8,), SENT)]) if acc else None, n=cpad(C) + 8)
        db = Buf(dev, n=cpad(C) + 8)
        kw = dict(x=xs.view(), N=N, C=C, H=H, W=W, group=group, slope=K.SLOPE, gamma=gm.ptr, beta=bt.ptr, stats=st.ptr)
        kw[outname] = os_.view()
        if name != 'bnorm_lrelu_jvp':
            kw['ga'] = gs.view()
        if name != 'bnorm_lrelu_bwd':
            kw['t'] = ts.view()
        if name == 'bnorm_second':
            kw.update(accumulate=int(acc), dgamma=None if no_dg else dg.ptr, pscale=K.PSCALE)
        if name == 'bnorm_lrelu_bwd' and not no_dg:
            kw.update(dgamma=dg.ptr, dbeta=db.ptr, pscale=K.PSCALE)
        assert call(via, name, **kw) == 0
        tag = '%s N%d g%d C%d %dx%d %s' % ('-'.join([name] + [str(e) for e in extra]), N, group, C, H, W, via)
        got = os_.nchw()
        # xhat = (x - mean) (1) * rstd (1), z = xhat * gamma (1) + beta (1) from the statistics row of the group; the sums over the group:
        # lane_chain(images * ceil(HW / 64)); then the kernel's expression term by term
        ev_ok(tag, got[:, :C], ref[outname], margins)
        if acc:        # out -= rstd^2 * 0 in the padding channels: what was there
            assert bool((got[:, C:] == 3.25).all())
        else:
            assert bool((got[:, C:] == 0).all())
        assert os_.outside_untouched() and xs.untouched() and gs.untouched() and ts.untouched() and gm.untouched() and bt.untouched() and st.untouched()
        if name == 'bnorm_lrelu_jvp' or no_dg:
            assert dg.untouched() and db.untouched()
            continue
        # dgamma / dbeta: the per-group totals (the chain above), added over the groups in order (1 each), * pscale (1); second: + what was there (1)
        d = dg.get()
        ev_ok(tag + ' dgamma', d[:C], ref['dgamma'], margins)
        assert biteq(d[C:], torch.full_like(d[C:], SENT)) and dg.guards_ok()
        if name == 'bnorm_lrelu_bwd':
            d = db.get()
            ev_ok(tag + ' dbeta', d[:C], ref['dbeta'], margins)
            assert biteq(d[C:], torch.full_like(d[C:], SENT)) and db.guards_ok()
        else:
            assert db.untouched()


@gpu
@VIA
@pytest.mark.parametrize('case', K.RUNNING, ids=['C%d-rows%d-count%d-g%d' % r for r in K.RUNNING])
def test_bnorm_running(case, via, margins):
    dev = _gpu()
    C, Gn, count, g = case
    i, ref = K.ref_bn_running(*case)
    st = Buf(dev, bn_stats(dict(mean=i['mean'], rstd=torch.full((Gn, C), JUNK), var=i['var']), C))
    for with_nbt in (True, False):
        rm, rv = (Buf(dev, torch.cat([i[k], torch.full((8,), SENT)])) for k in ('rmean0', 'rvar0'))
        nbt = Buf(dev, torch.tensor([SENT, 7.0, SENT]))
        assert call(via, 'bnorm_running', stats=st.ptr, g=g, C=C, count=count, momentum=K.MOMENTUM, running_mean=rm.ptr, running_var=rv.ptr,
                    num_batches_tracked=nbt.ptr + 4 if with_nbt else None) == 0
        tag = 'C%d count %d g %d %s' % (C, count, g, via)
        # 1 - momentum (1), its product (1), momentum * stat (1), the variance's count / (count - 1) (1) and its product (1), the sum (1)
        ev_ok('bnorm_running mean ' + tag, rm.get()[:C], ref['running_mean'], margins)
        ev_ok('bnorm_running var ' + tag, rv.get()[:C], ref['running_var'], margins)
        assert biteq(rm.get()[C:], torch.full((8,), SENT)) and biteq(rv.get()[C:], torch.full((8,), SENT)) and rm.guards_ok() and rv.guards_ok()
        assert biteq(nbt.get(), torch.tensor([SENT, 8.0 if with_nbt else 7.0, SENT])) and nbt.guards_ok() and st.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_gan_loss (= dasr_bce_logits for gan_type 0)
ACC0 = (K.ACC0['loss'], K.ACC0['score'])   # what the loss / score accumulators hold before the launch


def check_acc(name, got, want_bound, margins):
    """an accumulator against (value, bound) of oracle/norm_gan_cases.py::gan_accs / ragan_accs: the per-term bounds, summed, plus L u32 (coef sum |terms|
    + |acc0|) with L counted as in test_l1_diff (R.acc_sum); tests/test_blocked_ref.py holds every such bound below 2e-5 of coef sum |terms| + |acc0|"""
    want, bound = want_bound
    err = abs(float(got) - want)
    margins('elementwise %s: |err| / bound %.3f' % (name, err / bound))
    assert err <= bound, (name, err, bound)


@gpu
@VIA
@pytest.mark.parametrize('target', K.TARGETS, ids=['t1', 't0', 't0.9'])
@pytest.mark.parametrize('C', K.PIX_C)
@pytest.mark.parametrize('gan_type', [0, 1, 2])
def test_gan_loss(gan_type, C, target, via, margins):
    dev = _gpu()
    N = K.PIX_N
    for H, W in K.PIX_HW:
        i, ref = K.ref_gan_loss(gan_type, target, C, H, W)
        coef, gcoef, scoef = K.gan_coefs(C, H, W)
        xs = slab(dev, i['x'], pad=9.0)                              # the padding channels hold junk: never read
        accs = K.gan_accs(gan_type, target, C, H, W)
        # loss / score / grad each null in turn, all three, none
        for outs in ('lsg', 'sg', 'lg', 'ls', '', 'l'):
            acc = Buf(dev, torch.tensor([SENT, ACC0[0], ACC0[1], SENT]))
            gs = out_slab(dev, N, C, H, W)
            kw = dict(x=xs.view(), N=N, C=C, H=H, W=W, gan_type=gan_type, target=target, coef=coef, gcoef=gcoef, score_coef=scoef)
            if 'l' in outs:
                kw['loss_acc'] = acc.ptr + 4
            if 's' in outs:
                kw['score_acc'] = acc.ptr + 8
            if 'g' in outs:
                kw['grad'] = gs.view()
            assert call(via, 'gan_loss', **kw) == 0
            tag = 'type %d t %g C%d %dx%d [%s] %s' % (gan_type, target, C, H, W, outs, via)
            a = acc.get()
            # per element: type 0 max(x, 0) - x t (2) + log1pf(expf(-|x|)) (2 u each, 1 for the sum); type 1 x - t (1), its square (1); type 2 exact.
            # A thread adds its C terms, then the workgroup and grid chain; the score is the plain sum of x
            if 'l' in outs:
                check_acc('gan_loss loss ' + tag, a[1], accs['loss'], margins)
            else:
                assert float(a[1]) == ACC0[0]
            if 's' in outs:
                check_acc('gan_loss score ' + tag, a[2], accs['score'], margins)
            else:
                assert float(a[2]) == ACC0[1]
            assert float(a[0]) == SENT and float(a[3]) == SENT and acc.guards_ok() and xs.untouched()
            if 'g' not in outs:
                assert gs.untouched()
                continue
            got = gs.nchw()
            assert zeros_from(got, C) and gs.outside_untouched()
            if gan_type == 2:      # -+ gcoef: exact
                assert biteq(got[:, :C], ref['grad'].v.float())
                continue
            # type 0: expf (2 u), 1 + e (1), the division (1), - t (1), * gcoef (1); type 1: x - t (1), * 2 gcoef (1)
            ev_ok('gan_loss grad ' + tag, got[:, :C], ref['grad'], margins)
            if gan_type == 0:      # saturated logits: sigmoid is exactly 1 (0) at +100 and +20 (-100), the gradient the exact constant gcoef * (s - t)
                x, tt, gc = i['x'], torch.tensor(target), torch.tensor(gcoef)
                for v, s in ((100.0, 1.0), (20.0, 1.0), (-100.0, 0.0)):
                    assert bool((x == v).any()) and biteq(got[:, :C][x == v], ((torch.tensor(s) - tt) * gc).expand(int((x == v).sum())))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_ragan: three stages, the all-reduces between them played by the host
RAGAN = [(f, ta, tb) for f, ts in K.RAGAN_T.items() for ta, tb in ts]


@gpu
@VIA
@pytest.mark.parametrize('form,ta,tb', RAGAN, ids=['form%d-ta%g-tb%g' % r for r in RAGAN])
def test_ragan(form, ta, tb, via, margins):
    dev = _gpu()
    N, NG = K.PIX_N, K.N_GLOB
    for H, W in K.RAGAN_HW:
        HW = H * W
        i, ref = K.ref_ragan(form, ta, tb, H, W)
        coef, gcoef, scoef = K.gan_coefs(1, H, W)
        as_, bs = slab(dev, i['a'], pad=9.0), slab(dev, i['b'], pad=-9.0, lead=2)
        sums, part = Buf(dev, n=2 * HW), Buf(dev, n=2 * HW)
        base = dict(a=as_.view(), b=bs.view(), N=N, H=H, W=W, n_glob=NG, form=form, ta=ta, tb=tb, coef=coef, gcoef=gcoef, eps=K.RAGAN_EPS, score_coef=scoef,
                    sums=sums.ptr, part=part.ptr)
        tag = 'form %d ta %g tb %g %dx%d %s' % (form, ta, tb, H, W, via)
        # stage 0: the N local samples added in order
        assert call(via, 'ragan', stage=0, **base) == 0
        s = sums.get()
        bounded('ragan sums_a ' + tag, s[:HW], ref['sums_a'].v.view(-1), ref['sums_a'].tol().view(-1), margins)
        bounded('ragan sums_b ' + tag, s[HW:], ref['sums_b'].v.view(-1), ref['sums_b'].tol().view(-1), margins)
        assert sums.guards_ok() and part.untouched()
        # the SUM all-reduce over n_glob = 6 samples.  The kernel's own local words have just been held to the reference; what stage 1 reads is UPLOADED
        # in their place: the global buffer of oracle/norm_gan_cases.py::ragan_state (the reference's local sums rounded to fp32 plus the four remote
        # samples' fp32 words), so that the reference of the next stage reads the very words the kernel reads
        sums.put(torch.cat([i['sums_a'].view(-1), i['sums_b'].view(-1)]))
        # stage 1: z = x - sums * (1 / n_glob) (2), the term; a thread adds la + lb over its N samples (2 N terms), then the workgroup and grid chain
        accs = K.ragan_accs(form, ta, tb, H, W)
        for outs in ('lab', 'l', 'a', 'b', ''):
            acc = Buf(dev, torch.tensor([SENT, 0.25, SENT, -1.5, SENT, 0.75, SENT]))
            part.put(torch.full((2 * HW,), SENT))
            kw = dict(base, stage=1)
            for ch, nm, off in (('l', 'loss_acc', 4), ('a', 'score_a', 12), ('b', 'score_b', 20)):
                if ch in outs:
                    kw[nm] = acc.ptr + off
            assert call(via, 'ragan', **kw) == 0
            a = acc.get()
            t1 = '%s [%s]' % (tag, outs)
            if 'l' in outs:
                check_acc('ragan loss ' + t1, a[1], accs['loss'], margins)
            if 'a' in outs:
                check_acc('ragan score_a ' + t1, a[3], accs['score_a'], margins)
            if 'b' in outs:
                check_acc('ragan score_b ' + t1, a[5], accs['score_b'], margins)
            want = torch.tensor([SENT, 0.25, SENT, -1.5, SENT, 0.75, SENT])
            keep = [k for k in range(7) if not (k == 1 and 'l' in outs or k == 3 and 'a' in outs or k == 5 and 'b' in outs)]
            assert biteq(a[keep], want[keep]) and acc.guards_ok()
            p = part.get()
            # part: the N local d-terms added in order
            bounded('ragan part_a ' + t1, p[:HW], ref['qa'].v.view(-1), ref['qa'].tol().view(-1), margins)
            bounded('ragan part_b ' + t1, p[HW:], ref['qb'].v.view(-1), ref['qb'].tol().view(-1), margins)
            assert part.guards_ok() and sums.guards_ok()
        part.put(torch.cat([i['part_a'].view(-1), i['part_b'].view(-1)]))       # the second all-reduce, uploaded in the same way
        # stage 2: g = gcoef * (d - part * (1 / n_glob)); ga or gb may be null
        for outs in ('ab', 'a', 'b'):
            ga, gb = out_slab(dev, N, 1, H, W), out_slab(dev, N, 1, H, W, lead=3)
            kw = dict(base, stage=2)
            if 'a' in outs:
                kw['ga'] = ga.view()
            if 'b' in outs:
                kw['gb'] = gb.view()
            acc = Buf(dev, torch.tensor([0.25]))
            assert call(via, 'ragan', loss_acc=acc.ptr, **kw) == 0
            assert acc.untouched()                                   # stage 2 accumulates nothing
            for ch, sl, nm in (('a', ga, 'ga'), ('b', gb, 'gb')):
                if ch not in outs:
                    assert sl.untouched()
                    continue
                got = sl.nchw()
                ev_ok('ragan %s %s [%s]' % (nm, tag, outs), got[:, :1], ref[nm], margins)
                assert zeros_from(got, 1) and sl.outside_untouched()
        assert as_.untouched() and bs.untouched()


@gpu
@VIA
@pytest.mark.parametrize('ta,tb', K.RAGAN_T[1], ids=['ta%g-tb%g' % t for t in K.RAGAN_T[1]])
def test_ragan_form1_saturated_logits_stay_finite(ta, tb, via):
    """form 1 on relativistic logits of +-20 and +-100 (n_glob = N = 2, b = 0, so za = a - 0 and zb = -mean a): -log(1 - sigmoid + eps) at a saturated
    sigmoid is ill-conditioned, so no value is pinned here -- every word the three stages write is finite, every loss term lies in [-log(1 + eps),
    -log(eps)] up to the rounding of the sum and of logf, and the d-terms have the sign of their target"""
    import math
    dev = _gpu()
    N, H, W, eps = 2, 1, 4, K.RAGAN_EPS
    a = torch.tensor([[20.0, -20.0, 100.0, -100.0], [100.0, -100.0, 20.0, -20.0]]).view(N, 1, H, W)
    b = torch.zeros(N, 1, H, W)
    as_, bs = slab(dev, a, pad=9.0), slab(dev, b, pad=-9.0, lead=2)
    sums, part, acc = Buf(dev, n=2 * H * W), Buf(dev, n=2 * H * W), Buf(dev, torch.zeros(3))
    ga, gb = out_slab(dev, N, 1, H, W), out_slab(dev, N, 1, H, W, lead=3)
    base = dict(a=as_.view(), b=bs.view(), N=N, H=H, W=W, n_glob=N, form=1, ta=ta, tb=tb, coef=1.0, gcoef=1.0, eps=eps, score_coef=1.0, sums=sums.ptr,
                part=part.ptr)
    assert call(via, 'ragan', stage=0, **base) == 0
    assert call(via, 'ragan', stage=1, loss_acc=acc.ptr, score_a=acc.ptr + 4, score_b=acc.ptr + 8, **base) == 0
    assert call(via, 'ragan', stage=2, ga=ga.view(), gb=gb.view(), **base) == 0
    assert biteq(sums.get()[:4], torch.tensor([120.0, -120.0, 120.0, -120.0])) and biteq(sums.get()[4:], torch.zeros(4))
    terms = N * H * W * (1 + int(tb >= 0))
    lo, hi = -math.log(1.0 + eps), -math.log(eps)
    tiny = 4 * R.U32 * hi * terms                                    # s + eps rounded (1), logf 1 ulp (2), one to spare; the sum of at most `terms` such
    loss, sa, sb = (float(v) for v in acc.get())
    assert math.isfinite(loss) and terms * lo - tiny <= loss <= terms * hi + tiny, (loss, terms)
    assert 0.0 <= sa <= N * H * W and 0.0 <= sb <= N * H * W           # the scores are sums of sigmoids
    p = part.get()
    assert bool(torch.isfinite(p).all()) and bool((p[:4] <= 0).all() if ta > 0.5 else (p[:4] >= 0).all())
    assert bool((p[4:] == 0).all() if tb < 0 else ((p[4:] <= 0).all() if tb > 0.5 else (p[4:] >= 0).all()))
    for sl in (ga, gb):
        got = sl.nchw()
        assert bool(torch.isfinite(got).all()) and zeros_from(got, 1) and sl.outside_untouched()
    assert sums.guards_ok() and part.guards_ok() and acc.guards_ok() and as_.untouched() and bs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_grad_penalty / dasr_fill_scaled
@gpu
@VIA
@pytest.mark.parametrize('zero', [False, True], ids=['randn', 'all_zero'])
@pytest.mark.parametrize('C', K.PIX_C)
def test_grad_penalty(C, zero, via, margins):
    dev = _gpu()
    N = K.PIX_N
    for H, W in K.PIX_HW:
        i, ref = K.ref_gp(C, H, W, zero)
        gs = slab(dev, i['g'], pad=9.0)                              # the padding channels hold junk: only the C real ones are read
        part = Buf(dev, n=256)
        tag = 'C%d %dx%d zero %d %s' % (C, H, W, zero, via)
        base = dict(g=gs.view(), N=N, C=C, H=H, W=W, weight=K.GP_WEIGHT, part256=part.ptr)

        def finished(out3, acc, nrm, pen, fac, what, is_zero):
            o, a = out3.get(), acc.get()
            # the sum of squares: C products and adds per pixel thread, the wave and workgroup sums, the non-zero partials in order; sqrtf (1); nrm - 1
            # (1), * weight (1), * (nrm - 1) (1); 2 weight (nrm - 1) (1) / nrm (1) * (1 / world) (1); the add into the accumulator (1)
            for k, r in enumerate((nrm, pen, fac)):
                bounded('grad_penalty %s out3[%d] %s' % (what, k, tag), o[k:k + 1], r.v.view(1), r.tol().view(1), margins)
            bounded('grad_penalty %s loss_acc %s' % (what, tag), a[1:2], (0.25 + pen.v).view(1), pen.tol().view(1) + R.U32 * (0.25 + pen.v.abs()).view(1), margins)
            assert float(a[0]) == SENT and float(a[2]) == SENT and acc.guards_ok() and out3.guards_ok()
            if is_zero:
                assert float(o[0]) == 0.0 and float(o[1]) == K.GP_WEIGHT and float(o[2]) == 0.0
        # stage 0: everything in one call; out3[3] is not written
        out3, acc = Buf(dev, n=4), Buf(dev, torch.tensor([SENT, 0.25, SENT]))
        assert call(via, 'grad_penalty', out3=out3.ptr, loss_acc=acc.ptr + 4, stage=0, world=1, **base) == 0
        finished(out3, acc, ref['nrm'], ref['pen'], ref['fac'], 'stage 0', zero)
        assert float(out3.get()[3]) == SENT and part.guards_ok()
        # stage 1: the local sum of squares into out3[3], nothing else (loss_acc is not touched even when given)
        out3, acc = Buf(dev, n=4), Buf(dev, torch.tensor([SENT, 0.25, SENT]))
        assert call(via, 'grad_penalty', out3=out3.ptr, loss_acc=acc.ptr + 4, stage=1, world=2, **base) == 0
        o = out3.get()
        bounded('grad_penalty stage 1 out3[3] ' + tag, o[3:4], ref['s'].v.view(1), ref['s'].tol().view(1), margins)
        assert biteq(o[:3], torch.full((3,), SENT)) and acc.untouched() and out3.guards_ok()
        # the all-reduce: out3[3] is overwritten with the reference's local sum (rounded to fp32) plus the second rank's word, added in fp32 -- the word
        # the reference of stage 2 reads; stage 2 with world 2: nrm^2 = out3[3] / world^2
        word = torch.tensor([float(ref['s'].v)], dtype=torch.float32) + torch.tensor([i['other']])
        out3.t[G + 3:G + 4] = word.to(dev)
        part_before = part.t.clone()
        assert call(via, 'grad_penalty', out3=out3.ptr, loss_acc=acc.ptr + 4, stage=2, world=2, **base) == 0
        finished(out3, acc, ref['nrm2'], ref['pen2'], ref['fac2'], 'stage 2', False)      # (with the other rank's word the norm is not zero)
        assert biteq(out3.get()[3:4], word) and biteq(part.t, part_before) and gs.untouched()


@gpu
@VIA
@pytest.mark.parametrize('C', K.PIX_C + [22])
def test_fill_scaled(C, via):
    """factor * scalar[0], one fp32 product, on the C real channels; zero on the padding channels of the ceil(C / 16) planes"""
    dev = _gpu()
    N = K.PIX_N
    factor = R.f32(1.0 / 70.0)
    for H, W in K.PIX_HW:
        sc = Buf(dev, torch.tensor([SENT, -2.7182817, SENT]))
        xs = out_slab(dev, N, C, H, W)
        assert call(via, 'fill_scaled', x=xs.view(), N=N, C=C, H=H, W=W, scalar=sc.ptr + 4, factor=factor) == 0
        got = xs.nchw()
        want = (torch.tensor(factor) * torch.tensor(-2.7182817)).expand(N, C, H, W)
        assert biteq(got[:, :C], want) and zeros_from(got, C) and xs.outside_untouched() and sc.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# argument checks: each returns DASR_EINVAL before any launch and leaves every slab and buffer as it was
@gpu
@VIA
def test_argument_checks(via):
    dev = _gpu()
    N, C, H, W = 2, 5, 5, 7
    s = [out_slab(dev, N, C, H, W, lead=k) for k in (1, 2, 3, 1)]
    bufs = [Buf(dev, n=256 + 8) for _ in range(6)]                   # (part256 of dasr_grad_penalty is the largest)
    v, b = [t.view() for t in s], [t.ptr for t in bufs]
    dims = dict(N=N, C=C, H=H, W=W)
    degenerate = [dict(N=0), dict(C=0), dict(C=-1), dict(H=0), dict(W=0), dict(H=-1)]
    # InstanceNorm group (stats of the forward may be null; the kernels that divide by slope refuse slope <= 0)
    ok = {'inorm_lrelu_fwd': dict(x=v[0], eps=1e-5, slope=0.2, y=v[1], stats=b[0], **dims),
          'inorm_lrelu_bwd': dict(a=v[0], ga=v[1], slope=0.2, stats=b[0], gx=v[2], **dims),
          'inorm_lrelu_jvp': dict(a=v[0], t=v[1], slope=0.2, stats=b[0], out=v[2], **dims),
          'inorm_second': dict(a=v[0], t=v[1], ga=v[2], slope=0.2, stats=b[0], out=v[3], accumulate=0, **dims)}
    bad = {'inorm_lrelu_fwd': [dict(x=None), dict(y=None)],
           'inorm_lrelu_bwd': [dict(a=None), dict(ga=None), dict(gx=None), dict(stats=None), dict(slope=0.0), dict(slope=-0.2)],
           'inorm_lrelu_jvp': [dict(a=None), dict(t=None), dict(out=None), dict(stats=None), dict(slope=0.0), dict(slope=-0.2)],
           'inorm_second': [dict(a=None), dict(t=None), dict(ga=None), dict(out=None), dict(stats=None), dict(slope=0.0), dict(slope=-0.2)]}
    # BatchNorm group
    bn = dict(group=2, slope=0.2, gamma=b[1], beta=b[2], stats=b[0], **dims)
    ok.update({'bnorm_lrelu_fwd': dict(bn, x=v[0], eps=1e-5, y=v[1]),
               'bnorm_lrelu_bwd': dict(bn, x=v[0], ga=v[1], gx=v[2], dgamma=b[3], dbeta=b[4], pscale=1.0),
               'bnorm_lrelu_jvp': dict(bn, x=v[0], t=v[1], out=v[2]),
               'bnorm_second': dict(bn, x=v[0], t=v[1], ga=v[2], out=v[3], accumulate=0, dgamma=b[3], pscale=1.0)})
    common = [dict(group=0), dict(group=-1), dict(gamma=None), dict(beta=None), dict(stats=None), dict(x=None)]
    bad.update({'bnorm_lrelu_fwd': common + [dict(y=None)],
                'bnorm_lrelu_bwd': common + [dict(ga=None), dict(gx=None), dict(dgamma=None), dict(dbeta=None)],      # dgamma / dbeta: both or none
                'bnorm_lrelu_jvp': common + [dict(t=None), dict(out=None)],
                'bnorm_second': common + [dict(t=None), dict(ga=None), dict(out=None)]})
    ok['bnorm_running'] = dict(stats=b[0], g=0, C=C, count=70, momentum=0.1, running_mean=b[3], running_var=b[4], num_batches_tracked=b[5])
    bad['bnorm_running'] = [dict(stats=None), dict(g=-1), dict(C=0), dict(count=0), dict(running_mean=None), dict(running_var=None)]
    # losses
    ok['gan_loss'] = dict(x=v[0], gan_type=0, target=1.0, coef=1.0, gcoef=1.0, loss_acc=b[5], score_acc=b[5] + 4, score_coef=1.0, grad=v[1], **dims)
    bad['gan_loss'] = [dict(x=None), dict(C=0), dict(C=-1), dict(C=17), dict(gan_type=3), dict(gan_type=-1), dict(N=0), dict(H=0)]
    ok['ragan'] = dict(a=v[0], b=v[1], N=N, H=H, W=W, stage=1, n_glob=N, form=0, ta=1.0, tb=0.0, coef=1.0, gcoef=1.0, eps=1e-8, sums=b[0], part=b[1],
                       loss_acc=b[5], score_a=b[5] + 4, score_b=b[5] + 8, score_coef=1.0, ga=v[2], gb=v[3])
    bad['ragan'] = [dict(a=None), dict(b=None), dict(N=0), dict(H=0), dict(W=0), dict(n_glob=N - 1), dict(stage=3), dict(stage=-1), dict(form=4),
                    dict(form=-1), dict(sums=None), dict(part=None)]
    ok['grad_penalty'] = dict(g=v[0], weight=10.0, part256=b[0], out3=b[1], loss_acc=b[5], stage=0, world=1, **dims)
    bad['grad_penalty'] = [dict(g=None), dict(part256=None), dict(out3=None), dict(C=17), dict(C=0), dict(N=0), dict(H=0), dict(W=0), dict(stage=3),
                           dict(stage=-1), dict(stage=0, world=2)] + ([dict(world=0)] if via == 'abi' else [])     # (a recorded op reads world 0 as 1)
    ok['fill_scaled'] = dict(x=v[0], scalar=b[0], factor=1.0, **dims)
    bad['fill_scaled'] = [dict(x=None), dict(scalar=None), dict(N=0), dict(C=0), dict(H=0), dict(W=0)]
    for name, cases in bad.items():
        for d in cases + (degenerate if name.startswith(('inorm', 'bnorm_lrelu', 'bnorm_second')) else []):
            assert call(via, name, **dict(ok[name], **d)) == EINVAL, (name, d)
    assert all(t.untouched() for t in s) and all(t.untouched() for t in bufs)
    # ... and each call the bad ones were derived from is accepted as it stands (on the same slabs, last: it writes), so that every refusal above is
    # owed to the one argument it changes
    for name, kw in ok.items():
        assert call(via, name, **kw) == 0, name
    assert all(t.outside_untouched() for t in s) and all(t.guards_ok() for t in bufs)
