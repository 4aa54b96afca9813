"""Shapes and seeded inputs of the LPIPS-layer, PReLU-slope-gradient and crop-gather kernel tests: tests/test_gpu_lpips_prelu.py runs the kernels on
them, tests/test_blocked_ref.py shows on a machine without a GPU that stock fp32 arithmetic meets the bounds on exactly these inputs and that the
listed wrong variants do not.  Every function ref_* returns (inputs, {name: Ev}); `wrong=` selects a deliberately wrong variant of the reference."""
import functools

import torch

from oracle import blocked_ref as R

N = 2


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(base, *dims):
    s = base
    for d in dims:
        s = s * 31 + d
    return s


# ---- dasr_lpips_s2d -----------------------------------------------------------------------------------------------------------------------------
SCALE4, SHIFT4 = [R.f32(v) for v in (2.1, 2.2, 2.3, 0.0)], [R.f32(v) for v in (-1.0, -0.9, -0.8, 0.0)]
# (H, W, symmetry code): the four codes without a transpose on a non-square image, all eight on a square one
S2D = [(8, 12, xf) for xf in (0, 2, 4, 6)] + [(12, 12, xf) for xf in range(8)]
QUARTER_TURNS = (3, 5)                    # the codes that are not their own inverse


@functools.lru_cache(maxsize=None)
def s2d_inputs(H, W):
    g = gen(_seed(400, H, W))
    Hs, Ws = (H + 4) // 4, (W + 4) // 4
    return dict(x=torch.rand(N, 3, H, W, generator=g), gy=torch.randn(N, 48, Hs, Ws, generator=g), x0=torch.randn(N, 3, H, W, generator=g))


def ref_s2d_fwd(H, W, xf, wrong=None):
    i = s2d_inputs(H, W)
    return i, dict(y=R.lpips_s2d(i['x'], SCALE4, SHIFT4, xf, wrong))


def ref_s2d_adj(H, W, xf, wrong=None):
    i = s2d_inputs(H, W)
    return i, dict(x=R.lpips_s2d_adj(i['gy'], i['x0'], SCALE4, xf, wrong))


# ---- dasr_maxpool3s2 / dasr_maxpool3s2_bwd ----------------------------------------------------------------------------------------------------
POOL_C = [16, 20, 40]
# one window; an even size whose last row and column lie in no window (4: one window, 8 x 6: 3 x 2); 3 x 4 windows, every pixel covered
POOL_HW = [(3, 3), (4, 4), (8, 6), (7, 9)]
POOL_VALUES = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.5])


@functools.lru_cache(maxsize=None)
def pool_inputs(C, H, W):
    """x from five values (ties everywhere), finite and far above -3.4e38 (the kernel's contract); the first window of channel 0 all zero, of channel
    1 all negative; the padding channels zero in x, gy and gx0.  Tensors hold whole planes: [N][16 K][H][W]."""
    g = gen(_seed(410, C, H, W))
    Cp = R.planes(C) * 16
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    x = POOL_VALUES[torch.randint(0, 5, (N, Cp, H, W), generator=g)]
    x[:, 0, :3, :3] = 0.0
    x[:, 1, :3, :3] = POOL_VALUES[torch.randint(0, 2, (N, 3, 3), generator=g)]
    gy, gx0 = torch.randn(N, Cp, Ho, Wo, generator=g), torch.randn(N, Cp, H, W, generator=g)
    x[:, C:], gy[:, C:], gx0[:, C:] = 0.0, 0.0, 0.0
    return dict(x=x, gy=gy, gx0=gx0)


def ref_pool_fwd(C, H, W, wrong=None):
    i = pool_inputs(C, H, W)
    return i, dict(y=R.Ev(R.maxpool3s2(i['x'])[0]))


def ref_pool_bwd(C, H, W, relu, acc, wrong=None):
    i = pool_inputs(C, H, W)
    return i, dict(gx=R.maxpool3s2_bwd(i['x'], i['gy'], relu, i['gx0'] if acc else None, wrong))


# ---- dasr_lpips_head ------------------------------------------------------------------------------------------------------------------------------
HEAD_C = [16, 48, 64]
HEAD_HW = (9, 15)                         # N H W = 270 threads: two workgroups, the second partial
HEAD_IMAGES, PAIR_OFF = 5, 3              # f0 = images 0, 1; f1 = images 3, 4; image 2 is never read (the GPU test fills it with NaN)
HEAD_EPS = R.f32(1e-10)
HEAD_ACC0 = 0.25
# planted pixels (n, y, x): f0 all zero and f1 not; both all zero; only f1 zero; f0 of the size of eps (the only place where eps shows in fp32)
PIX_F0_ZERO, PIX_BOTH_ZERO, PIX_F1_ZERO, PIX_TINY = (0, 0, 0), (0, 4, 7), (1, 8, 14), (1, 2, 3)


def head_coefs():
    cnt = N * HEAD_HW[0] * HEAD_HW[1]
    return R.f32(1.0 / cnt), R.f32(0.7 / cnt)      # coef, gcoef


@functools.lru_cache(maxsize=None)
def head_inputs(C):
    """signed features (the kernel takes them) with exact +0 and -0 entries; non-negative lin weights, one of them zero"""
    H, W = HEAD_HW
    g = gen(_seed(420, C))
    f = torch.randn(HEAD_IMAGES, C, H, W, generator=g)
    f[:, ::5, 1, 1], f[:, 1::5, 1, 1] = 0.0, -0.0
    for (n, y, x), z0, z1 in ((PIX_F0_ZERO, True, False), (PIX_BOTH_ZERO, True, True), (PIX_F1_ZERO, False, True)):
        if z0:
            f[n, :, y, x] = 0.0
        if z1:
            f[n + PAIR_OFF, :, y, x] = 0.0
    n, y, x = PIX_TINY
    f[n, :, y, x] *= 1e-9
    lin = torch.rand(C, generator=g)
    lin[3] = 0.0
    return dict(f=f, lin=lin)


def ref_head(C, relu, wrong=None):
    i = head_inputs(C)
    val, g0 = R.lpips_head(i['f'][:N], i['f'][PAIR_OFF:PAIR_OFF + N], i['lin'], HEAD_EPS, head_coefs()[1], relu, wrong)
    return i, dict(val=val, g0=g0)


def head_acc(C, relu=0):
    """(value, bound) of the loss accumulator: one term per thread, then the workgroup and grid chain (R.acc_sum)"""
    H, W = HEAD_HW
    return R.acc_sum(ref_head(C, relu)[1]['val'], head_coefs()[0], HEAD_ACC0, 0, (N * H * W + 255) // 256)


# ---- dasr_prelu_grad / dasr_prelu_grad_f16 / dasr_prelu_final -----------------------------------------------------------------------------------
# (C, H, W): padding channels; whole planes; 2 x 4 x 96 x 96 x 4 = 294 912 vector loads > 1024 x 256: the grid-stride loop takes a second pass
PRELU = [(20, 5, 7), (64, 10, 12), (64, 96, 96)]
PRELU_A, PRELU_SCALE, PRESCALE = R.f32(0.2), 0.5, 1024.0


@functools.lru_cache(maxsize=None)
def prelu_inputs(C, H, W, kind):
    """y with exact zeros of both signs; f16: y and gx rounded to f16, gx pre-scaled by the power of two PRESCALE.  Whole planes, padding zero."""
    g = gen(_seed(430, C, H, W))
    Cp = R.planes(C) * 16
    y, gx = torch.randn(N, Cp, H, W, generator=g), torch.randn(N, Cp, H, W, generator=g)
    y[:, ::3, 1, 2], y[:, 1::3, 1, 2] = 0.0, -0.0
    y[:, C:], gx[:, C:] = 0.0, 0.0
    if kind == 'f16':
        y, gx = R.r16(y, 'f16'), R.r16(gx * PRESCALE, 'f16')
    return dict(y=y, gx=gx)


def ref_prelu(C, H, W, kind, wrong=None):
    i = prelu_inputs(C, H, W, kind)
    scale = PRELU_SCALE / PRESCALE if kind == 'f16' else PRELU_SCALE     # (a power of two: the product is exact on either route)
    return i, dict(d=R.prelu_grad(i['y'], i['gx'], PRELU_A, scale, wrong))


FINAL_NB, FINAL_COUNT, FINAL_GAP = [1, 256, 257, 700], 3, 5
FINAL_SLOPES = [0.25, 0.1, 0.4]


@functools.lru_cache(maxsize=None)
def final_inputs(nb):
    return dict(partial=torch.randn(FINAL_COUNT, nb, generator=gen(_seed(440, nb))))


def ref_prelu_final(nb, wrong=None):
    i = final_inputs(nb)
    return i, dict(d=R.prelu_final(i['partial'], FINAL_SLOPES, PRELU_SCALE, wrong))


# ---- dasr_gather_crops ----------------------------------------------------------------------------------------------------------------------------
CROP_SIZE, CROP_C = 7, 3


@functools.lru_cache(maxsize=None)
def crop_images():
    g = gen(450)
    return dict(a=torch.rand(3, 22, 20, generator=g), b=torch.rand(1, 9, 11, generator=g), c=torch.rand(1, 12, 10, generator=g))


def _desc(img, vH, vW, y0, x0, flags):
    return dict(img=crop_images()[img], name=img, vH=vH, vW=vW, y0=y0, x0=x0, flags=flags)


def crop_descs(launch):
    """'all': eight descriptors, every flag code once, three- and one-channel images of different sizes; no resize, the non-dyadic down-scale
    22 x 20 -> 10 x 12, the up-scale -> 33 x 25 (windows at the first and at the last rows / columns: the edge clamp), vH == H with vW != W.
    'edge': two windows that hang over the edge of the (resized / plain) view -- zero there, nothing read."""
    if launch == 'all':
        return [_desc('a', 22, 20, 3, 4, 0), _desc('b', 9, 11, 2, 4, 1), _desc('a', 10, 12, 3, 5, 2), _desc('a', 33, 25, 0, 0, 3),
                _desc('a', 33, 25, 26, 18, 4), _desc('c', 12, 15, 2, 8, 5), _desc('a', 10, 12, 0, 0, 6), _desc('b', 9, 11, 2, 4, 7)]
    return [_desc('a', 10, 12, 6, 8, 5), _desc('a', 22, 20, -2, 17, 3)]


def ref_gather(launch, wrong=None):
    descs = crop_descs(launch)
    dst, exact = R.gather_crops(descs, CROP_C, CROP_SIZE, wrong)
    return dict(descs=descs, exact=exact), dict(dst=dst)


# ---- (id, fn, args, the `wrong` variants that must leave the bound on these inputs) ----------------------------------------------------------------
def evals():
    for H, W, xf in S2D:
        s = '%dx%d-xf%d' % (H, W, xf)
        yield 's2d_fwd-' + s, ref_s2d_fwd, (H, W, xf), ['border_shift', 'block_xy']
        yield 's2d_adj-' + s, ref_s2d_adj, (H, W, xf), ['adj_forward_map'] if xf in QUARTER_TURNS else []
    for C in POOL_C:
        for H, W in POOL_HW:
            s = 'C%d-%dx%d' % (C, H, W)
            yield 'pool_fwd-' + s, ref_pool_fwd, (C, H, W), []
            for relu in (0, 1):
                for acc in (0, 1):
                    yield 'pool_bwd-relu%d-acc%d-%s' % (relu, acc, s), ref_pool_bwd, (C, H, W, relu, acc), ['last_max'] + (['relu_ge'] if relu else [])
    for C in HEAD_C:
        for relu in (0, 1):
            yield 'head-C%d-relu%d' % (C, relu), ref_head, (C, relu), ['eps_in_sqrt', 'no_x0k2', 'k2_s0cubed'] + (['relu_f1'] if relu else [])
    for C, H, W in PRELU:
        for kind in ('f32', 'f16'):
            yield 'prelu-%s-C%d-%dx%d' % (kind, C, H, W), ref_prelu, (C, H, W, kind), ['div_a', 'skip_plane']
    for nb in FINAL_NB:
        yield 'prelu_final-nb%d' % nb, ref_prelu_final, (nb,), ['div_a']
    yield 'gather-all', ref_gather, ('all',), ['flip_order', 'no_half_pixel', 'no_clamp']
    yield 'gather-edge', ref_gather, ('edge',), []


WRONG = ['border_shift', 'block_xy', 'adj_forward_map', 'last_max', 'relu_ge', 'eps_in_sqrt', 'no_x0k2', 'k2_s0cubed', 'relu_f1', 'div_a', 'skip_plane',
         'flip_order', 'no_half_pixel', 'no_clamp']
