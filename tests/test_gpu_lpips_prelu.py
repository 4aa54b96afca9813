"""GPU parity tests of the LPIPS layers of csrc/lpips.hip (dasr_lpips_s2d with its eight symmetries, dasr_maxpool3s2 and its backward, dasr_lpips_head),
the PReLU slope-gradient kernels of csrc/gan.hip (dasr_prelu_grad, dasr_prelu_grad_f16, dasr_prelu_final) and the fp32 batch assembler
dasr_gather_crops of csrc/misc.hip, against the fp64 references of oracle/blocked_ref.py (themselves held to stock torch by tests/test_blocked_ref.py).

Set-up as in tests/test_gpu_elementwise.py, whose machinery (Slab, Buf, call, ev_ok) this file shares with tests/test_gpu_norm_gan.py: every blocked tensor is plane(s) p0 > 0 of
a wider sentinel-filled slab (n_stride != K * cb_stride), everything outside the written view must hold the sentinel bit for bit afterwards and inputs
must be untouched; flat buffers have sentinel words in front and behind; every case through the ctypes entry point (via = abi) and as a recorded op
through dasr_run_ops (via = op; dasr_gather_crops has no op kind).  Shapes and seeded inputs come from oracle/lpips_prelu_cases.py:
tests/test_blocked_ref.py shows on the same inputs that stock fp32 arithmetic meets every bound applied here and that a list of wrong variants does not.

What is asserted: |got - ref| <= Ev.tol() ELEMENTWISE, the bound carried along the kernel's own expression (one rounding per operation, a fused
multiply-add counted as two, sqrtf and the divisions one each, reductions along the kernel's chain); data movement and results documented as exact
bit for bit.  The comment beside each comparison names the chain.  No tolerance here is tuned to a GPU run: the margins log records the slack."""
import ctypes
import functools

import pytest
import torch

from oracle import blocked_ref as R
from oracle import lpips_prelu_cases as K
from test_gpu_elementwise import EINVAL, SENT, VIA, Buf, Slab, _gpu, biteq, call, ev_ok, gpu

N = K.N


@functools.lru_cache(maxsize=None)
def ref_of(fn, *args):
    """the fp64 reference of a case, computed once and shared by both routes"""
    return fn(*args)


def bits0(t):
    """every element is +0, bit for bit"""
    return biteq(t, torch.zeros_like(t))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_lpips_s2d.  Contract (dasr_hip.h): mode 0 reads channels 0..2 of plane 0 of x and writes all 16 slots of 3 planes of y, exact +0 where the
# padded grid lies outside the image; mode 1 adds into channels 0..2 of plane 0 of x and leaves channels 3..15 and every other plane alone.
def _s2d_slabs(dev, H, W, x, gy=None):
    Hs, Ws = (H + 4) // 4, (W + 4) // 4
    xs = Slab(dev, 'f32', N, 1, H, W, R.pack(x, 'f32', pad=SENT))        # channels 3..15 of the image plane hold the (finite) sentinel
    ys = Slab(dev, 'f32', N, 3, Hs, Ws, None if gy is None else R.pack(gy), lead=2)
    return xs, ys


@gpu
@VIA
@pytest.mark.parametrize('H,W,xf', K.S2D, ids=['%dx%d-xf%d' % c for c in K.S2D])
def test_lpips_s2d_forward(H, W, xf, via, margins):
    dev = _gpu()
    from dasr_amd.dsn_model import symmetry_code
    i, ref = ref_of(K.ref_s2d_fwd, H, W, xf)
    xs, ys = _s2d_slabs(dev, H, W, i['x'])
    assert call(via, 'lpips_s2d', x=xs.view(), N=N, H=H, W=W, scale4=K.SCALE4, shift4=K.SHIFT4, y=ys.view(), mode=xf << 4) == 0
    got = ys.nchw()
    # scale * x (1) + shift (1), read through the reference's index map of the symmetry
    ev_ok('lpips_s2d fwd %dx%d xf%d %s' % (H, W, xf, via), got, ref['y'], margins)
    border = (ref['y'].v == 0) & (ref['y'].e == 0)
    assert int(border.sum()) == N * 3 * ((H + 4) * (W + 4) - H * W) and bits0(got[border])      # the conv's zero padding: +0, bit for bit
    assert not bool((got == SENT).any()) and ys.outside_untouched() and xs.untouched()
    # the same against torch.rot90 / torch.flip, through the trainer's own translation of a draw into a code
    hit = 0
    for k_rot, rows, cols in [(k, r, c) for k in range(4) for r in (0, 1) for c in (0, 1)]:
        if symmetry_code(k_rot, rows, cols) != xf:
            continue
        hit += 1
        t = torch.rot90(i['x'].double(), k_rot, [2, 3])
        t = torch.flip(t, (2,)) if rows else t
        t = torch.flip(t, (3,)) if cols else t
        want = R.lpips_s2d(t, K.SCALE4, K.SHIFT4, 0)
        assert bool(((got.double() - want.v).abs() <= want.tol()).all()), (k_rot, rows, cols)
    assert hit == 2                                                      # every symmetry of the square is two of the sixteen (rotation, flip, flip) draws


@gpu
@VIA
@pytest.mark.parametrize('H,W,xf', K.S2D, ids=['%dx%d-xf%d' % c for c in K.S2D])
def test_lpips_s2d_adjoint(H, W, xf, via, margins):
    dev = _gpu()
    i, ref = ref_of(K.ref_s2d_adj, H, W, xf)
    xs, ys = _s2d_slabs(dev, H, W, i['x0'], i['gy'])
    assert call(via, 'lpips_s2d', x=xs.view(), N=N, H=H, W=W, scale4=K.SCALE4, shift4=K.SHIFT4, y=ys.view(), mode=1 | xf << 4) == 0
    got = xs.nchw()
    # scale * gy (1), + x (1), routed back through the inverse of the symmetry's index map
    ev_ok('lpips_s2d adj %dx%d xf%d %s' % (H, W, xf, via), got[:, :3], ref['x'], margins)
    assert biteq(got[:, 3:], torch.full_like(got[:, 3:], SENT)) and xs.outside_untouched() and ys.untouched()
    # <s2d_T(x) - shift part, gy> == <x, adj_T(gy)> on the kernel's own outputs: with shift 0 and onto x0 = 0 either side holds ONE rounding per
    # element (the product with scale; adding zero is exact), so the two inner products, taken in fp64, differ by at most u (sum |y gy| + sum |x adj|)
    zero4 = [0.0] * 4
    xl, yl = _s2d_slabs(dev, H, W, i['x'])
    assert call(via, 'lpips_s2d', x=xl.view(), N=N, H=H, W=W, scale4=K.SCALE4, shift4=zero4, y=yl.view(), mode=xf << 4) == 0
    xa, ya = _s2d_slabs(dev, H, W, torch.zeros_like(i['x0']), i['gy'])
    assert call(via, 'lpips_s2d', x=xa.view(), N=N, H=H, W=W, scale4=K.SCALE4, shift4=zero4, y=ya.view(), mode=1 | xf << 4) == 0
    ylin, adj, gy, x = yl.nchw().double(), xa.nchw()[:, :3].double(), i['gy'].double(), i['x'].double()
    lhs, rhs, slack = float((ylin * gy).sum()), float((x * adj).sum()), R.U32 * float((ylin * gy).abs().sum() + (x * adj).abs().sum())
    margins('elementwise lpips_s2d adjoint identity %dx%d xf%d %s: |lhs - rhs| / bound %.3f' % (H, W, xf, via, abs(lhs - rhs) / slack))
    assert abs(lhs - rhs) <= slack


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_maxpool3s2 / dasr_maxpool3s2_bwd.  Contract (dasr_hip.h): whole 16-channel planes, the padding channels like real ones -- zero in, zero out;
# the first maximum in scan order wins a tie; inputs finite and above -3.4e38; the backward writes EVERY pixel of gx, exact zero (accumulate: the old
# value) in a row / column no window covers.
def _whole(dev, t, lead=1):
    Nn, Cp, H, W = t.shape
    return Slab(dev, 'f32', Nn, Cp // 16, H, W, R.pack(t), lead=lead)


POOL = [(C, hw) for C in K.POOL_C for hw in K.POOL_HW]
POOL_IDS = ['C%d-%dx%d' % (C, hw[0], hw[1]) for C, hw in POOL]


@gpu
@VIA
@pytest.mark.parametrize('C,hw', POOL, ids=POOL_IDS)
def test_maxpool3s2_forward(C, hw, via):
    dev = _gpu()
    H, W = hw
    i, ref = ref_of(K.ref_pool_fwd, C, H, W)
    xs = _whole(dev, i['x'])
    ys = Slab(dev, 'f32', N, xs.K, (H - 3) // 2 + 1, (W - 3) // 2 + 1, None, lead=2)
    assert call(via, 'maxpool3s2', x=xs.view(), N=N, C=C, H=H, W=W, y=ys.view()) == 0
    got = ys.nchw()
    assert torch.equal(got.double(), ref['y'].v)                         # a maximum is moved, not computed: equal by value
    assert bits0(got[:, C:]) and ys.outside_untouched() and xs.untouched()


@gpu
@VIA
@pytest.mark.parametrize('relu,acc', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('C,hw', POOL, ids=POOL_IDS)
def test_maxpool3s2_backward(C, hw, relu, acc, via, margins):
    dev = _gpu()
    H, W = hw
    i, ref = ref_of(K.ref_pool_bwd, C, H, W, relu, acc)
    xs, gs = _whole(dev, i['x']), _whole(dev, i['gy'], lead=2)
    os_ = _whole(dev, i['gx0'], lead=3) if acc else Slab(dev, 'f32', N, xs.K, H, W, None, lead=3)
    assert call(via, 'maxpool3s2_bwd', x=xs.view(), gy=gs.view(), N=N, C=C, H=H, W=W, gx=os_.view(), relu_mask=relu, accumulate=acc) == 0
    got = os_.nchw()
    # the gradients of the (at most 2 x 2) windows whose first maximum the pixel is: the first add is to zero, three more, one for accumulate
    ev_ok('maxpool3s2_bwd C%d %dx%d relu %d acc %d %s' % (C, H, W, relu, acc, via), got, ref['gx'], margins)
    Hc, Wc = 2 * ((H - 3) // 2) + 3, 2 * ((W - 3) // 2) + 3                # rows / columns covered by a window
    base = i['gx0'] if acc else torch.zeros_like(got)                    # the rest: exact zero, or what gx held
    assert biteq(got[:, :, Hc:], base[:, :, Hc:]) and biteq(got[:, :, :, Wc:], base[:, :, :, Wc:])
    assert (Hc < H or Wc < W) == (hw in ((4, 4), (8, 6)))
    if relu:                                                             # nothing flows into x <= 0 (the windows that are all zero or all negative)
        dead = i['x'] <= 0
        assert biteq(got[dead], i['gx0'][dead] if acc else torch.zeros_like(got[dead]))
    assert (biteq(got[:, C:], i['gx0'][:, C:]) if acc else bits0(got[:, C:]))
    assert os_.outside_untouched() and xs.untouched() and gs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_lpips_head.  Contract (dasr_hip.h): images n and n + pair_off of f are compared, nothing else of f is read; signed features are accepted; at a
# pixel whose f0 is all zero the derivative of the norm is taken as 0 (k2 = 0): g0 stays finite; g0 is written on all C channels of N images.
@gpu
@VIA
@pytest.mark.parametrize('with_g0', [1, 0], ids=['g0', 'nog0'])
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('C', K.HEAD_C)
def test_lpips_head(C, relu, with_g0, via, margins):
    dev = _gpu()
    H, W = K.HEAD_HW
    i, ref = ref_of(K.ref_head, C, relu)
    coef, gcoef = K.head_coefs()
    Kp = C // 16
    fs = Slab(dev, 'f32', K.HEAD_IMAGES, Kp, H, W, R.pack(i['f']))
    fs.b.t[K.PAIR_OFF - 1, fs.p0:fs.p0 + Kp] = float('nan')              # the image between the two stacks: a read of it would poison the result
    fs.before = fs.b.t.cpu().clone()
    lin = Buf(dev, i['lin'])
    f0 = i['f'][:N]
    for n, y, x in (K.PIX_F0_ZERO, K.PIX_BOTH_ZERO):
        assert bool((f0[n, :, y, x] == 0).all())
    runs = []
    for _ in range(2):
        acc = Buf(dev, torch.tensor([K.HEAD_ACC0]))
        gs = Slab(dev, 'f32', N, Kp, H, W, None, lead=2)
        kw = dict(f=fs.view(), pair_off=K.PAIR_OFF, N=N, C=C, H=H, W=W, lin=lin.ptr, eps=K.HEAD_EPS, coef=coef, gcoef=gcoef, loss_acc=acc.ptr,
                  relu_mask=relu)
        if with_g0:
            kw['g0'] = gs.view()
        assert call(via, 'lpips_head', **kw) == 0
        runs.append((acc.get(), gs.get()))
        assert acc.guards_ok() and fs.untouched() and lin.untouched()
        assert gs.outside_untouched() if with_g0 else gs.untouched()
    tag = 'C%d relu %d g0 %d %s' % (C, relu, with_g0, via)
    # the accumulator: per pixel the chain of lpips_head (sums of C terms, sqrtf, the divisions), then one term per thread through the workgroup and
    # grid chain of test_l1_diff (R.acc_sum), two workgroups, onto a non-zero accumulator
    want, bound = K.head_acc(C, relu)
    err = abs(float(runs[0][0][0].double()) - want)
    margins('elementwise lpips_head %s loss: |err| / bound %.3f' % (tag, err / bound))
    assert err <= bound, (err, bound)
    assert biteq(runs[0][0], runs[1][0]) and biteq(runs[0][1], runs[1][1])            # a fixed order of summation: the same bits on a second run
    if with_g0:
        got = R.unpack(runs[0][1])
        # d = f0 i0 - f1 i1 (3, behind the two norm chains), ((2 w) d) i0 (2) - f0 k2 (k2: the dot chain, r0 s0 s0, the division), * gcoef (1)
        ev_ok('lpips_head %s g0' % tag, got, ref['g0'], margins)
        n, y, x = K.PIX_F0_ZERO
        assert bool(torch.isfinite(got[n, :, y, x]).all()) and (relu or float(got[n, :, y, x].abs().max()) > 1.0)
        n, y, x = K.PIX_BOTH_ZERO
        assert bool((got[n, :, y, x] == 0).all())
        if relu:
            assert bool((got[f0 <= 0] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_prelu_grad / dasr_prelu_grad_f16 / dasr_prelu_final.  Contract (dasr_hip.h): dst = scale * sum_{y <= 0} gx y / a^2 over whole planes (padding
# channels zero in); scratch256 holds 1024 floats, of which the first min(1024, ceil(vector loads / 256)) are written.
PRELU_CASES = [(c, kind) for c in K.PRELU for kind in ('f32', 'f16')]


@gpu
@VIA
@pytest.mark.parametrize('case,kind', PRELU_CASES, ids=['%s-C%d-%dx%d' % ((k,) + c) for c, k in PRELU_CASES])
def test_prelu_grad(case, kind, via, margins):
    dev = _gpu()
    C, H, W = case
    i, ref = ref_of(K.ref_prelu, C, H, W, kind)
    Kp = R.planes(C)
    ys = Slab(dev, kind, N, Kp, H, W, R.pack(i['y'], kind))
    gs = Slab(dev, kind, N, Kp, H, W, R.pack(i['gx'], kind), lead=2)
    slope, scratch, dst = Buf(dev, torch.tensor([K.PRELU_A])), Buf(dev, n=1024), Buf(dev, n=1)
    kw = dict(y=ys.view(), gx=gs.view(), N=N, C=C, H=H, W=W, slope=slope.ptr, scratch256=scratch.ptr, dst=dst.ptr)
    if kind == 'f32':
        kw['scale'] = K.PRELU_SCALE
    elif via == 'abi':                    # the caller folds 1 / pre-scale into scale ...
        kw['scale'] = K.PRELU_SCALE / K.PRESCALE
    else:                                 # ... the recorded op carries it in its own slot (both powers of two: the same fp32 product)
        kw.update(scale=K.PRELU_SCALE, inv_prescale=1.0 / K.PRESCALE)
    assert call(via, 'prelu_grad' if kind == 'f32' else 'prelu_grad_f16', **kw) == 0
    # each term rounded to fp32 once, the per-thread sums in double, their cast and the workgroup tree (10), the same again over the partials (10),
    # scale * tot (1), a * a (1), the division (1) -- relative to sum |terms|, not to the (cancelling) total
    ev_ok('prelu_grad %s C%d %dx%d %s' % (kind, C, H, W, via), dst.get()[0], ref['d'], margins)
    vec = N * Kp * H * W * 4
    nb = min((vec + 255) // 256, 1024)
    assert (nb == 1024) == (case == K.PRELU[-1]) and (vec > 1024 * 256) == (case == K.PRELU[-1])     # only the last case needs the grid-stride loop
    sc = scratch.get()
    assert biteq(sc[nb:], torch.full_like(sc[nb:], SENT)) and bool(torch.isfinite(sc[:nb]).all()) and scratch.guards_ok()
    assert dst.guards_ok() and slope.untouched() and ys.untouched() and gs.untouched()


@gpu
@VIA
@pytest.mark.parametrize('nb', K.FINAL_NB)
def test_prelu_final(nb, via, margins):
    dev = _gpu()
    i, ref = ref_of(K.ref_prelu_final, nb)
    stride, cnt = nb + K.FINAL_GAP, K.FINAL_COUNT
    rows = torch.full((cnt, stride), SENT)                               # the gaps between the rows hold a finite value that must not be read
    rows[:, :nb] = i['partial']
    part, slopes, dst = Buf(dev, rows), Buf(dev, torch.tensor(K.FINAL_SLOPES)), Buf(dev, n=cnt)
    sp = torch.tensor([slopes.ptr + 4 * k for k in range(cnt)], dtype=torch.int64, device=dev)
    dp = torch.tensor([dst.ptr + 4 * k for k in range(cnt)], dtype=torch.int64, device=dev)
    assert call(via, 'prelu_final', partial=part.ptr, nblocks=nb, stride=stride, count=cnt, slopes=sp.data_ptr(), dsts=dp.data_ptr(),
                scale=K.PRELU_SCALE) == 0
    # per row: the per-thread sums in double, their cast and the workgroup tree (10), scale * tot (1), a * a (1), the division (1)
    ev_ok('prelu_final nb %d %s' % (nb, via), dst.get(), ref['d'], margins)
    assert dst.guards_ok() and part.untouched() and slopes.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_gather_crops.  Contract (dasr_hip.h): every element of dst is written; zero for channels >= desc.C and wherever the window leaves the
# (resized) view, where nothing is read.  Descriptors are device memory and are not validated: they are valid here.
@gpu
@pytest.mark.parametrize('launch', ['all', 'edge'])
def test_gather_crops(launch, margins):
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.engine import _stream
    i, ref = ref_of(K.ref_gather, launch)
    imgs = {name: Buf(dev, img) for name, img in K.crop_images().items()}
    descs = (_lib.CropDesc * len(i['descs']))()
    for d, D in zip(descs, i['descs']):
        c, H, W = D['img'].shape
        d.src, d.C, d.H, d.W, d.vH, d.vW, d.y0, d.x0, d.flags = imgs[D['name']].ptr, c, H, W, D['vH'], D['vW'], D['y0'], D['x0'], D['flags']
    dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    n, Cc, size = len(descs), K.CROP_C, K.CROP_SIZE
    assert (n * Cc * size * size) % 256 != 0
    dst = Buf(dev, n=n * Cc * size * size)
    assert _lib.lib().dasr_gather_crops(dd.data_ptr(), n, Cc, size, dst.ptr, _stream()) == 0
    torch.cuda.synchronize()
    got = dst.get().view(n, Cc, size, size)
    want = ref['dst']
    assert biteq(got[i['exact']], want.v[i['exact']].float())           # crops without a resize, the zero channels, outside the view: bit for bit
    # a resized sample: the six roundings of the blend and, per axis, the fp32 error of the source coordinate (the division, the product, the
    # difference, the weight) times the steepest slope of the interpolant around it (R.gather_crops)
    ev_ok('gather_crops %s' % launch, got, want, margins)
    assert dst.guards_ok() and all(b.untouched() for b in imgs.values())


# ---------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@VIA
def test_argument_checks(via):
    """each returns DASR_EINVAL with nothing launched: sentinel-filled outputs stay untouched.  No kernel is reached with a null pointer."""
    dev = _gpu()
    H, W = 8, 12
    xs, ys = Slab(dev, 'f32', N, 1, H, W), Slab(dev, 'f32', N, 3, 3, 4)
    s2d = dict(x=xs.view(), N=N, H=H, W=W, scale4=K.SCALE4, shift4=K.SHIFT4, y=ys.view(), mode=0)
    bad = [dict(H=6), dict(W=10), dict(mode=2), dict(mode=1 << 4), dict(mode=1 | 3 << 4), dict(N=0), dict(N=-1), dict(x=None), dict(y=None)]
    if via == 'abi':                      # (a recorded op holds the eight floats itself)
        bad += [dict(scale4=None), dict(shift4=None)]
    for b in bad:
        assert call(via, 'lpips_s2d', **{k: v for k, v in dict(s2d, **b).items() if v is not None}) == EINVAL, b
    assert xs.untouched() and ys.untouched()
    # max-pool: sizes below one window, null tensors
    ps, po, pg = Slab(dev, 'f32', N, 1, 7, 9), Slab(dev, 'f32', N, 1, 3, 4), Slab(dev, 'f32', N, 1, 7, 9)
    fwd = dict(x=ps.view(), N=N, C=16, H=7, W=9, y=po.view())
    for b in (dict(H=2), dict(W=2), dict(N=0), dict(C=0), dict(x=None), dict(y=None)):
        assert call(via, 'maxpool3s2', **{k: v for k, v in dict(fwd, **b).items() if v is not None}) == EINVAL, b
    bwd = dict(x=ps.view(), gy=po.view(), N=N, C=16, H=7, W=9, gx=pg.view(), relu_mask=1, accumulate=0)
    for b in (dict(H=2), dict(W=2), dict(N=0), dict(C=0), dict(x=None), dict(gy=None), dict(gx=None)):
        assert call(via, 'maxpool3s2_bwd', **{k: v for k, v in dict(bwd, **b).items() if v is not None}) == EINVAL, b
    assert ps.untouched() and po.untouched() and pg.untouched()
    # head: C not a multiple of 16, N <= 0, lin or f null
    fs, gs, lin, acc = Slab(dev, 'f32', 5, 1, 5, 7), Slab(dev, 'f32', N, 1, 5, 7), Buf(dev, n=16), Buf(dev, n=1)
    head = dict(f=fs.view(), pair_off=3, N=N, C=16, H=5, W=7, lin=lin.ptr, eps=K.HEAD_EPS, coef=1.0, gcoef=1.0, loss_acc=acc.ptr, g0=gs.view(), relu_mask=0)
    for b in (dict(C=8), dict(C=20), dict(N=0), dict(N=-2), dict(H=0), dict(lin=None), dict(f=None)):
        assert call(via, 'lpips_head', **{k: v for k, v in dict(head, **b).items() if v is not None}) == EINVAL, b
    assert fs.untouched() and gs.untouched() and lin.untouched() and acc.untouched()
    # slope gradient: an empty tensor, any null tensor or pointer
    for kind, name in (('f32', 'prelu_grad'), ('f16', 'prelu_grad_f16')):
        yt, gt = Slab(dev, kind, N, 1, 5, 7), Slab(dev, kind, N, 1, 5, 7)
        slope, scratch, dst = Buf(dev, n=1), Buf(dev, n=1024), Buf(dev, n=1)
        pg_ = dict(y=yt.view(), gx=gt.view(), N=N, C=16, H=5, W=7, slope=slope.ptr, scratch256=scratch.ptr, dst=dst.ptr, scale=1.0)
        for b in (dict(N=0), dict(C=0), dict(H=0), dict(W=-1), dict(y=None), dict(gx=None), dict(slope=None), dict(scratch256=None), dict(dst=None)):
            assert call(via, name, **{k: v for k, v in dict(pg_, **b).items() if v is not None}) == EINVAL, (name, b)
        assert scratch.untouched() and dst.untouched() and slope.untouched()
    part, sl, ds = Buf(dev, n=32), Buf(dev, n=2), Buf(dev, n=2)
    sp = torch.tensor([sl.ptr, sl.ptr + 4], dtype=torch.int64, device=dev)
    dp = torch.tensor([ds.ptr, ds.ptr + 4], dtype=torch.int64, device=dev)
    fin = dict(partial=part.ptr, nblocks=8, stride=16, count=2, slopes=sp.data_ptr(), dsts=dp.data_ptr(), scale=1.0)
    for b in (dict(nblocks=0), dict(stride=7), dict(count=0), dict(partial=None), dict(slopes=None), dict(dsts=None)):
        assert call(via, 'prelu_final', **{k: v for k, v in dict(fin, **b).items() if v is not None}) == EINVAL, b
    assert ds.untouched() and part.untouched()


@gpu
def test_gather_crops_argument_checks():
    dev = _gpu()
    from dasr_amd import _lib
    L = _lib.lib()
    img, dst = Buf(dev, torch.zeros(1, 9, 11)), Buf(dev, n=49)
    descs = (_lib.CropDesc * 1)()
    d = descs[0]
    d.src, d.C, d.H, d.W, d.vH, d.vW, d.y0, d.x0, d.flags = img.ptr, 1, 9, 11, 9, 11, 0, 0, 0
    dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    for n, Cc, size, dp, op in ((0, 1, 7, dd.data_ptr(), dst.ptr), (1, 0, 7, dd.data_ptr(), dst.ptr), (1, 1, 0, dd.data_ptr(), dst.ptr),
                                (-1, -1, 7, dd.data_ptr(), dst.ptr), (1, 1, 7, None, dst.ptr), (1, 1, 7, dd.data_ptr(), None)):
        assert L.dasr_gather_crops(dp, n, Cc, size, op, None) == EINVAL, (n, Cc, size)
    torch.cuda.synchronize()
    assert dst.untouched()
    assert ctypes.sizeof(_lib.CropDesc) == 40
