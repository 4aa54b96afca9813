"""The data gradient of the HR tail's nearest-x2 upconvs in its sub-pixel form on f16 tensors (dasr_conv_params::ups = 2, conv_subpix_dgrad_kernel):
one launch on the low-resolution grid instead of a 3x3 conv on the up-sampled grid + a 2x2 sum.  Driven through the C ABI as test_gpu_kernels.py
does; references are fp64 torch on the CPU (conv_transpose2d, the adjoint of conv2d, then the 2x2 block sum, the adjoint of nearest-x2).

Shapes (low-resolution h x w; the kernel's tile is 16 x 32 outputs, its stage a 17 x 33 parity sub-image): 8x32 and 16x32 (exact tiles), 20x36
(partial tiles both ways, tile seams), 1x1 and 3x5 (everything is border), 17x33 (one pixel past a tile).

Tolerances.  (a) On operands from a coarse binary grid (weights k / 1024 with |k| <= 127: every 2- and 4-tap sum is an f16 number; gradients small
integers) every product and partial sum is an fp32 number whatever the order: the fp32-output launch must EQUAL the fp64 reference, at every pixel
-- the index algebra (parities, reversed taps, borders, seams) has nowhere to hide.  (b) On real-valued data the bound is the one the issue sets:
the direct form (the parent's launches: 3x3 data-gradient conv to an f16 tensor on the up-sampled grid, then dasr_downsum2x_f16) is run on the
same operands, its normwise error against the same fp64 reference (fp32 master weights un-rounded) is measured, and the sub-pixel form gets twice
that, never more than the 1e-3 the HR-tail tests use.  Both figures are printed; measured values are recorded in profiles/hr_subpixel.txt.

The forward and the weight gradient of the upconvs stay on the direct form (profiles/hr_subpixel.txt says why), so there is nothing of theirs here."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NF, N, SLOPE = 64, 2, 0.2
SHAPES = [(8, 32), (16, 32), (20, 36), (1, 1), (3, 5), (17, 33)]
IDS = ['%dx%d' % s for s in SHAPES]
ACT_TOL, GRAD_TOL = 1e-3, 1e-2


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def blocked16(x, dev):
    """NCHW cpu tensor of f16 numbers -> f16 BTensor on the device (layout plumbing only)"""
    from dasr_amd.engine import BTensor
    n, c, h, w = x.shape
    b = BTensor(n, c, h, w, False, dev, f16=True)
    b.t.copy_(x.reshape(n, c // 16, 16, h, w).permute(0, 1, 3, 4, 2).contiguous().half())
    return b


def tapmasks_from_definition():
    """packed tap 4 (2 py + px) + 2 a + b of the ups = 2 launch, derived here from the forward alone: y[Y][X] reads x[(Y + ky - 1) >> 1][(X + kx - 1) >> 1]
    through tap (ky, kx), so gradient pixel (2 (m - py + a) + py, 2 (n - px + b) + px) reaches input pixel (m, n) through exactly the taps collected here"""
    m = n = 4
    out = []
    for py, px, a, b in ((py, px, a, b) for py in (0, 1) for px in (0, 1) for a in (0, 1) for b in (0, 1)):
        Y, X = 2 * (m - py + a) + py, 2 * (n - px + b) + px
        out.append(sum(1 << (ky * 3 + kx) for ky in range(3) for kx in range(3) if (Y + ky - 1) >> 1 == m and (X + kx - 1) >> 1 == n))
    return out


def test_plan_tapmasks_are_the_definition():
    """the masks the generator registers (rrdbnet.subpixel_dgrad_tapmasks) are the ones the kernel tests below run on"""
    from dasr_amd.rrdbnet import subpixel_dgrad_tapmasks
    assert subpixel_dgrad_tapmasks() == tapmasks_from_definition()


_PACKS = {}


def packs(kind, dev):
    """(weights [co][ci][3][3] fp32, pack registry, 16-tap sub-pixel image, 9-tap direct image) of the data gradient of one upconv.
    'grid': weights k / 1024, |k| <= 127;  'real': He-scaled normal fp32 masters, a different draw per upconv"""
    if kind not in _PACKS:
        from dasr_amd.engine import ParamStore, PackRegistry
        g = torch.Generator().manual_seed({'grid': 3, 'real_up1': 5, 'real_up2': 7}[kind])
        if kind == 'grid':
            w = torch.randint(-127, 128, (NF, NF, 3, 3), generator=g).float() / 1024
        else:
            w = torch.randn(NF, NF, 3, 3, generator=g) * math.sqrt(2.0 / (NF * 9))
        P = ParamStore([('w', (NF, NF, 3, 3))], dev)
        P.load_state_dict({'w': w})
        pack = PackRegistry(P)
        seg = [(P.off('w'), NF, NF, 0, NF, 0, 1)]
        bw16 = tapmasks_from_definition()
        sub = pack.add(NF, NF, 16, 2, 2, seg, tapmap=[0] * 16, src_ntaps=9, tapmasks=bw16)
        direct = pack.add(NF, NF, 9, 2, 2, seg)
        pack.finalize()
        pack.run()
        torch.cuda.synchronize()
        _PACKS[kind] = (w, P, pack, sub, direct)
    return _PACKS[kind]


def ref_dgrad(g, w):
    """fp64: dL/dx of y = conv2d(nearest_x2(x), w, padding=1) for dL/dy = g"""
    gu = F.conv_transpose2d(g.double(), w.double(), padding=1)
    n, c, h2, w2 = gu.shape
    return gu.view(n, c, h2 // 2, 2, w2 // 2, 2).sum((3, 5))


def run_subpixel(dev, pk, g_hi, h, w, mask=None, alpha=1.0, f32_out=True):
    from dasr_amd.engine import BTensor, OpList, conv_op
    _, P, pack, sub = pk[:4]
    gb = blocked16(g_hi, dev)
    out = BTensor(N, NF, h, w, True, dev) if f32_out else BTensor(N, NF, h, w, False, dev, f16=True)
    mb = blocked16(mask, dev) if mask is not None else None
    ops = OpList()
    ops.add(conv_op(pack, sub, gb.view(), False, NF, 2 * h, 2 * w, h, w, N, ups=2, mask=mb.view() if mb else None, mask_f32=0, slope=SLOPE, alpha=alpha,
                    out_f32=out.view() if f32_out else None, out_bf16=None if f32_out else out.view(), out16_f16=0 if f32_out else 1))
    ops.run()
    torch.cuda.synchronize()
    return out.nchw().cpu()


def run_direct(dev, pk, g_hi, h, w, mask=None, out_scale=1.0, f32_out=True):
    """the parent's two launches: 3x3 data gradient on the 2h x 2w grid -> f16 tensor, then the 2x2 sum (+ mask, scale)"""
    from dasr_amd import _lib
    from dasr_amd.engine import BTensor, OpList, conv_op, make_op
    _, P, pack, _, direct = pk[:5]
    gb = blocked16(g_hi, dev)
    g_up = BTensor(N, NF, 2 * h, 2 * w, False, dev, f16=True)
    out = BTensor(N, NF, h, w, True, dev) if f32_out else BTensor(N, NF, h, w, False, dev, f16=True)
    mb = blocked16(mask, dev) if mask is not None else None
    ops = OpList()
    ops.add(conv_op(pack, direct, gb.view(), False, NF, 2 * h, 2 * w, 2 * h, 2 * w, N, out_bf16=g_up.view(), out16_f16=1))
    ops.add(make_op(_lib.OP_DOWNSUM_F16, src=g_up.view(), N=N, C=NF, H=h, W=w, mask=mb and mb.view(), slope=SLOPE, out_scale=out_scale,
                    dst_f32=out.view() if f32_out else None, dst_f16=None if f32_out else out.view()))
    ops.run()
    torch.cuda.synchronize()
    return out.nchw().cpu()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_subpixel_dgrad_equals_fp64_on_grid_operands(shape):
    """(a) of the module docstring: |out| <= 64 * 36 * 3 * 127 / 1024 < 2^10 on a 2^-10 grid: 20 bits, exact in fp32 in any summation order; alpha 2^-7
    is a power of two.  Every HR pixel carries a gradient, so every parity / tap-sum class meets every border, corner and tile seam."""
    dev = _gpu()
    h, w = shape
    pk = packs('grid', dev)
    g = torch.Generator().manual_seed(100 * h + w)
    g_hi = torch.randint(-3, 4, (N, NF, 2 * h, 2 * w), generator=g).float()
    want = ref_dgrad(g_hi, pk[0]) * 2.0 ** -7
    got = run_subpixel(dev, pk, g_hi, h, w, alpha=2.0 ** -7)
    assert torch.equal(got.double(), want), (shape, float((got.double() - want).abs().max()))


@pytest.mark.parametrize('shape', [(20, 36), (3, 5)], ids=['20x36', '3x5'])
def test_subpixel_dgrad_impulses_tell_every_tap_sum_apart(shape):
    """one unit impulse of the gradient per parity at a corner, an edge, the interior (and the tile seam where the image has one), each in a channel
    of its own: the response is that channel's column of reversed tap sums, exact on grid weights, and the weights differ per tap and channel"""
    dev = _gpu()
    h, w = shape
    pk = packs('grid', dev)
    g_hi = torch.zeros(N, NF, 2 * h, 2 * w)
    spots = [(0, 0), (0, 2 * w - 1), (2 * h - 1, 0), (2 * h - 1, 2 * w - 1), (0, w), (0, w + 1), (h, 0), (h + 1, 0), (h, w), (h, w + 1), (h + 1, w), (h + 1, w + 1)]
    if h > 16 and w > 32:
        spots += [(31, 63), (31, 64), (32, 63), (32, 64), (33, 65), (2 * h - 1, 64)]
    for c, (y, x) in enumerate(spots):
        g_hi[c % N, c, y, x] = 1.0
    want = ref_dgrad(g_hi, pk[0])
    got = run_subpixel(dev, pk, g_hi, h, w)
    assert torch.equal(got.double(), want)
    assert float(want.abs().sum()) > 0


@pytest.mark.parametrize('shape', [(20, 36), (17, 33), (1, 1)], ids=['20x36', '17x33', '1x1'])
def test_subpixel_dgrad_is_the_adjoint_of_the_upconv(shape):
    """<conv(nearest_x2(x)), g> = <x, dgrad(g)> with the forward in fp64 on the CPU and the data gradient from the kernel, for x on all pixels and
    for x on the border frame only (the rows / columns whose taps meet the zero padding).  Grid operands: both sides are exact sums of numbers on a
    2^-10 grid below 2^40 -- exact in fp64 -- so the two inner products must agree to the last bit."""
    dev = _gpu()
    h, w = shape
    pk = packs('grid', dev)
    g = torch.Generator().manual_seed(7 * h + w)
    g_hi = torch.randint(-3, 4, (N, NF, 2 * h, 2 * w), generator=g).float()
    got = run_subpixel(dev, pk, g_hi, h, w).double()
    frame = torch.zeros(1, 1, h, w, dtype=torch.float64)
    frame[..., 0, :] = frame[..., -1, :] = frame[..., :, 0] = frame[..., :, -1] = 1
    for sel in (torch.ones_like(frame), frame):
        x = torch.randint(-3, 4, (N, NF, h, w), generator=g).double() * sel
        y = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), pk[0].double(), padding=1)
        lhs, rhs = float((y * g_hi.double()).sum()), float((x * got).sum())
        assert lhs == rhs, (shape, lhs, rhs)


VARIANTS = ['up2_mask_f16', 'up2_nomask_f16', 'up1_alpha_f32']


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_subpixel_dgrad_is_no_worse_than_the_direct_form(shape, variant):
    """(b) of the module docstring, for both upconvs' launches: upconv2 (LeakyReLU' mask of u1 -> f16 gradient; also without the mask) and upconv1
    (alpha = 1 / gscale -> fp32 gradient of the trunk output).  Gradient and mask tensors hold f16 numbers, the weights are fp32 masters."""
    dev = _gpu()
    h, w = shape
    up1 = variant.startswith('up1')
    pk = packs('real_up1' if up1 else 'real_up2', dev)
    g = torch.Generator().manual_seed(1000 + 100 * h + w)
    gscale = 2.0 ** 10
    g_hi = (torch.randn(N, NF, 2 * h, 2 * w, generator=g) * (0.25 if up1 else 1.0)).half().float()
    mask = torch.randn(N, NF, h, w, generator=g).half().float() if variant == 'up2_mask_f16' else None
    want = ref_dgrad(g_hi, pk[0])
    if mask is not None:
        want = torch.where(mask.double() > 0, want, want * SLOPE)
    if up1:
        want = want / gscale
        got = run_subpixel(dev, pk, g_hi, h, w, alpha=1.0 / gscale, f32_out=True)
        old = run_direct(dev, pk, g_hi, h, w, out_scale=1.0 / gscale, f32_out=True)
    else:
        got = run_subpixel(dev, pk, g_hi, h, w, mask=mask, f32_out=False)
        old = run_direct(dev, pk, g_hi, h, w, mask=mask, f32_out=False)
    e_new, e_old = rel(got, want), rel(old, want)
    tol = min(2.0 * e_old, ACT_TOL)
    print('subpixel dgrad %s %dx%d: normwise error vs fp64 sub-pixel %.3e, direct form %.3e, bound %.3e' % (variant, h, w, e_new, e_old, tol))
    assert e_new <= tol, (variant, shape, e_new, e_old)


def test_subpixel_dgrad_launch_is_validated():
    """what the launcher refuses (DASR_EINVAL, nothing launched): a gradient grid that is not twice the output grid, f32 tensors, a bf16 output, and
    every epilogue term outside the documented set (activation, bias, a strided sub-grid output)"""
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.engine import BTensor, conv_op
    L = _lib.lib()
    _, P, pack, sub = packs('grid', dev)[:4]
    h, w = 3, 5
    gb, out = BTensor(N, NF, 2 * h, 2 * w, False, dev, f16=True), BTensor(N, NF, h, w, False, dev, f16=True)
    ok = conv_op(pack, sub, gb.view(), False, NF, 2 * h, 2 * w, h, w, N, ups=2, out_bf16=out.view(), out16_f16=1)
    assert L.dasr_conv(C.byref(ok.conv), None) == 0
    for change in (dict(Hin=2 * h + 1), dict(Win=w), dict(out16_f16=0), dict(in_f32=1), dict(stride=2), dict(in_stride=2), dict(act=1), dict(act=2), dict(out_oy=1),
                   dict(out_ox=1), dict(out_W=4 * w), dict(out_stride=2), dict(bias=out.t.data_ptr()), dict(mt=3)):
        bad = conv_op(pack, sub, gb.view(), False, NF, 2 * h, 2 * w, h, w, N, ups=2, out_bf16=out.view(), out16_f16=1)
        for k, v in change.items():
            setattr(bad.conv, k, v)
        assert L.dasr_conv(C.byref(bad.conv), None) == -22, change
    torch.cuda.synchronize()


def test_sr_step_with_the_subpixel_tail_matches_the_split_bf16_tail(monkeypatch):
    """plan level: N 2, nf 64, nb 1, LR 20 x 36 -- one whole SR step with the f16 tail (sub-pixel data gradients) against the same step with
    DASR_HR_PREC=3 (the sub-pixel path in ~fp32): SR output within 1e-3, every gradient tensor -- the HR tail's and, through dL/d(trunk output), the
    trunk's -- within 1e-2 normwise (the tolerances of the HR-tail tests, rrdbnet.py::_register_stream_packs).  The f16 plan holds no 2x2 down-sum
    and runs both upconv data gradients as ups = 2 launches on the low-resolution grids (the forward keeps its ups = 1 launches)."""
    dev = _gpu()
    from oracle import fixtures
    from dasr_amd import _lib, options
    from dasr_amd.models import create_model
    case = dict(kind='sr', nf=64, nb=1, n=2, lr=(20, 36))
    batch = fixtures.make_batch(case)
    res = {}
    for prec in ('2', '3'):
        monkeypatch.setenv('DASR_HR_PREC', prec)
        opt = fixtures.make_opt(case)
        opt['gpu_ids'] = [0]
        m = create_model(options.dict_to_nonedict(opt))
        m.netG.load_state_dict(fixtures.seeded_state_dict(m.netG.state_dict(), 1, 0.1))
        m.update_learning_rate()
        m.feed_data(batch)
        m.optimize_parameters(1)
        torch.cuda.synchronize()
        plan = m._out_plans[0]
        res[prec] = (m.fake_H.cpu().clone(), m.netG.params.grad_dict(), plan.g_t0.nchw().cpu().clone(), plan)
    plan = res['2'][3]
    kinds = [o.op for o in plan.bwd.ops]
    assert _lib.OP_DOWNSUM_F16 not in kinds
    sub = [o for o in plan.bwd.ops if o.op == _lib.OP_CONV and o.conv.ups == 2]
    assert [(o.conv.Hout, o.conv.Wout) for o in sub] == [(40, 72), (20, 36)]
    assert not any(o.op == _lib.OP_CONV and not o.conv.in_f32 and o.conv.ups == 0 and o.conv.cin == 64 and o.conv.cout == 64 and o.conv.Hout == 40
                   for o in plan.bwd.ops[:plan.tail_end])   # no 3x3 data gradient towards an up-sampled tensor is left
    e_sr = rel(res['2'][0], res['3'][0])
    e_gt0 = rel(res['2'][2], res['3'][2])
    worst, wk = 0.0, None
    for k, gv in res['2'][1].items():
        r = rel(gv, res['3'][1][k])
        if r > worst:
            worst, wk = r, k
    print('subpixel f16 tail vs DASR_HR_PREC=3: SR %.3e, dL/d(trunk output) %.3e, worst gradient %.3e at %s' % (e_sr, e_gt0, worst, wk))
    assert e_sr < ACT_TOL
    assert e_gt0 < GRAD_TOL
    assert worst < GRAD_TOL, (wk, worst)
