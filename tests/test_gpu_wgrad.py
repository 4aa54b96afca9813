"""GPU parity tests of the weight-gradient path (csrc/wgrad.hip: wgrad3_ld_kernel, wgrad_kernel, wgrad_reduce_kernel; the operand producers of
csrc/misc.hip) against fp64 references, driven the way the product drives them: WgradGroup / WgradGroup3 -> OpList -> dasr_run_ops.

The operands are rounded to the kernel's staging format (bf16, f16, or f16 of g_scale * g) before they reach the device, so every product is exact in
fp32 and only the fp32 accumulation differs from the fp64 reference.  Each weight and bias element is checked against

    |got - ref| <= c * 2^-23 * sum |g| |x|

with c derived from the accumulation length L (fp32 roundings in sequence behind one element; each errs by at most 2^-24 of a partial sum bounded
by sum |g||x|; they are independent and of mean zero, so c = 4 + 2 sqrt(L) is several standard deviations of their sum: tens, not thousands).
Workspace and gradient buffer are NaN-poisoned after Workspace.finalize(), the parameters next to the target hold a sentinel that must come back
bit-unchanged: a reduce that reads a partial no workgroup wrote, or writes outside its [cout][cin][kh][kw] block, fails."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

from test_gpu_kernels import bf16r, rel, to_blocked

pytestmark = pytest.mark.gpu

EINVAL = -22
SENTINEL = -1234.5678


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f16r(x):
    return x.half().float()


def blocked16(x, dev, f16):
    """NCHW cpu tensor (already representable) -> 16-bit BTensor (f16 or bf16) on the device"""
    from dasr_amd.engine import BTensor
    N, Cc, H, W = x.shape
    b = BTensor(N, Cc, H, W, False, dev, f16=f16)
    xp = torch.zeros(N, b.planes * 16, H, W)
    xp[:, :Cc] = x
    b.t.copy_(xp.view(N, b.planes, 16, H, W).permute(0, 1, 3, 4, 2).to(b.t.dtype))
    return b


def acc_c(L):
    return 4.0 + 2.0 * math.sqrt(L)


def params_with_neighbours(dev, convs):
    """ParamStore [pre | (w, b) per conv | post] with NaN in the whole gradient buffer and the sentinel in the neighbours"""
    from dasr_amd.engine import ParamStore
    spec = [('pre', (37,))]
    for k, shape in convs:
        spec += [(k + 'weight', shape), (k + 'bias', (shape[0],))]
    spec += [('post', (29,))]
    P = ParamStore(spec, dev)
    return P


def poison(P, ws, owned):
    """NaN in the workspace (ws=None: left alone) and in the gradients the reduce owns, the sentinel everywhere else"""
    if ws is not None:
        ws.buf.fill_(float('nan'))
    P.grad.fill_(float('nan'))
    for k in P.spec:
        if k not in owned:
            P.view(k, P.grad).fill_(SENTINEL)


def check_neighbours(P, owned):
    for k in P.spec:
        if k not in owned:
            v = P.view(k, P.grad).cpu()
            assert torch.equal(v, torch.full_like(v, SENTINEL)), 'parameter %s next to the target was written' % k


def check_elem(name, got, ref, absref, c, margins, norm_tol=2e-5):
    """element bound + norm-relative check; returns the worst (|err| / bound) for the sensitivity checks"""
    got = got.double()
    assert torch.isfinite(got).all(), '%s: NaN / inf left in the gradient (an element the reduce owns was not written)' % name
    err = (got - ref).abs()
    bound = c * 2.0 ** -23 * absref
    worst = float((err / bound.clamp_min(1e-300)).max())
    r = rel(got, ref)
    margins('wgrad %s: worst |err| / bound %.3f (c %.1f), norm-rel %.2e' % (name, worst, c, r))
    assert (err <= bound).all(), '%s: %d elements beyond the bound, worst %.3f of it' % (name, int((err > bound).sum()), worst)
    assert r < norm_tol, (name, r)
    return worst


def wref(x, g, kh, stride, pad, ups=0):
    """fp64 weight gradient and sum |g||x| per element, bias gradient and sum |g| per channel"""
    xx = x.double()
    if ups:
        xx = F.interpolate(xx, scale_factor=2, mode='nearest')
    shape = (g.shape[1], x.shape[1], kh, kh)
    gd = g.double()
    return (conv2d_weight(xx, shape, gd, stride=stride, padding=pad), conv2d_weight(xx.abs(), shape, gd.abs(), stride=stride, padding=pad),
            gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3)))


def run(ops, ws, P, owned):
    ws.finalize()
    poison(P, ws, owned)
    from dasr_amd.engine import OpList
    ol = OpList()
    for o in ops:
        ol.add(o)
    ol.run()
    torch.cuda.synchronize()
    check_neighbours(P, owned)
    return ol


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# wgrad3_ld_kernel (WgradGroup3, kh = 33)
W3_CASES = [
    # name, f16, g_scale, ups, N, cin, cout, Hin, Win, target, forced nsplit, expected nsplit
    ('bf16_c16o3_1x1_ns1', False, 0, 0, 1, 16, 3, 1, 1, 256, None, 1),
    ('f16_c32o48_2x3_ns3', True, 4096.0, 0, 3, 32, 48, 2, 3, 256, None, 3),
    ('f16_c96o160_ups7x15_ns5', True, 4096.0, 1, 3, 96, 160, 7, 15, 20, None, 5),
    ('bf16_c192o96_ups12x20_ns24', False, 0, 1, 3, 192, 96, 12, 20, 256, None, 24),
    ('f16s1_c192o32_9x17_ns4', True, 1.0, 0, 1, 192, 32, 9, 17, 256, None, 4),
    ('f16_c96o48_24x40_ns8', True, 4096.0, 0, 1, 96, 48, 24, 40, 20, None, 8),
    ('bf16_c32o96_9x17_idle', False, 0, 0, 1, 32, 96, 9, 17, 256, 6, 6),
]


def _w3_group(P, key, gb, xb, cout, cin, Hin, Win, Hout, Wout, N, ups):
    from dasr_amd.engine import WgradGroup3, ceil_div
    grp = WgradGroup3()
    octs = list(range(0, cout, 32))
    for c0 in range(0, cin, 64):   # the part layout of rrdbnet._Plan._wg3
        blk = min(64, cin - c0)
        for k0 in range(0, len(octs), 3):
            sub = octs[k0:k0 + 3]
            tiles = [dict(dst_w_off=P.off(key + 'weight'), dst_b_off=P.off(key + 'bias') if c0 == 0 else None, cout=cout, cin=cin, oc0=oc0, c0=c0,
                          n_ctiles=min(2, ceil_div(blk, 32))) for oc0 in sub]
            grp.add_block(gb.view(sub[0]), min(2 * len(sub), gb.planes - sub[0] // 16), xb.view(c0), ceil_div(blk, 16), ceil_div(blk, 32),
                          Hin, Win, Hout, Wout, N, tiles, want_bias=(c0 == 0), ups=ups)
    return grp


@pytest.mark.parametrize('case', W3_CASES, ids=[c[0] for c in W3_CASES])
def test_wgrad3_matches_fp64(case, margins):
    dev = _gpu()
    from dasr_amd.engine import Workspace, ceil_div
    name, f16, gs, ups, N, cin, cout, Hin, Win, target, force, want_ns = case
    Hout, Wout = (2 * Hin, 2 * Win) if ups else (Hin, Win)
    g = torch.Generator().manual_seed(len(name))
    x = (f16r if f16 else bf16r)(torch.randn(N, cin, Hin, Win, generator=g))
    if f16 and gs > 1:   # gradients of ~1e-6: subnormal (or zero) in f16 without the pre-scale
        g16 = f16r(torch.randn(N, cout, Hout, Wout, generator=g) * 1e-6 * gs)
    elif f16:
        g16 = f16r(torch.randn(N, cout, Hout, Wout, generator=g) * 1e-2)
    else:
        g16 = bf16r(torch.randn(N, cout, Hout, Wout, generator=g))
    gtrue = g16 / gs if (f16 and gs) else g16   # what the f16 tensor stands for (exact: gs is a power of two)
    key = 'c.'
    P = params_with_neighbours(dev, [(key, (cout, cin, 3, 3))])
    owned = {key + 'weight', key + 'bias'}
    xb, gb = blocked16(x, dev, f16), blocked16(g16, dev, f16)
    ws = Workspace(dev)
    grp = _w3_group(P, key, gb, xb, cout, cin, Hin, Win, Hout, Wout, N, ups)
    if f16:
        grp.f16, grp.g_scale = True, gs
    grp.finalize(ws, dev, target_wgs=target, nsplit=force)
    ntiles = N * ceil_div(Hout, 8) * ceil_div(Wout, 16)
    assert grp.nsplit == want_ns and (force is None or want_ns > ntiles), (grp.nsplit, ntiles)
    ops = grp.ops(P.grad.data_ptr())
    assert ops[1].get('few_splits') == int(want_ns <= 4)
    ol = run(ops, ws, P, owned)
    dw, aw, db, ab = wref(x, gtrue, 3, 1, 1, ups)
    K = ceil_div(ntiles, grp.nsplit) * 8   # MFMA k-steps behind one partial
    gd = P.grad_dict()
    check_elem(name + ' w', gd[key + 'weight'], dw, aw, acc_c(2 * K + ceil_div(grp.nsplit, 16) + 5), margins)
    check_elem(name + ' b', gd[key + 'bias'], db, ab, acc_c(8 * K + 7 + grp.nsplit), margins)
    if 1 < grp.nsplit <= ntiles:
        # sensitivity: the reduce of the same workspace with one split fewer (its last split holds a pixel tile) must fail the element bound
        reds = _reduce_image(grp)
        for rp in reds:
            rp.nsplit -= 1
        _upload_reduce(grp, reds)
        P.grad.fill_(float('nan'))
        ol.run(1, 2)
        torch.cuda.synchronize()
        got = P.grad_dict()[key + 'weight'].double()
        assert ((got - dw).abs() > acc_c(2 * K + 5) * 2.0 ** -23 * aw).any(), 'a dropped split stays inside the bound'


def _reduce_image(grp):
    from dasr_amd import _lib
    raw = bytes(grp.r_dev.cpu().numpy().tobytes())
    return list((_lib.WgradReducePart * (len(raw) // C.sizeof(_lib.WgradReducePart))).from_buffer_copy(raw))


def _upload_reduce(grp, reds):
    """rewrite the reduce table in place (same size, same device buffer: the recorded ops keep their pointer)"""
    from dasr_amd import _lib
    arr = (_lib.WgradReducePart * len(reds))(*reds)
    grp.r_dev.copy_(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the grouped dense-block launch as TrunkStore records it
RDB_CASES = [
    # name, nf, f16, RDBs, N, expect ppu > 0
    ('nf64_bf16_12rdb_ppu', 64, False, 12, 1, True),
    ('nf32_f16_6rdb_ppu', 32, True, 6, 1, True),
    ('nf32_bf16_3rdb_ns8', 32, False, 3, 3, False),
    ('nf64_f16_2rdb_ns8', 64, True, 2, 2, False),
]


@pytest.mark.parametrize('case', RDB_CASES, ids=[c[0] for c in RDB_CASES])
def test_dense_block_group_matches_fp64(case, margins):
    dev = _gpu()
    from dasr_amd import rrdbnet
    from dasr_amd.engine import ParamStore, BTensor, Workspace, WgradGroup3, ceil_div
    name, nf, f16, n_rdb, N, want_ppu = case
    h, w, GC = 12, 20, rrdbnet.GC
    sc = nf + 4 * GC
    gs = 1024.0 if f16 else 0.0
    P = ParamStore(rrdbnet.rrdbnet_param_spec(3, 3, nf, ceil_div(n_rdb, 3)), dev)
    g = torch.Generator().manual_seed(n_rdb * nf)
    rq = f16r if f16 else bf16r
    grp, ws, rdbs, ppu, owned = WgradGroup3(), Workspace(dev), [], 0, set()
    for r in range(n_rdb):
        pre = 'model.1.sub.%d.RDB%d.conv' % (r // 3, r % 3 + 1)
        S = rq(torch.randn(N, sc, h, w, generator=g))
        G16 = rq(torch.randn(N, sc, h, w, generator=g) * (1e-4 * gs if f16 else 1.0))
        Sb, Gb = blocked16(S, dev, f16), blocked16(G16, dev, f16)
        ppu, _ = rrdbnet.rdb_wgrad_parts(grp, nf, pre, P, BTensor.wrap(Gb.t, sc, False), BTensor.wrap(Sb.t, sc, False), h, w, N)
        rdbs.append((pre, S, G16 / gs if f16 else G16, Sb, Gb))
        owned |= {'%s%d.0.%s' % (pre, j, t) for j in range(1, 6) for t in ('weight', 'bias')}
    if f16:
        grp.f16, grp.g_scale = True, gs
    grp.finalize(ws, dev, target_wgs=256, ppu=ppu)
    assert (grp.ppu > 0) == want_ppu, (grp.ppu, grp.nsplit, len(grp.parts))
    ops = grp.ops(P.grad.data_ptr())
    run(ops, ws, P, owned)
    gd = P.grad_dict()
    K = ceil_div(N * ceil_div(h, 8) * ceil_div(w, 16), grp.nsplit) * 8
    worst_w = worst_b = 0.0
    for pre, S, G, _, _ in rdbs:
        for j in range(1, 6):
            cin, cout = nf + (j - 1) * GC, (GC if j < 5 else nf)
            goff = 0 if j == 5 else nf + (4 - j) * GC   # gradient slab: conv5 | conv4 | conv3 | conv2 | conv1
            dw, aw, db, ab = wref(S[:, :cin], G[:, goff:goff + cout], 3, 1, 1)
            k = '%s%d.0.' % (pre, j)
            worst_w = max(worst_w, check_elem('%s %s%d w' % (name, pre[-9:], j), gd[k + 'weight'], dw, aw, acc_c(2 * K + 5), lambda m: None))
            worst_b = max(worst_b, check_elem('%s %s%d b' % (name, pre[-9:], j), gd[k + 'bias'], db, ab, acc_c(8 * K + 7 + grp.nsplit), lambda m: None))
    margins('wgrad %s (ppu %d, nsplit %d, %d parts): worst |err| / bound w %.3f b %.3f' % (name, grp.ppu, grp.nsplit, len(grp.parts), worst_w, worst_b))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# wgrad_kernel (WgradGroup)
WG_CASES = [
    # name, kh, stride, cin, cout, H, W, N, f16 (g_scale 4096), pairs, scale, target, min nsplit
    ('f16_k4s2', 4, 2, 16, 64, 32, 40, 2, True, 1, 1.0, 768, 1),
    ('f16_k4s1_scale_half', 4, 1, 64, 32, 15, 18, 1, True, 1, 0.5, 768, 1),
    ('f16_k3s1', 3, 1, 48, 40, 11, 19, 2, True, 1, 1.0, 24, 1),
    ('k5_tap_split', 5, 1, 64, 40, 13, 21, 2, False, 1, 1.0, 768, 1),
    ('k1', 1, 1, 80, 24, 13, 17, 2, False, 1, 1.0, 768, 1),
    ('k3s2', 3, 2, 64, 48, 24, 40, 2, False, 1, 1.0, 768, 1),
    ('f16_more_pairs', 3, 1, 32, 48, 14, 22, 2, True, 3, 1.0, 768, 1),
    ('ns256', 3, 1, 32, 64, 64, 128, 4, False, 1, 1.0, 768, 129),
]


@pytest.mark.parametrize('case', WG_CASES, ids=[c[0] for c in WG_CASES])
def test_wgrad_four_wave_matches_fp64(case, margins):
    dev = _gpu()
    from dasr_amd.engine import WgradGroup, Workspace, ceil_div
    name, kh, stride, cin, cout, H, W, N, f16, pairs, scale, target, min_ns = case
    pad = (kh - 1) // 2 if stride == 1 else 1
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kh) // stride + 1
    gs = 4096.0 if f16 else 0.0
    g = torch.Generator().manual_seed(kh * 100 + cin + cout)
    data = []
    for _ in range(pairs):
        if f16:   # f32 tensors whose staging (f16 of x, f16 of gs * g) is exact
            x = f16r(torch.randn(N, cin, H, W, generator=g))
            gy = f16r(torch.randn(N, cout, Ho, Wo, generator=g) * 1e-6 * gs) / gs
        else:
            x, gy = bf16r(torch.randn(N, cin, H, W, generator=g)), bf16r(torch.randn(N, cout, Ho, Wo, generator=g))
        data.append((x, gy, to_blocked(x, True, dev), to_blocked(gy, True, dev)))
    key = 'c.'
    P = params_with_neighbours(dev, [(key, (cout, cin, kh, kh))])
    owned = {key + 'weight', key + 'bias'}
    ws, grp = Workspace(dev), WgradGroup(kh, stride)
    (_, _, xb, gb) = data[0]
    grp.add_conv(gb.view, True, gb.planes, xb.view, True, xb.planes, cout, cin, H, W, Ho, Wo, N, P.off(key + 'weight'), P.off(key + 'bias'), pad=pad,
                 f16=f16, g_scale=gs, more_pairs=[(d[3].view, d[2].view) for d in data[1:]])
    grp.finalize(ws, dev, target_wgs=target)
    assert grp.nsplit >= min_ns, grp.nsplit
    ops = grp.ops(P.grad.data_ptr(), scale=scale)
    assert ops[0].get('f32') == (3 if f16 else 1) and ops[1].get('inv_prescale') == (1.0 / gs if f16 else 0.0)
    ol = run(ops, ws, P, owned)
    dw = aw = 0
    for x, gy, _, _ in data:
        a, b_, _, _ = wref(x, gy, kh, stride, pad)
        dw, aw = dw + a, aw + b_
    _, _, db, ab = wref(data[0][0], data[0][1], kh, stride, pad)   # the bias: first pair only
    ph = 2 if stride == 2 else (8 if kh in (3, 1) else 4)
    ntiles = N * ceil_div(Ho, ph) * ceil_div(Wo, 16)
    K = ceil_div(ntiles, grp.nsplit) * ph
    nsp = grp.nsplit * pairs
    gd = P.grad_dict()
    c_w = acc_c(2 * K + ceil_div(nsp, 16) + 5)
    check_elem(name + ' w', gd[key + 'weight'], dw * scale, aw * scale, c_w, margins)
    # f32 tensors: the bias is summed from the unrounded gradient, per thread over its tiles, then over 256 threads in LDS
    check_elem(name + ' b', gd[key + 'bias'], db * scale, ab * scale, acc_c(ceil_div(ntiles, grp.nsplit) + 256 * 2 + 7 + grp.nsplit), margins)
    # sensitivity: a reduce scale off by 2^-10 is seen by the element bound
    ol.set(1, 'scale', scale * (1 + 2 ** -10))
    P.grad.fill_(float('nan'))
    ol.run(1, 2)
    torch.cuda.synchronize()
    got = P.grad_dict()[key + 'weight'].double()
    assert ((got - dw * scale).abs() > c_w * 2.0 ** -23 * aw * scale).any(), 'a reduce scale off by 2^-10 stays inside the bound'


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_split_operand_wgrad_is_fp32_grade(margins):
    """split operands (gan_nets: dasr_f16_residual of g at 4096 and of x at 1, three variants g.x + g.x_lo + g_lo.x) on UNROUNDED f32 data.

    Error budget against fp64: the dropped g_lo.x_lo term and the f16 rounding of x_lo / g_lo each leave ~2^-22 of a product (with subnormal x_lo at most
    2^-25 absolute), the fp32 accumulation ~2^-24 sqrt(L) of sum |g||x|; the cancellation sum |g||x| / |dW| ~ sqrt(N H W) ~ 30 at this size: a
    norm-relative error of a few 1e-7 to 2e-6.  Asserted: 1e-5.  One f16 operand pair alone leaves ~2^-12 per product: >= 10x worse."""
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.engine import BTensor, OpList, WgradGroup, Workspace, make_op
    N, cin, cout, H, W, kh = 2, 48, 40, 16, 24, 3
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, cin, H, W, generator=g)
    gy = torch.randn(N, cout, H, W, generator=g) * 1e-3
    xb, gb = to_blocked(x, True, dev), to_blocked(gy, True, dev)
    g_lo, x_lo = BTensor(N, cout, H, W, True, dev), BTensor(N, cin, H, W, True, dev)
    prep = OpList()
    for src, dst, sc in ((gb, g_lo, 4096.0), (xb, x_lo, 1.0)):
        prep.add(make_op(_lib.OP_CVT_F16, x=src.view(), N=N, C=src.C, H=src.H, W=src.W, scale=sc, y=dst.view(), form=3))
    prep.run()
    dw, aw, db, ab = wref(x, gy, kh, 1, 1)
    res = {}
    for mode in ('split', 'single', 'split_bias_all'):
        key = 'c.'
        P = params_with_neighbours(dev, [(key, (cout, cin, kh, kh))])
        owned = {key + 'weight', key + 'bias'}
        ws, grp = Workspace(dev), WgradGroup(kh, 1)
        grp.add_conv(gb.view, True, gb.planes, xb.view, True, xb.planes, cout, cin, H, W, H, W, N, P.off(key + 'weight'), P.off(key + 'bias'),
                     f16=True, g_scale=4096.0, split=None if mode == 'single' else (g_lo.view, x_lo.view))
        grp.finalize(ws, dev, target_wgs=48)
        ops = grp.ops(P.grad.data_ptr())
        if mode == 'split_bias_all':   # sensitivity: the bias summed over all 3 * nsplit splits (the variants' zero bias partials are not written)
            reds = _reduce_image(grp)
            for rp in reds:
                assert rp.bias_nsplit == grp.nsplit and rp.nsplit == 3 * grp.nsplit
                rp.bias_nsplit = rp.nsplit
            _upload_reduce(grp, reds)
        run(ops, ws, P, owned)
        res[mode] = P.grad_dict()
    e_split, e_single = rel(res['split'][key + 'weight'], dw), rel(res['single'][key + 'weight'], dw)
    margins('wgrad split operands: norm-rel %.2e (bound 1e-5), single f16 pair %.2e (ratio %.0f)' % (e_split, e_single, e_single / e_split))
    assert e_split < 1e-5, e_split
    assert e_single > 10 * e_split, (e_single, e_split)
    ntiles = N * 2 * 2
    check_elem('split b', res['split'][key + 'bias'], db, ab, acc_c(ntiles + 512 + 7 + 3 * ntiles), margins)
    bad = res['split_bias_all'][key + 'bias'].double()
    assert not torch.isfinite(bad).all() or ((bad - db).abs() > 1e-3 * ab).any(), 'bias summed over the variants went unnoticed'


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def bits_equal(got, want, src, what):
    """bitwise equality of two 16-bit tensors (NaN payloads aside), with the first mismatches and their source values in the message"""
    g16, w16 = got.view(torch.int16), want.view(torch.int16)
    same = (g16 == w16) | (torch.isnan(got.float()) & torch.isnan(want.float()))
    if not bool(same.all()):
        i = (~same).nonzero()[:6].tolist()
        raise AssertionError('%s: %d mismatches, e.g. %s' % (what, int((~same).sum()), ['src %r got %r want %r' % (
            float(src[tuple(k)]), float(got[tuple(k)]), float(want[tuple(k)])) for k in i]))


@pytest.mark.parametrize('C_', [3, 40, 64])
def test_operand_producers_round_like_torch(C_):
    """dasr_cvt_f16, dasr_cvt_split16 (f16 and bf16) and dasr_f16_residual: bit-exact against torch's half() / bfloat16() rounding, padding planes
    included, with values at the f16 overflow and subnormal limits"""
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.engine import BTensor
    L = _lib.lib()
    N, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(C_)
    x = torch.randn(N, C_, H, W, generator=g) * torch.exp2(torch.randint(-20, 12, (N, C_, H, W), generator=g).float())
    special = torch.tensor([65504.0, 65519.0, 65520.0, 65536.0, 2 ** -14, 2 ** -24, 2 ** -25, 1.5 * 2 ** -25, 3 * 2 ** -26, 2 ** -14 - 2 ** -24,
                            1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 0.0])
    flat = x.view(-1)
    flat[:special.numel()] = special
    flat[special.numel():2 * special.numel()] = -special
    xb = to_blocked(x, True, dev)
    P = xb.planes
    whole = xb.t.cpu()   # [N][planes][H][W][16] (pad channels zero)
    for scale in (1.0, 0.75, 2.0 ** -3):
        y = BTensor(N, C_, H, W, False, dev, f16=True)
        y.t.fill_(float('nan'))
        _lib.check(L.dasr_cvt_f16(xb.view(), N, C_, H, W, C.c_float(scale), y.view(), _stream()), 'cvt_f16')
        torch.cuda.synchronize()
        bits_equal(y.t.cpu(), (whole * scale).half(), whole * scale, 'cvt_f16 scale %g' % scale)
        for f16, dt in ((1, torch.float16), (0, torch.bfloat16)):
            ys = BTensor(N, 32 * P, H, W, False, dev, f16=bool(f16))   # hi planes [0, P), lo planes [P, 2P)
            ys.t.fill_(float('nan'))
            _lib.check(L.dasr_cvt_split16(xb.view(), N, C_, H, W, C.c_float(scale), ys.view(), f16, _stream()), 'cvt_split16')
            torch.cuda.synchronize()
            vv = whole * scale
            hi = vv.to(dt)
            lo = (vv - hi.float()).to(dt)
            got = ys.t.cpu()
            bits_equal(got[:, :P], hi, vv, 'cvt_split16 hi f16 %d scale %g' % (f16, scale))
            bits_equal(got[:, P:], lo, vv - hi.float(), 'cvt_split16 lo f16 %d scale %g' % (f16, scale))
    for scale in (1.0, 2.0 ** 12, 2.0 ** -3):   # power-of-two scales (what the product uses): h / scale is exact
        r = BTensor(N, C_, H, W, True, dev)
        r.t.fill_(float('nan'))
        _lib.check(L.dasr_f16_residual(xb.view(), N, C_, H, W, C.c_float(scale), r.view(), _stream()), 'f16_residual')
        torch.cuda.synchronize()
        want = whole - (whole * scale).half().float() * (1.0 / scale)
        got = r.t.cpu()
        same = (got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
        assert same.all(), ('f16_residual', scale, got[~same][:4], want[~same][:4])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_wgrad_argument_checks_reject_before_launch():
    """dasr_wgrad: kh 33 with f32 = 1, an invalid ppu, ppu bits on kh != 33, bits above the ppu byte: DASR_EINVAL and no workgroup ran (the workspace keeps
    its poison)"""
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.engine import WgradGroup, Workspace
    L = _lib.lib()
    N, cin, cout, H, W = 1, 64, 96, 8, 16
    x, gy = bf16r(torch.randn(N, cin, H, W)), bf16r(torch.randn(N, cout, H, W))
    P = params_with_neighbours(dev, [('c.', (cout, cin, 3, 3))])
    xb, gb = blocked16(x, dev, False), blocked16(gy, dev, False)
    ws = Workspace(dev)
    g3 = _w3_group(P, 'c.', gb, xb, cout, cin, H, W, H, W, N, 0)   # one part
    g3.finalize(ws, dev, target_wgs=256)
    assert len(g3.parts) == 1 and g3.nsplit == 1
    xf, gf = to_blocked(x, True, dev), to_blocked(gy, True, dev)
    g4 = WgradGroup(3, 1)
    g4.add_conv(gf.view, True, gf.planes, xf.view, True, xf.planes, cout, cin, H, W, H, W, N, P.off('c.weight'), P.off('c.bias'))
    g4.finalize(ws, dev, target_wgs=8)
    ws.finalize()
    ws.buf.fill_(float('nan'))
    torch.cuda.synchronize()
    wsp = C.c_void_p(ws.buf.data_ptr())
    p3, n3 = C.c_void_p(g3.w_dev.data_ptr()), len(g3.parts)
    p4, n4 = C.c_void_p(g4.w_dev.data_ptr()), len(g4.parts)
    bad = [(p3, n3, 1, 33, 1, 1),              # grouped 3x3 kernel on f32 tensors
           (p3, n3, 1 | (2 << 16), 33, 1, 0),   # ppu 2 does not divide 1 part
           (p3, n3, 1 | (1 << 16), 33, 1, 0),   # ppu 1: 1 unit x 1 split is not a multiple of 8
           (p3, n3, 1 | (1 << 24), 33, 1, 0),   # bits above the ppu byte
           (p3, n3, 0, 33, 1, 0),               # no split
           (p4, n4, g4.nsplit | (1 << 16), 3, 1, 1),   # ppu bits on the 4-wave kernel
           (p4, n4, g4.nsplit, 7, 1, 1)]        # no such kernel size
    for parts, n, ns, kh, st, f32 in bad:
        assert L.dasr_wgrad(parts, n, ns, kh, st, f32, wsp, _stream()) == EINVAL, (ns, kh, f32)
    torch.cuda.synchronize()
    assert torch.isnan(ws.buf).all(), 'a rejected dasr_wgrad call launched workgroups'
    assert L.dasr_wgrad(p3, n3, 1, 33, 1, 0, wsp, _stream()) == 0   # the same arguments with valid flags do launch
    torch.cuda.synchronize()
    assert not torch.isnan(ws.buf).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['wgrad3', 'k5'])
def test_few_splits_reduce_is_bit_identical_to_the_general_path(kind):
    """wgrad_reduce_kernel: on one workspace the few-splits grid (one workgroup per oc) and the general grid give bit-identical gradients"""
    dev = _gpu()
    from dasr_amd.engine import WgradGroup, Workspace
    g = torch.Generator().manual_seed(5)
    ws = Workspace(dev)
    if kind == 'wgrad3':
        N, cin, cout, H, W = 2, 96, 80, 12, 20
        x, gy = bf16r(torch.randn(N, cin, H, W, generator=g)), bf16r(torch.randn(N, cout, H, W, generator=g))
        P = params_with_neighbours(dev, [('c.', (cout, cin, 3, 3))])
        xb, gb = blocked16(x, dev, False), blocked16(gy, dev, False)
        grp = _w3_group(P, 'c.', gb, xb, cout, cin, H, W, H, W, N, 0)
        grp.finalize(ws, dev, target_wgs=8)
    else:
        N, cin, cout, H, W = 2, 40, 48, 13, 21
        x, gy = torch.randn(N, cin, H, W, generator=g), torch.randn(N, cout, H, W, generator=g)
        P = params_with_neighbours(dev, [('c.', (cout, cin, 5, 5))])
        xb, gb = to_blocked(x, True, dev), to_blocked(gy, True, dev)
        grp = WgradGroup(5, 1)
        grp.add_conv(gb.view, True, gb.planes, xb.view, True, xb.planes, cout, cin, H, W, H, W, N, P.off('c.weight'), P.off('c.bias'), pad=2)
        grp.finalize(ws, dev, target_wgs=16)
    assert 1 < grp.nsplit <= 4
    ops = grp.ops(P.grad.data_ptr(), scale=0.5)
    assert ops[1].get('few_splits') == 1
    ol = run(ops, ws, P, {'c.weight', 'c.bias'})
    a = P.grad.clone()
    ol.set(1, 'few_splits', 0)
    poison(P, None, {'c.weight', 'c.bias'})
    ol.run(1, 2)
    torch.cuda.synchronize()
    check_neighbours(P, {'c.weight', 'c.bias'})
    assert torch.equal(a.view(torch.int32), P.grad.view(torch.int32))
