"""oracle/conv_ref.py (the fp64 model tests/test_gpu_conv.py holds dasr_conv to) against stock torch in fp64, on a machine without a GPU: F.conv2d,
F.interpolate and autograd on un-rounded operands (rounding=False), or on operands every rounding keeps (small dyadic numbers).  The parity forms
are built with the tables the networks ship: _PARITY_TAPS / _PARITY_PAD (gan_nets.py), _P3_TAPS (dsn_model.py), _SUBPIXEL_ROWS (rrdbnet.py)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import blocked_ref as R
from oracle import conv_ref as CR

TOL = 1e-12   # fp64 against fp64 in another summation order, values O(1)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, tol=TOL):
    return a.shape == b.shape and float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def fwd(x, w, b, stride, pad, pad_x, Ho, Wo):
    """F.conv2d with separate row / column padding, cut to the Ho x Wo outputs the launch asks for"""
    kh = w.shape[2]
    xp = F.pad(x.double(), (pad_x, kh + stride, pad, kh + stride))
    return F.conv2d(xp, w.double(), None if b is None else b.double(), stride=stride)[:, :, :Ho, :Wo]


GEOM = ([(3, 1, p, -1) for p in (0, 1, 2)] + [(3, 2, 1, -1)] + [(4, s, p, -1) for s in (1, 2) for p in (0, 1, 2, 3)] +
        [(2, 1, p, q) for p in (0, 1) for q in (0, 1)] + [(5, 1, 2, -1), (1, 1, 0, -1)])


@pytest.mark.parametrize('kh,stride,pad,pad_x', GEOM, ids=['k%ds%dp%dx%d' % (g[0], g[1], g[2], g[2] if g[3] < 0 else g[3]) for g in GEOM])
def test_every_kernel_size_stride_and_pad_matches_conv2d(kh, stride, pad, pad_x):
    g = gen(kh * 100 + stride * 10 + pad)
    N, cin, cout, H, W = 2, 5, 7, 11, 13
    px = pad if pad_x < 0 else pad_x
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * px - kh) // stride + 1
    w, b, x = torch.randn(cout, cin, kh, kh, generator=g), torch.randn(cout, generator=g), torch.randn(N, cin, H, W, generator=g)
    ref, S, L = CR.conv(w, b, x, Ho, Wo, prec=3, kh=kh, stride=stride, pad=pad, pad_x=pad_x, rounding=False)
    assert close(ref, fwd(x, w, b, stride, pad, px, Ho, Wo))
    assert close(S, fwd(x.abs(), w.abs(), None, stride, pad, px, Ho, Wo)) and L == 3 * kh * kh * cin
    # one output row / column more than the natural size: the extra taps read zero padding
    ref2, _, _ = CR.conv(w, b, x, Ho + 1, Wo + 1, prec=1, kh=kh, stride=stride, pad=pad, pad_x=pad_x, rounding=False)
    assert close(ref2, fwd(x, w, b, stride, pad, px, Ho + 1, Wo + 1))


@pytest.mark.parametrize('prec', [1, 2, 3, 4])
def test_rounded_operands_that_every_format_holds_are_exact(prec):
    """multiples of 1/8 below 4: bf16, f16 and their remainders (zero) hold them, so the rounded model equals the un-rounded conv exactly and S
    counts every product once"""
    g = gen(prec)
    w = torch.randint(-15, 16, (6, 4, 3, 3), generator=g).float() / 8
    x = torch.randint(-15, 16, (2, 4, 6, 9), generator=g).float() / 8
    ref, S, L = CR.conv(w, None, x, 6, 9, prec=prec, in_scale=4096.0)
    assert torch.equal(ref, fwd(x, w, None, 1, 1, 1, 6, 9)) and torch.equal(S, fwd(x.abs(), w.abs(), None, 1, 1, 1, 6, 9))
    assert L == 9 * 4 * (3 if prec >= 3 else 1)


def test_operand_rounding_per_precision():
    """one product: prec 1 / 2 round both operands once; 3 / 4 form hi*hi + hi*lo + lo*hi (no lo*lo); in_scale is applied before the f16 rounding
    and undone on the accumulator (a value below f16's subnormals survives only with it)"""
    wv, xv = 1.2345678, 0.87654321
    w, x = torch.tensor(wv).view(1, 1, 1, 1), torch.tensor(xv).view(1, 1, 1, 1)
    for prec, kind in ((1, 'bf16'), (2, 'f16'), (3, 'bf16'), (4, 'f16')):
        ref, S, L = CR.conv(w, None, x, 1, 1, prec=prec, kh=1, pad=0)
        wh, wl = (t.double() for t in R.split16(w, kind))
        xh, xl = (t.double() for t in R.split16(x, kind))
        want = wh * xh if prec < 3 else wh * xh + wh * xl + wl * xh
        assert torch.equal(ref, want) and L == (1 if prec < 3 else 3)
        assert torch.equal(S, want.abs() if prec < 3 else (wh * xh).abs() + (wh * xl).abs() + (wl * xh).abs())
    tiny = torch.tensor(2e-8).view(1, 1, 1, 1)   # below half of f16's smallest subnormal (2^-25): rounds to zero unscaled
    assert float(CR.conv(w, None, tiny, 1, 1, prec=2, kh=1, pad=0)[0]) == 0.0
    got = float(CR.conv(w, None, tiny, 1, 1, prec=2, kh=1, pad=0, in_scale=4096.0)[0])
    assert abs(got - wv * 2e-8) < 2.0 ** -10 * wv * 2e-8
    # split tensor: the stored planes are the operands
    hi, lo = R.split16(x, 'f16')
    ref, S, L = CR.conv(w, None, hi, 1, 1, prec=2, kh=1, pad=0, x_lo=lo)
    wh, wl = (t.double() for t in R.split16(w, 'f16'))
    assert torch.equal(ref, wh * hi.double() + wh * lo.double() + wl * hi.double()) and L == 3


def test_ups_matches_interpolate_then_conv2d():
    g = gen(3)
    w, b, x = torch.randn(6, 4, 3, 3, generator=g), torch.randn(6, generator=g), torch.randn(2, 4, 5, 7, generator=g)
    ref, _, _ = CR.conv(w, b, x, 10, 14, ups=1, rounding=False)
    assert close(ref, F.conv2d(F.interpolate(x.double(), scale_factor=2, mode='nearest'), w.double(), b.double(), padding=1))


def test_epilogue_order():
    g = gen(4)
    w, b, x = torch.randn(5, 4, 3, 3, generator=g), torch.randn(5, generator=g), torch.randn(2, 4, 6, 7, generator=g)
    m, r1, r2 = (torch.randn(2, 5, 6, 7, generator=g) for _ in range(3))
    m[0, 0, 0, 0], m[0, 1, 0, 0] = 0.0, -0.0
    d = CR.conv_detail(w, b, x, 6, 7, rounding=False, act=1, slope=-0.25, mask=m, alpha=0.3, res1=r1, beta1=-2.0, res2=r2, beta2=0.5)
    y = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    y = torch.where(y > 0, y, -0.25 * y)
    y = y * torch.where(m.double() > 0, 1.0, -0.25)
    assert close(d['ref'], 0.3 * y - 2.0 * r1.double() + 0.5 * r2.double()) and d['gain'] == 0.3
    d = CR.conv_detail(w, b, x, 6, 7, rounding=False, act=2, alpha=2.0)
    assert close(d['ref'], 2.0 * torch.sigmoid(F.conv2d(x.double(), w.double(), b.double(), padding=1))) and d['gain'] == 0.5
    hi, lo = CR.out16(d['ref'], 3.0, 'f16', split=True)
    assert torch.equal(hi, (3.0 * d['ref']).float().half()) and torch.equal(lo, ((3.0 * d['ref']).float() - hi.float()).half())


def _flat(*ws):
    offs, n = [], 0
    for w in ws:
        offs.append(n)
        n += w.numel()
    return torch.cat([w.reshape(-1) for w in ws]), offs


@pytest.mark.parametrize('kh,pad_fwd', [(3, 1), (4, 1), (4, 2), (5, 2), (1, 0)])
def test_stride1_dgrad_pack_matches_autograd(kh, pad_fwd):
    """transposed, tap-reversed pack, pad = kh - 1 - pad_fwd"""
    g = gen(kh)
    cin, cout, H, W = 5, 6, 9, 11
    w = torch.randn(cout, cin, kh, kh, generator=g)
    Ho, Wo = H + 2 * pad_fwd - kh + 1, W + 2 * pad_fwd - kh + 1
    gy = torch.randn(2, cout, Ho, Wo, generator=g)
    x = torch.zeros(2, cin, H, W, dtype=torch.double, requires_grad=True)
    (F.conv2d(x, w.double(), padding=pad_fwd) * gy.double()).sum().backward()
    flat, (o,) = _flat(w)
    wb = CR.pack_weights(flat, cin, cout, kh * kh, [(o, cout, cin, 0, cout, 0, 1)])
    ref, _, _ = CR.conv(wb, None, gy, H, W, kh=kh, pad=kh - 1 - pad_fwd, rounding=False)
    assert close(ref, x.grad)


def test_pack_concatenates_up_to_five_segments():
    """forward: the torch.cat of a dense block as source-channel offsets; data gradient: transposed segments of the later convs side by side"""
    g = gen(8)
    ws = [torch.randn(4, 3 + 2 * k, 3, 3, generator=g) for k in range(5)]   # conv k reads 3 + 2 k channels
    flat, offs = _flat(*ws)
    # one forward conv over [x0 (3) | x1 (2)] assembled from two segments of ws[1]
    wf = CR.pack_weights(flat, 4, 16, 9, [(offs[1], 4, 5, 0, 3, 0, 0), (offs[1], 4, 5, 3, 2, 3, 0)])
    assert torch.equal(wf[:, :5], ws[1].reshape(4, 5, 9)) and float(wf[:, 5:].abs().max()) == 0.0
    # data gradient w.r.t. channels [1, 3) of the input all five convs share: five transposed segments, packed cin = 5 * 4
    wb = CR.pack_weights(flat, 2, 32, 9, [(offs[k], 4, 3 + 2 * k, 4 * k, 4, 1, 1) for k in range(5)])
    gys = [torch.randn(2, 4, 6, 7, generator=g) for _ in range(5)]
    x = torch.zeros(2, 11, 6, 7, dtype=torch.double, requires_grad=True)
    sum((F.conv2d(x[:, :3 + 2 * k], ws[k].double(), padding=1) * gys[k].double()).sum() for k in range(5)).backward()
    gcat = torch.cat(gys + [torch.zeros(2, 12, 6, 7)], dim=1)
    ref, _, L = CR.conv(wb, None, gcat, 6, 7, rounding=False)
    assert close(ref, x.grad[:, 1:3]) and L == 3 * 9 * 32


def _s2_dgrad(kh, taps, pads, hi, wi, seed):
    """the four 2x2 parity sub-convs of a stride-2 data gradient, written with out_stride 2 into one tensor"""
    g = gen(seed)
    cin, cout = 5, 6
    w = torch.randn(cout, cin, kh, kh, generator=g)
    ho, wo = (hi + 2 - kh) // 2 + 1, (wi + 2 - kh) // 2 + 1
    gy = torch.randn(2, cout, ho, wo, generator=g)
    x = torch.zeros(2, cin, hi, wi, dtype=torch.double, requires_grad=True)
    (F.conv2d(x, w.double(), stride=2, padding=1) * gy.double()).sum().backward()
    flat, (o,) = _flat(w)
    out = torch.full((2, cin, hi, wi), float('nan'), dtype=torch.double)
    for py in (0, 1):
        for px in (0, 1):
            tm = [(-1 if (taps[py][a] < 0 or taps[px][b] < 0) else taps[py][a] * kh + taps[px][b]) for a in (0, 1) for b in (0, 1)]
            wb = CR.pack_weights(flat, cin, cout, 4, [(o, cout, cin, 0, cout, 0, 1)], tapmap=tm, src_ntaps=kh * kh)
            hs, wsub = (hi - py + 1) // 2, (wi - px + 1) // 2
            ref, _, _ = CR.conv(wb, None, gy, hs, wsub, kh=2, pad=pads[py], pad_x=pads[px], rounding=False, out_stride=2, out_oy=py, out_ox=px)
            CR.scatter(out, ref, 2, py, px)
    assert close(out, x.grad)


@pytest.mark.parametrize('hi,wi', [(9, 11), (10, 7)])
def test_stride2_4x4_parity_dgrad_matches_autograd(hi, wi):
    from dasr_amd.gan_nets import _PARITY_PAD, _PARITY_TAPS
    _s2_dgrad(4, _PARITY_TAPS, _PARITY_PAD, hi, wi, 21)


@pytest.mark.parametrize('hi,wi', [(9, 11), (10, 7)])
def test_stride2_3x3_parity_dgrad_matches_autograd(hi, wi):
    from dasr_amd.dsn_model import _P3_TAPS
    _s2_dgrad(3, _P3_TAPS, {0: 0, 1: 0}, hi, wi, 22)


def _subpixel_masks():
    from dasr_amd.rrdbnet import _SUBPIXEL_ROWS as rows
    fw = {(py, px): [sum(1 << (ky * 3 + kx) for ky in rows[py][a] for kx in rows[px][b]) for a in (0, 1) for b in (0, 1)] for py in (0, 1) for px in (0, 1)}
    bw = {(py, px): [sum(1 << (ky * 3 + kx) for ky in rows[py][1 - a] for kx in rows[px][1 - b]) for a in (0, 1) for b in (0, 1)]
          for py in (0, 1) for px in (0, 1)}
    return fw, bw


def test_forward_subpixel_parities_match_nearest_then_3x3():
    g = gen(31)
    nf, h, w_ = 5, 5, 7
    w, b, x = torch.randn(nf, nf, 3, 3, generator=g), torch.randn(nf, generator=g), torch.randn(2, nf, h, w_, generator=g)
    flat, (o,) = _flat(w)
    fw, _ = _subpixel_masks()
    out = torch.full((2, nf, 2 * h, 2 * w_), float('nan'), dtype=torch.double)
    for (py, px), masks in fw.items():
        wp = CR.pack_weights(flat, nf, nf, 4, [(o, nf, nf, 0, nf, 0, 0)], tapmap=[0, 0, 0, 0], src_ntaps=9, tapmasks=masks)
        ref, _, _ = CR.conv(wp, b, x, h, w_, kh=2, pad=1 - py, pad_x=1 - px, rounding=False, out_stride=2, out_oy=py, out_ox=px)
        CR.scatter(out, ref, 2, py, px)
    want = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode='nearest'), w.double(), b.double(), padding=1)
    assert close(out, want, 1e-6)   # the packed tap is an fp32 sum of fp32 taps: 2^-24 relative per tap, not an fp64 one


def test_in_stride_transposed_parities_match_autograd():
    """data gradient of nearest-x2 + 3x3: four launches reading the parity sub-grids of the gradient in place, chained through res1 as
    RRDBNet._subpixel_dgrad chains them"""
    g = gen(32)
    nf, h, w_ = 5, 5, 7
    w = torch.randn(nf, nf, 3, 3, generator=g)
    gy = torch.randn(2, nf, 2 * h, 2 * w_, generator=g)
    x = torch.zeros(2, nf, h, w_, dtype=torch.double, requires_grad=True)
    (F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w.double(), padding=1) * gy.double()).sum().backward()
    flat, (o,) = _flat(w)
    _, bw = _subpixel_masks()
    acc = None
    for py in (0, 1):
        for px in (0, 1):
            wp = CR.pack_weights(flat, nf, nf, 4, [(o, nf, nf, 0, nf, 0, 1)], tapmap=[0, 0, 0, 0], src_ntaps=9, tapmasks=bw[(py, px)])
            acc, _, _ = CR.conv(wp, None, gy, h, w_, kh=2, pad=py, pad_x=px, rounding=False, in_stride=2, in_oy=py, in_ox=px, Hin=h, Win=w_,
                                res1=acc, beta1=0.0 if acc is None else 1.0)
    assert close(acc, x.grad, 1e-6)
