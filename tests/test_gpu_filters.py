"""GPU parity tests of the second half of csrc/gan.hip -- the kernels that build the discriminator's input (Haar DWT forward / adjoint, padded and
un-padded depthwise low-pass with its frequency split), the domain-distance map (dasr_ddm_spread, dasr_bilinear_up) and the DSN's -log losses
(dasr_logloss, dasr_sigmoid_bwd) -- in every mode include/dasr_hip.h documents, against the fp64 references of oracle/blocked_ref.py (themselves held
to stock torch and to the adjoint identity by tests/test_blocked_ref.py).

Set-up as in tests/test_gpu_elementwise.py, whose machinery this file shares: every blocked tensor is plane p0 > 0 of a wider sentinel-filled slab and
everything outside the written view must hold the sentinel bit for bit afterwards; input channels from C on hold finite junk; N = 2, H != W, one size
below 256 threads (one partial workgroup) and one above that is no multiple of 256; every case through the ctypes entry point (via = abi) and as a
recorded op through dasr_run_ops (via = op).

What is asserted: |got - ref| <= k u32 magnitude ELEMENTWISE (a wrong border row or corner is one element, which no norm over the tensor shows), k =
the roundings behind an element, derived beside each assertion (a fused multiply-add counted as two; a t-tap sum accumulated in fp32: every term goes
through its product and at most t - 1 additions, t in all); exact zeros / bit-unchanged values in the channels the header says so."""
import math

import pytest
import torch

from oracle import blocked_ref as R
from test_gpu_elementwise import EINVAL, SENT, U32, VIA, Slab, _gpu, _grid_chain, biteq, bounded, call, gen, gpu

N = 2
SMALL, BIG = (5, 7), (13, 19)          # N * H * W = 70: one partial workgroup; 494: a full and a partial one


def full16(x, g):
    """[N][C][H][W] -> the 16 channels of one plane: x, then finite junk (neither zero nor the sentinel)"""
    n, c, h, w = x.shape
    t = torch.randn(n, 16, h, w, generator=g) * 3.0 + 5.0
    t[:, :c] = x.float()
    return t


def plane(dev, x16, lead=1):
    """one plane holding the 16-channel tensor x16 inside a sentinel-filled slab"""
    n, _, h, w = x16.shape
    return Slab(dev, 'f32', n, 1, h, w, R.pack(x16.float()), lead=lead)


def empty(dev, h, w, lead=2):
    return Slab(dev, 'f32', N, 1, h, w, None, lead=lead)


def zeros_from(t, c):
    return biteq(t[:, c:], torch.zeros_like(t[:, c:]))


def nonsym(k, g):
    """a k x k kernel that is no transpose, flip or rotation of itself: pins the tap orientation"""
    w = torch.rand(k, k, generator=g) + 0.1
    assert not torch.equal(w, w.t()) and not torch.equal(w, w.flip(0)) and not torch.equal(w, w.flip(1)) and not torch.equal(w, w.flip(0, 1))
    return w.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_dwt_fwd / dasr_dwt_bwd
NORMS = [0, 1, 2, 3, 5]


@gpu
@VIA
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('Cc', [1, 3, 5])
def test_dwt_fwd(Cc, norm, via, margins):
    dev = _gpu()
    g = gen(200)
    nb = Cc if norm & 2 else 3 * Cc                      # channels of hc
    offset = bool(norm & 1) and not norm & 4
    for H2, W2 in (SMALL, BIG):
        x = torch.randn(N, Cc, 2 * H2, 2 * W2, generator=g)
        xs = plane(dev, full16(x, g))
        (ll, llm), (hc, hcm) = R.dwt(x, norm)
        for outs in ('ll', 'hc', 'both'):
            ls, hs = empty(dev, H2, W2), empty(dev, H2, W2, lead=3)
            kw = dict(x=xs.view(), N=N, C=Cc, H2=H2, W2=W2, norm=norm)
            if outs != 'hc':
                kw['ll'] = ls.view()
            if outs != 'll':
                kw['hc'] = hs.view()
            assert call(via, 'dwt_fwd', **kw) == 0
            tag = 'C%d norm %d %s %dx%d %s' % (Cc, norm, outs, H2, W2, via)
            if outs == 'hc':
                assert ls.untouched()
            else:
                got = ls.nchw()
                # k = 3: the three additions of a + b + c + d; * 0.5 and * 0.5 again are exact
                bounded('dwt_fwd ll ' + tag, got[:, :Cc], ll, 3 * U32 * llm, margins)
                assert zeros_from(got, Cc) and ls.outside_untouched()
            if outs == 'll':
                assert hs.untouched()
            else:
                got = hs.nchw()
                # k: three additions per band, + 0.5 (1, bit 0 without bit 2); the 'sum' format adds two additions and the division by 3 (3)
                k = 3 + int(offset) + (3 if norm & 2 else 0)
                bounded('dwt_fwd hc ' + tag, got[:, :nb], hc, k * U32 * hcm, margins)
                assert zeros_from(got, nb) and hs.outside_untouched()
            assert xs.untouched()


@gpu
@VIA
@pytest.mark.parametrize('Cc', [1, 3, 5])
def test_dwt_fwd_is_exact_on_small_integers(Cc, via):
    """norm 0 on integers in [-8, 8]: every sum and the halving are exact, so the bands are the reference bit for bit"""
    dev = _gpu()
    g = gen(201)
    H2, W2 = BIG
    x = torch.randint(-8, 9, (N, Cc, 2 * H2, 2 * W2), generator=g).float()
    xs, ls, hs = plane(dev, full16(x, g)), empty(dev, H2, W2), empty(dev, H2, W2, lead=3)
    assert call(via, 'dwt_fwd', x=xs.view(), N=N, C=Cc, H2=H2, W2=W2, norm=0, ll=ls.view(), hc=hs.view()) == 0
    (ll, _), (hc, _) = R.dwt(x, 0)
    assert biteq(ls.nchw(Cc), ll.float()) and biteq(hs.nchw(3 * Cc), hc.float())
    assert zeros_from(ls.nchw(), Cc) and zeros_from(hs.nchw(), 3 * Cc) and ls.outside_untouched() and hs.outside_untouched()


@gpu
@VIA
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('Cc', [1, 3, 5])
def test_dwt_bwd(Cc, norm, via, margins):
    dev = _gpu()
    g = gen(202)
    nb = Cc if norm & 2 else 3 * Cc
    for H2, W2 in (SMALL, BIG):
        gll, ghc = torch.randn(N, Cc, H2, W2, generator=g), torch.randn(N, nb, H2, W2, generator=g)
        gls, ghs = plane(dev, full16(gll, g)), plane(dev, full16(ghc, g), lead=2)
        g0 = torch.randn(N, 16, 2 * H2, 2 * W2, generator=g)
        for bands in ('both', 'gll', 'ghc'):
            a, b = (gll if bands != 'ghc' else None), (ghc if bands != 'gll' else None)
            ref, mag = R.dwt_adj(a, b, Cc, norm)
            for acc in (0, 1):
                os_ = plane(dev, g0, lead=3) if acc else empty(dev, 2 * H2, 2 * W2, lead=3)
                kw = dict(N=N, C=Cc, H2=H2, W2=W2, norm=norm, gx=os_.view(), accumulate=acc)
                if a is not None:
                    kw['gll'] = gls.view()
                if b is not None:
                    kw['ghc'] = ghs.view()
                assert call(via, 'dwt_bwd', **kw) == 0
                got = os_.nchw()
                # k: the three additions of l + lh + hl + hh (the scale is a power of two); 'sum' format: the constant 1 / 3 and its product (2);
                # accumulate: the add into gx (1)
                k = 3 + (2 if norm & 2 and b is not None else 0) + acc
                tag = 'C%d norm %d %s acc %d %dx%d %s' % (Cc, norm, bands, acc, H2, W2, via)
                if acc:
                    prev = g0[:, :Cc].double()
                    bounded('dwt_bwd ' + tag, got[:, :Cc], ref + prev, k * U32 * (mag + prev.abs()), margins)
                    assert biteq(got[:, Cc:], g0[:, Cc:])            # += 0: channels from C on keep what they held
                else:
                    bounded('dwt_bwd ' + tag, got[:, :Cc], ref, k * U32 * mag, margins)
                    assert zeros_from(got, Cc)
                assert os_.outside_untouched() and gls.untouched() and ghs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_lowpass
def _weights(name, g):
    """(w [k][k] fp32, mode bit 1, the two sizes)"""
    from oracle.nets import gaussian_kernel2d
    if name == 'gauss5':
        return gaussian_kernel2d(5).contiguous(), 0, (SMALL, BIG)
    if name == 'gauss9':
        return gaussian_kernel2d(9).contiguous(), 0, (SMALL, BIG)
    if name == 'gauss5_nv':
        return gaussian_kernel2d(5).contiguous(), 2, (SMALL, BIG)
    if name == 'nonsym5':
        return nonsym(5, g), 0, (SMALL, BIG)
    # the FSD domain-distance map: on 6 x 9 the window overhangs on all four sides at once
    assert name == 'box17_nv'
    return torch.full((17, 17), 1.0 / 289.0), 2, ((6, 9), (20, 28))


@gpu
@VIA
@pytest.mark.parametrize('Cc', [1, 3, 4])
@pytest.mark.parametrize('wname', ['gauss5', 'gauss9', 'nonsym5', 'box17_nv'])
def test_lowpass_forward(wname, Cc, via, margins):
    dev = _gpu()
    g = gen(203)
    w, nv, sizes = _weights(wname, g)
    k, wd = w.shape[0], w.to(dev)
    a_h, b_h = 0.25, 0.75
    for H, W in sizes:
        x = torch.randn(N, Cc, H, W, generator=g)
        xs = plane(dev, full16(x, g))
        low, mag = R.lowpass(x, w.double(), bool(nv))
        # t = k * k taps: a term goes through its product and at most t - 1 additions; mode bit 1: the fraction's division, its reciprocal and
        # the product with it (c = 3)
        e_low = (k * k + (3 if nv else 0)) * U32 * mag
        for outs in ('low', 'high', 'both'):
            ls, hs = empty(dev, H, W), empty(dev, H, W, lead=3)
            kw = dict(x=xs.view(), w=wd.data_ptr(), k=k, N=N, C=Cc, H=H, W=W, mode=nv, a_h=a_h, b_h=b_h)
            if outs != 'high':
                kw['out_low'] = ls.view()
            if outs != 'low':
                kw['out_high'] = hs.view()
            assert call(via, 'lowpass', **kw) == 0
            tag = '%s C%d %s %dx%d %s' % (wname, Cc, outs, H, W, via)
            if outs == 'high':
                assert ls.untouched()
            else:
                got = ls.nchw()
                bounded('lowpass low ' + tag, got[:, :Cc], low, e_low, margins)
                assert zeros_from(got, Cc) and ls.outside_untouched()
            if outs == 'low':
                assert hs.untouched()
            else:
                got = hs.nchw()
                # a_h * (x - low) + b_h: the error of low times |a_h|, then x - low (1), * a_h (1), + b_h (1) on |a_h| (|x| + |low|) + |b_h|
                bound = a_h * e_low + 3 * U32 * (a_h * (x.double().abs() + mag) + b_h)
                bounded('lowpass high ' + tag, got[:, :Cc], a_h * (x.double() - low) + b_h, bound, margins)
                assert zeros_from(got, Cc) and hs.outside_untouched()
            assert xs.untouched()


@gpu
@VIA
@pytest.mark.parametrize('Cc', [1, 3, 4])
@pytest.mark.parametrize('wname', ['gauss5', 'gauss5_nv', 'box17_nv'])
def test_lowpass_adjoint(wname, Cc, via, margins):
    """mode 1 with symmetric kernels only (the header's contract: the kernel correlates with w where the adjoint correlates with the flipped w)"""
    dev = _gpu()
    g = gen(204)
    w, nv, sizes = _weights(wname, g)
    assert torch.equal(w, w.t()) and torch.equal(w, w.flip(0)) and torch.equal(w, w.flip(1))
    k, wd = w.shape[0], w.to(dev)
    a_h = 0.25
    for H, W in sizes:
        gl, gh = torch.randn(N, Cc, H, W, generator=g), torch.randn(N, Cc, H, W, generator=g)
        gls, ghs = plane(dev, full16(gl, g)), plane(dev, full16(gh, g), lead=2)
        g0 = torch.randn(N, 16, H, W, generator=g)
        for ins in ('both', 'x', 'x2'):
            a, b = (gl if ins != 'x2' else None), (gh if ins != 'x' else None)
            ref, mag = R.lowpass_adj(a, b, w.double(), a_h, bool(nv))
            for acc in (0, 1):
                os_ = plane(dev, g0, lead=3) if acc else empty(dev, H, W, lead=3)
                kw = dict(w=wd.data_ptr(), k=k, N=N, C=Cc, H=H, W=W, mode=1 | nv, a_h=a_h, b_h=99.0, out_low=os_.view(), accumulate=acc)
                if a is not None:
                    kw['x'] = gls.view()
                if b is not None:
                    kw['x2'] = ghs.view()
                assert call(via, 'lowpass', **kw) == 0
                got = os_.nchw()
                # k: t = k * k for a tap sum; mode bit 1: the fraction's division and the division of the weight by it (2); x2 - low(x2), * a_h and the
                # add to low(x) (3); accumulate: the add into the output (1)
                kk = k * k + (2 if nv else 0) + 3 + acc
                tag = '%s C%d %s acc %d %dx%d %s' % (wname, Cc, ins, acc, H, W, via)
                if acc:
                    prev = g0[:, :Cc].double()
                    bounded('lowpass adjoint ' + tag, got[:, :Cc], ref + prev, kk * U32 * (mag + prev.abs()), margins)
                    assert biteq(got[:, Cc:], g0[:, Cc:])            # channels C..3: += 0; channels 4..15: not written
                else:
                    bounded('lowpass adjoint ' + tag, got[:, :Cc], ref, kk * U32 * mag, margins)
                    assert zeros_from(got, Cc)
                assert os_.outside_untouched() and gls.untouched() and ghs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_lowpass_valid
@gpu
@VIA
@pytest.mark.parametrize('Cc', [1, 3])
@pytest.mark.parametrize('mode', [0, 1])
def test_lowpass_valid(mode, Cc, via, margins):
    dev = _gpu()
    g = gen(205)
    k = 5
    w = nonsym(k, g)
    wd = w.to(dev)
    for H, W in ((k, k + 1), BIG):        # H == k: one output row; 13 x 19 -> 9 x 15 (270 threads forward, 494 in the adjoint)
        Ho, Wo = H - k + 1, W - k + 1
        ih, iw, oh, ow = (H, W, Ho, Wo) if mode == 0 else (Ho, Wo, H, W)
        x = torch.randn(N, Cc, ih, iw, generator=g)
        xs = plane(dev, full16(x, g))
        ref, mag = R.lowpass_valid(x, w.double()) if mode == 0 else R.lowpass_valid_adj(x, w.double(), H, W)
        g0 = torch.randn(N, 16, oh, ow, generator=g)
        for acc in (0, 1):
            os_ = plane(dev, g0, lead=2) if acc else empty(dev, oh, ow)
            assert call(via, 'lowpass_valid', x=xs.view(), w=wd.data_ptr(), k=k, N=N, C=Cc, H=H, W=W, mode=mode, out=os_.view(), accumulate=acc) == 0
            got = os_.nchw()
            kk = k * k + acc                   # t = k * k taps; accumulate: the add into the output (1)
            tag = 'mode %d C%d acc %d %dx%d %s' % (mode, Cc, acc, H, W, via)
            if acc:
                prev = g0[:, :Cc].double()
                bounded('lowpass_valid ' + tag, got[:, :Cc], ref + prev, kk * U32 * (mag + prev.abs()), margins)
                assert biteq(got[:, Cc:], g0[:, Cc:])
            else:
                bounded('lowpass_valid ' + tag, got[:, :Cc], ref, kk * U32 * mag, margins)
                assert zeros_from(got, Cc)
            assert os_.outside_untouched() and xs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_ddm_spread
@gpu
@VIA
@pytest.mark.parametrize('hw', [(24, 32), (32, 40)], ids=['24x32', '32x40'])
@pytest.mark.parametrize('arch', ['nld_s1', 'nld_s2'])
def test_ddm_spread(arch, hw, via, margins):
    from oracle.dsn_dataset import CONVNETS, receptive
    dev = _gpu()
    g = gen(206)
    H, W = hw
    n_h, n_w = receptive(H, CONVNETS[arch])[0], receptive(W, CONVNETS[arch])[0]
    d = torch.rand(N, 1, n_h, n_w, generator=g)
    ref, mag, cnt, (nh, nw, jump, rf, start) = R.ddm_spread(d, H, W, CONVNETS[arch])
    assert (nh, nw) == (n_h, n_w) and float(cnt.min()) >= 1
    ds, os_ = plane(dev, full16(d, g)), empty(dev, H, W)
    assert call(via, 'ddm_spread', d=ds.view(), N=N, n_h=n_h, n_w=n_w, H=H, W=W, jump=jump, rf=rf, start=float(start), out=os_.view()) == 0
    got = os_.nchw()
    # a pixel under c windows: c - 1 additions and the division by c (the count itself is a small integer: exact) are c roundings, and one to spare.
    # The magnitude is the mean of |d| over those windows: the sum's error is divided by c with the sum
    bounded('ddm_spread %s %dx%d %s' % (arch, H, W, via), got[:, :1], ref, (cnt + 1) * U32 * mag, margins)
    assert zeros_from(got, 1) and os_.outside_untouched() and ds.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_bilinear_up: plain NCHW [N][1][h][w] buffers
@gpu
@VIA
@pytest.mark.parametrize('hw', [(2, 3), (7, 9), (1, 6), (6, 1)], ids=['2x3', '7x9', '1x6', '6x1'])
@pytest.mark.parametrize('f', [2, 3, 4])
def test_bilinear_up(f, hw, via, margins):
    dev = _gpu()
    g = gen(207)
    h, w = hw
    G = 64                                                          # guard words in front of and behind both buffers
    src = torch.randn(N, 1, h, w, generator=g)
    sb, db = torch.full((G + src.numel() + G,), SENT, device=dev), torch.full((G + src.numel() * f * f + G,), SENT, device=dev)
    sb[G:G + src.numel()] = src.flatten().to(dev)
    sb0 = sb.clone()
    assert call(via, 'bilinear_up', src=sb.data_ptr() + 4 * G, N=N, h=h, w=w, factor=f, dst=db.data_ptr() + 4 * G) == 0
    ref, mag = R.bilinear_up(src, f)
    got = db[G:G + ref.numel()].cpu().view(ref.shape)
    # factors 2 and 4: 1 / f, the source coordinate, the weight l and 1 - l are all exact; a corner goes through its product with the column weight,
    # the add of the row's two terms, the product with the row weight and the add of the two rows: k = 4
    bound = 4 * U32 * mag
    if f == 3:
        # inv = fl(1 / 3) is off by at most u relative; (o + 0.5) * inv is rounded (u), the subtraction of 0.5 rounds a value no larger than that
        # product (u): the source coordinate is off by at most 3 u (o + 0.5) / 3 = u (o + 0.5).  The interpolant is continuous and piecewise linear in the
        # coordinate (also where the perturbed coordinate falls into the neighbouring cell), with slope at most the largest difference between
        # vertical / horizontal neighbours of the image: that error is at most u ((y + 0.5) Gy + (x + 0.5) Gx).  l = s - floor(s) is exact, 1 - l is
        # rounded: k = 5
        s = src.double()
        gy = s.diff(dim=2).abs().amax((1, 2, 3), keepdim=True) if h > 1 else torch.zeros(N, 1, 1, 1, dtype=torch.float64)
        gx = s.diff(dim=3).abs().amax((1, 2, 3), keepdim=True) if w > 1 else torch.zeros(N, 1, 1, 1, dtype=torch.float64)
        oy = (torch.arange(h * f, dtype=torch.float64) + 0.5).view(1, 1, -1, 1)
        ox = (torch.arange(w * f, dtype=torch.float64) + 0.5).view(1, 1, 1, -1)
        bound = 5 * U32 * mag + U32 * (oy * gy + ox * gx)
    bounded('bilinear_up f%d %dx%d %s' % (f, h, w, via), got, ref, bound, margins)
    dc = db.cpu()
    assert bool((dc[:G] == SENT).all()) and bool((dc[G + ref.numel():] == SENT).all()) and biteq(sb, sb0)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_logloss
def _logloss_bounds(v, mode, eps):
    """first-order error bounds, in units of u32, of the kernel's per-pixel p, loss and d loss / d logit (before gcoef) for fp32 logits v.
    p = 1 / (1 + expf(-v)): expf is accurate to 1 ulp = 2 u (the device math library's documented bound; it enters p with the factor e / (1 + e) <= 1),
    1 + e (1), the division (1): 4 u p, as test_sigmoid_fwd has it.
    mode 0: s = p + eps is rounded (1): |ds| <= 4 u p + u s; logf is accurate to 1 ulp = 2 u of its result and passes ds with 1 / s -- the condition
    factor 1 / (p + eps) on the error of p:                     |dl| <= u (4 p / s + 1) + 2 u |l|
    mode 1: q = 1 - p is rounded (1): |dq| <= 4 u p + u q; s = q + eps (1):  |dl| <= u ((4 p + q) / s + 1) + 2 u |l|        (condition factor 1 / (1 - p + eps))
    gradient -+ p q / s: p (4 u), q (4 u p / q + u), the product (1), s as above, the division (1), * gcoef (1), relative to |g|."""
    l, p, gr = R.logloss(v, mode, eps)
    q = 1.0 - p
    s = (p if mode == 0 else q) + eps
    rel_s = (4.0 * p if mode == 0 else 4.0 * p + q) / s + 1.0
    e_l = rel_s + 2.0 * l.abs()
    e_g = (4.0 + (4.0 * p / q + 1.0) + 1.0 + rel_s + 1.0 + 1.0) * gr.abs()
    return l, p, gr, 4.0 * p, e_l, e_g


@gpu
@VIA
@pytest.mark.parametrize('eps', [1e-8, 1e-3])
@pytest.mark.parametrize('mode', [0, 1])
def test_logloss(mode, eps, via, margins):
    dev = _gpu()
    g = gen(208)
    eps = R.f32(eps)
    for H, W in (SMALL, BIG):
        cnt = N * H * W
        v = torch.rand(N, 1, H, W, generator=g) * 12.0 - 6.0       # logits in [-6, 6]: the expression is well-conditioned
        xs = plane(dev, full16(v, g))
        coef, gcoef, scoef, acc0 = R.f32(1.0 / cnt), R.f32(0.3 / cnt), R.f32(0.7 / cnt), 0.25
        l, p, gr, e_p, e_l, e_g = _logloss_bounds(v, mode, eps)
        Lc = _grid_chain((cnt + 255) // 256)                       # one term per thread, then the workgroup and grid chain (coef and the add included)
        g0 = torch.randn(N, 16, H, W, generator=g)
        for grad in (None, 0, 1):
            for accs in ('loss', 'score', 'both'):
                acc = torch.full((4,), acc0, device=dev)
                gs = plane(dev, g0, lead=2) if grad == 1 else empty(dev, H, W)
                kw = dict(x=xs.view(), N=N, H=H, W=W, mode=mode, eps=eps, coef=coef, gcoef=gcoef, score_coef=scoef)
                if accs != 'score':
                    kw['loss_acc'] = acc.data_ptr()
                if accs != 'loss':
                    kw['score_acc'] = acc.data_ptr() + 4
                if grad is not None:
                    kw.update(grad=gs.view(), accumulate=grad)
                assert call(via, 'logloss', **kw) == 0
                tag = 'mode %d eps %g grad %s %s %dx%d %s' % (mode, eps, grad, accs, H, W, via)
                accc = acc.cpu().double()
                for slot, on, cf, val, e_val in ((0, accs != 'score', coef, l, e_l), (1, accs != 'loss', scoef, p, e_p)):
                    if not on:
                        assert float(accc[slot]) == acc0
                        continue
                    # the per-pixel errors, summed, plus the grid-sum convention L u32 (coef sum |terms| + what the accumulator held)
                    want = acc0 + cf * float(val.sum())
                    bound = U32 * cf * float(e_val.sum()) + Lc * U32 * (cf * float(val.abs().sum()) + acc0)
                    err = abs(float(accc[slot]) - want)
                    margins('elementwise logloss %s %s: |err| / bound %.3f (L %d)' % (tag, 'loss' if slot == 0 else 'score', err / bound, Lc))
                    assert err <= bound, (tag, slot, err, bound)
                assert bool((accc[2:] == acc0).all())
                if grad is None:
                    assert gs.untouched()
                    continue
                got = gs.nchw()
                if grad:       # + the add into the gradient (1)
                    prev = g0[:, :1].double()
                    bounded('logloss grad ' + tag, got[:, :1], gcoef * gr + prev, U32 * gcoef * e_g + U32 * (gcoef * gr.abs() + prev.abs()), margins)
                    assert biteq(got[:, 1:], g0[:, 1:])              # channels 1..3: += 0; channels 4..15: not written
                else:
                    bounded('logloss grad ' + tag, got[:, :1], gcoef * gr, U32 * gcoef * e_g, margins)
                    assert zeros_from(got, 1)
                assert gs.outside_untouched() and xs.untouched()


@gpu
@VIA
def test_logloss_saturated_logits_stay_finite(via):
    """logits +-30 and +-100, one pixel per launch with coef 1 into a zeroed accumulator (the sum of one term and zeros is that term): the loss is finite
    and inside [-log(1 + eps), -log(eps)] up to the rounding of the sum and of logf, the gradient is finite and has the sign of the mode"""
    dev = _gpu()
    for eps in (R.f32(1e-8), R.f32(1e-3)):
        lo, hi = -math.log(1.0 + eps), -math.log(eps)
        tiny = 4 * U32 * max(1.0, hi)                              # s = p + eps rounded (1), logf 1 ulp (2), one to spare
        for mode in (0, 1):
            for logit in (-100.0, -30.0, 30.0, 100.0):
                x16 = torch.full((1, 16, 1, 1), 3.0)
                x16[0, 0, 0, 0] = logit
                xs = Slab(dev, 'f32', 1, 1, 1, 1, R.pack(x16))
                gs = Slab(dev, 'f32', 1, 1, 1, 1, None, lead=2)
                acc = torch.zeros(4, device=dev)
                assert call(via, 'logloss', x=xs.view(), N=1, H=1, W=1, mode=mode, eps=eps, coef=1.0, gcoef=1.0, loss_acc=acc.data_ptr(), grad=gs.view()) == 0
                loss, gv = float(acc[0]), float(gs.nchw()[0, 0, 0, 0])
                assert math.isfinite(loss) and lo - tiny <= loss <= hi + tiny, (mode, eps, logit, loss)
                assert math.isfinite(gv) and (gv <= 0.0 if mode == 0 else gv >= 0.0), (mode, eps, logit, gv)
                assert zeros_from(gs.nchw(), 1) and gs.outside_untouched() and xs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_sigmoid_bwd
@gpu
@VIA
@pytest.mark.parametrize('Cc', [1, 3, 4])
def test_sigmoid_bwd(Cc, via, margins):
    dev = _gpu()
    g = gen(209)
    for H, W in (SMALL, BIG):
        y, go = torch.rand(N, Cc, H, W, generator=g), torch.randn(N, Cc, H, W, generator=g)
        ys, gs, zs = plane(dev, full16(y, g)), plane(dev, full16(go, g), lead=2), empty(dev, H, W, lead=3)
        assert call(via, 'sigmoid_bwd', y=ys.view(), g=gs.view(), N=N, C=Cc, H=H, W=W, gz=zs.view()) == 0
        ref, mag = R.sigmoid_bwd(y, go)
        got = zs.nchw()
        # three roundings: g * y, 1 - y, their product
        bounded('sigmoid_bwd C%d %dx%d %s' % (Cc, H, W, via), got[:, :Cc], ref, 3 * U32 * mag, margins)
        # channels from C on of plane 0: zero; the planes behind it (and in front) are not touched
        assert zeros_from(got, Cc) and zs.outside_untouched() and ys.untouched() and gs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# argument checks: each returns DASR_EINVAL before any launch and leaves every slab as it was
@gpu
@VIA
def test_dwt_argument_checks(via):
    dev = _gpu()
    H2, W2 = SMALL
    xs, ls, hs = empty(dev, 2 * H2, 2 * W2, lead=1), empty(dev, H2, W2), empty(dev, H2, W2, lead=3)
    dims = dict(N=N, H2=H2, W2=W2, norm=1)
    assert call(via, 'dwt_fwd', C=3, ll=ls.view(), hc=hs.view(), **dims) == EINVAL                       # x null
    assert call(via, 'dwt_fwd', x=xs.view(), C=3, **dims) == EINVAL                                      # both outputs null
    assert call(via, 'dwt_fwd', x=xs.view(), C=0, ll=ls.view(), hc=hs.view(), **dims) == EINVAL
    assert call(via, 'dwt_fwd', x=xs.view(), C=-1, ll=ls.view(), hc=hs.view(), **dims) == EINVAL
    assert call(via, 'dwt_bwd', gll=ls.view(), ghc=hs.view(), C=3, accumulate=0, **dims) == EINVAL       # gx null
    assert call(via, 'dwt_bwd', gx=xs.view(), C=3, accumulate=0, **dims) == EINVAL                       # both inputs null
    assert call(via, 'dwt_bwd', gll=ls.view(), ghc=hs.view(), gx=xs.view(), C=0, accumulate=0, **dims) == EINVAL
    assert xs.untouched() and ls.untouched() and hs.untouched()


@gpu
@VIA
def test_lowpass_argument_checks(via):
    dev = _gpu()
    H, W = SMALL
    xs, x2s, ls, hs = empty(dev, H, W, lead=1), empty(dev, H, W), empty(dev, H, W, lead=3), empty(dev, H, W)
    wd = torch.full((25,), 0.04, device=dev)
    base = dict(w=wd.data_ptr(), k=5, N=N, C=3, H=H, W=W, a_h=0.5, b_h=0.5)

    def rc(**kw):
        return call(via, 'lowpass', **dict(base, **kw))
    assert rc(mode=0, out_low=ls.view(), out_high=hs.view()) == EINVAL                                   # mode 0 without x
    assert rc(mode=0, x=xs.view()) == EINVAL                                                             # mode 0 without an output
    assert rc(mode=1, x=xs.view(), x2=x2s.view()) == EINVAL                                              # mode 1 without out_low
    assert rc(mode=1, out_low=ls.view()) == EINVAL                                                       # mode 1 without an input
    assert rc(mode=3, out_low=ls.view()) == EINVAL
    for k in (0, -1, -3):                                                                                # (a negative odd k passes k & 1)
        assert rc(mode=0, x=xs.view(), out_low=ls.view(), k=k) == EINVAL
    for Cc in (0, -1):
        assert rc(mode=0, x=xs.view(), out_low=ls.view(), C=Cc) == EINVAL
    assert rc(mode=0, x=xs.view(), out_low=ls.view(), w=None) == EINVAL
    assert xs.untouched() and x2s.untouched() and ls.untouched() and hs.untouched()
    # lowpass_valid
    for mode in (0, 1):
        ok = dict(x=xs.view(), w=wd.data_ptr(), k=5, N=N, C=3, H=H, W=W, mode=mode, out=ls.view())
        for bad in (dict(x=None), dict(out=None), dict(w=None), dict(k=0), dict(k=-1), dict(mode=2 + mode), dict(mode=-1)):
            assert call(via, 'lowpass_valid', **dict(ok, **bad)) == EINVAL, bad
    assert xs.untouched() and ls.untouched()


@gpu
@VIA
def test_loss_and_map_argument_checks(via):
    dev = _gpu()
    H, W = SMALL
    xs, gs, zs = empty(dev, H, W, lead=1), empty(dev, H, W), empty(dev, H, W, lead=3)
    acc = torch.full((4,), SENT, device=dev)
    ok = dict(x=xs.view(), N=N, H=H, W=W, mode=0, eps=1e-8, coef=1.0, gcoef=1.0, loss_acc=acc.data_ptr(), score_acc=acc.data_ptr() + 4, score_coef=1.0,
              grad=gs.view())
    for bad in (dict(x=None), dict(mode=2), dict(mode=-1)):
        assert call(via, 'logloss', **dict(ok, **bad)) == EINVAL, bad
    assert bool((acc.cpu() == SENT).all()) and xs.untouched() and gs.untouched()
    ok = dict(y=xs.view(), g=gs.view(), N=N, C=3, H=H, W=W, gz=zs.view())
    for bad in (dict(y=None), dict(g=None), dict(gz=None)):
        assert call(via, 'sigmoid_bwd', **dict(ok, **bad)) == EINVAL, bad
    assert xs.untouched() and gs.untouched() and zs.untouched()
    src, dst = torch.full((N * H * W,), SENT, device=dev), torch.full((N * H * W * 16,), SENT, device=dev)
    ok = dict(src=src.data_ptr(), N=N, h=H, w=W, factor=2, dst=dst.data_ptr())
    for bad in (dict(src=None), dict(dst=None), dict(factor=0), dict(factor=-2)):      # (total = N h w f^2 is positive for a negative factor)
        assert call(via, 'bilinear_up', **dict(ok, **bad)) == EINVAL, bad
    assert bool((src.cpu() == SENT).all()) and bool((dst.cpu() == SENT).all())
