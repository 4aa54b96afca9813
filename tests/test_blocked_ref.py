"""CPU checks of oracle/blocked_ref.py, the references tests/test_gpu_elementwise.py and tests/test_gpu_filters.py trust, against stock torch: they
run where no kernel can."""
import pytest
import torch
import torch.nn.functional as F

from oracle import blocked_ref as R


def gen(seed):
    return torch.Generator().manual_seed(seed)


def tied(shape, g):
    """multiples of 0.5 in [-2, 2]: tied maxima at positive values are common"""
    return torch.randint(-4, 5, shape, generator=g).double() * 0.5


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('C', [3, 20, 40])
def test_layout_round_trip(kind, C):
    x = R.r16(torch.randn(2, C, 5, 7, generator=gen(1)), kind).float() if kind != 'f32' else torch.randn(2, C, 5, 7, generator=gen(1))
    t = R.pack(x, kind, pad=7.0)
    K = R.planes(C)
    assert t.shape == (2, K, 5, 7, 16) and t.dtype == R.DTYPE[kind] and t.is_contiguous()
    assert torch.equal(R.unpack(t, C).float(), x)
    assert float(t[1, C // 16, 4, 6, C % 16 - 1]) == float(x[1, C - 1, 4, 6])          # channel c lives at plane c // 16, slot c % 16
    if C % 16:
        assert bool((R.unpack(t)[:, C:].float() == 7.0).all())                        # the padding channels hold `pad`


@pytest.mark.parametrize('kind', ['bf16', 'f16'])
def test_split_form(kind):
    v = torch.randn(2, 20, 3, 5, generator=gen(2))
    hi, lo = R.split16(v, kind)
    assert torch.equal(hi, R.r16(v, kind)) and torch.equal(lo, R.r16(v - hi.float(), kind))
    # hi + lo carries twice the mantissa bits: the remainder is below half an ulp of hi, and what is left after lo below half an ulp of that
    assert bool(((v.double() - hi.double() - lo.double()).abs() <= R.U16[kind] ** 2 * v.double().abs() + R.TINY16[kind]).all())
    t = R.pack_split(hi, lo)
    assert t.shape == (2, 4, 3, 5, 16)
    h2, l2 = R.unpack_split(t, 20)
    assert torch.equal(h2, hi) and torch.equal(l2, lo)
    assert torch.equal(t[:, 2:], R.pack(lo, kind))                                    # K hi planes, then K lo planes


def test_r16_is_torch_rounding_and_err16_bounds_it():
    x = torch.cat([torch.randn(4096, generator=gen(3)), torch.randn(4096, generator=gen(4)) * 2.0 ** -20])
    for kind in ('f16', 'bf16'):
        r = R.r16(x, kind)
        assert r.dtype == R.DTYPE[kind]
        assert bool(((r.double() - x.double()).abs() <= R.err16(x.double(), kind)).all())
    assert R.f32(0.3) != 0.3 and R.f32(0.3) == float(torch.tensor(0.3, dtype=torch.float32))


@pytest.mark.parametrize('C4', [64, 192])
def test_pixel_shuffle_and_adjoint(C4):
    x = torch.randn(2, C4, 3, 5, generator=gen(5), dtype=torch.float64).requires_grad_(True)
    y = F.pixel_shuffle(x, 2)
    assert torch.equal(R.pixel_shuffle(x.detach()), y.detach())
    g = torch.randn(y.shape, generator=gen(6), dtype=torch.float64)
    y.backward(g)
    v, mag = R.pixel_unshuffle(g)
    assert torch.equal(v, x.grad) and torch.equal(mag, x.grad.abs())
    assert torch.equal(R.pixel_unshuffle(R.pixel_shuffle(x.detach()))[0], x.detach())
    # with the LeakyReLU' of the activated shuffle input
    a = F.leaky_relu(x.detach(), 0.25).requires_grad_(False)
    pre = x.detach().clone().requires_grad_(True)
    F.pixel_shuffle(F.leaky_relu(pre, 0.25), 2).backward(g)
    assert torch.equal(R.pixel_unshuffle(g, a, 0.25)[0], pre.grad)


@pytest.mark.parametrize('hw', [(2, 2), (3, 3), (6, 10), (7, 11), (12, 9)])
@pytest.mark.parametrize('relu', [False, True])
def test_maxpool_fwd_bwd_with_ties(hw, relu):
    H, W = hw
    pre = tied((2, 5, H, W), gen(7)).requires_grad_(True)
    x = F.relu(pre) if relu else pre
    y = F.max_pool2d(x, 2)
    gy = torch.randn(y.shape, generator=gen(8), dtype=torch.float64)
    y.backward(gy)
    xd = x.detach()
    yy, _, am = R.maxpool2(xd)
    assert torch.equal(yy, y.detach())
    if H * W > 9:
        cand = torch.stack([xd[:, :, dy:2 * (H // 2):2, dx:2 * (W // 2):2] for dy in (0, 1) for dx in (0, 1)], -1)
        ties = ((cand == yy.unsqueeze(-1)).sum(-1) > 1) & (yy > 0)
        assert float(ties.double().mean()) > 0.1                                      # the inputs do exercise the tie-break
    gx, _, untouched = R.maxpool2_bwd(xd, gy, relu_mask=relu)
    # autograd routes through relu(pre): the same as relu_mask on the pooled maximum, except that torch also passes gradient to a maximum of exactly 0
    # from pre == 0 ... which relu' (0 at 0) then removes again: identical
    assert torch.equal(gx, pre.grad)
    assert bool((gx[:, :, untouched] == 0).all()) and int(untouched.sum()) == H * W - (H // 2 * 2) * (W // 2 * 2)


@pytest.mark.parametrize('kind', ['f16', 'bf16'])
def test_maxpool_split_compares_hi_plus_lo(kind):
    g = gen(9)
    v = (tied((2, 4, 6, 8), g) + torch.randint(-3, 4, (2, 4, 6, 8), generator=g).double() * 2.0 ** -14).float()
    hi, lo = R.split16(v, kind)
    assert torch.equal(hi.double() + lo.double(), v.double()) and bool((lo.float() != 0).any())
    yh, yl, am = R.maxpool2(hi, lo)
    assert torch.equal(yh.double() + yl.double(), F.max_pool2d(v.double(), 2))       # the pair of the maximum of hi + lo, unchanged
    _, _, am_hi = R.maxpool2(hi)
    assert bool((am != am_hi).any())                                                  # ... which hi alone does not find
    gy = torch.randn(2, 4, 3, 4, generator=g)
    gh, gl = R.split16(gy, kind)
    vv = v.double().requires_grad_(True)
    F.max_pool2d(vv, 2).backward(gh.double())
    gxh, gxl, _ = R.maxpool2_bwd(hi, gh, lo, gl)
    # ties of hi + lo: torch's CPU max-pool also takes the first maximum in scan order
    assert torch.equal(gxh.double(), vv.grad) and gxh.dtype == gh.dtype
    vv.grad = None
    F.max_pool2d(vv, 2).backward(gl.double())
    assert torch.equal(gxl.double(), vv.grad)


def test_downsum_is_four_times_avgpool():
    s = torch.randn(2, 20, 6, 10, generator=gen(10), dtype=torch.float64)
    v, mag = R.downsum2x(s)
    assert torch.allclose(v, F.avg_pool2d(s, 2) * 4, rtol=0, atol=1e-14) and torch.allclose(mag, F.avg_pool2d(s.abs(), 2) * 4, rtol=0, atol=1e-14)
    m = torch.randn(2, 20, 3, 5, generator=gen(11), dtype=torch.float64)
    m[0, 0, 0, 0], m[0, 0, 0, 1] = 0.0, -0.0
    v2, mag2 = R.downsum2x(s, m, 0.2, 0.5)
    want = torch.where(m > 0, v, v * 0.2) * 0.5
    assert torch.allclose(v2, want, rtol=0, atol=1e-14) and float(v2[0, 0, 0, 0]) == float(v[0, 0, 0, 0] * 0.2 * 0.5)
    assert bool((mag2 >= v2.abs() - 1e-14).all())
    # the adjoint of nearest-x2 upsampling
    lo = torch.randn(2, 20, 3, 5, generator=gen(12), dtype=torch.float64).requires_grad_(True)
    F.interpolate(lo, scale_factor=2, mode='nearest').backward(s)
    assert torch.allclose(v, lo.grad, rtol=0, atol=1e-14)


def test_axpby_affine_sigmoid_add():
    g = gen(13)
    x, z, m = (torch.randn(2, 20, 3, 5, generator=g) for _ in range(3))
    m[0, 0, 0, 0], m[0, 0, 0, 1] = 0.0, -0.0
    v, mag = R.axpby(x, 0.5, z, -1.25, m, 0.2)
    md = m.double().requires_grad_(True)
    F.leaky_relu(md, 0.2).sum().backward()                                            # LeakyReLU' as autograd has it: `slope` at +0 and -0
    assert torch.equal(R.lrelu_dash(m, 0.2), md.grad) and float(md.grad[0, 0, 0, 0]) == 0.2 and float(md.grad[0, 0, 0, 1]) == 0.2
    assert torch.allclose(v, (0.5 * x.double() + -1.25 * z.double()) * md.grad, rtol=0, atol=1e-15)
    assert bool((mag >= v.abs() - 1e-15).all())
    v1, mag1 = R.axpby(x, 2.0)
    assert torch.equal(v1, 2.0 * x.double()) and torch.equal(mag1, v1.abs())
    xa = torch.randn(2, 3, 4, 5, generator=g)
    va, ma = R.affine4(xa, [2.0, 0.3, -1.0, 9.0], [0.1, 0.2, 0.3, 9.0])
    sc = torch.tensor([R.f32(2.0), R.f32(0.3), R.f32(-1.0)], dtype=torch.float64).view(1, 3, 1, 1)
    sh = torch.tensor([R.f32(0.1), R.f32(0.2), R.f32(0.3)], dtype=torch.float64).view(1, 3, 1, 1)
    assert torch.equal(va, xa.double() * sc + sh) and bool((ma >= va.abs()).all())
    y0 = torch.randn(2, 3, 4, 5, generator=g)
    assert torch.equal(R.affine4(xa, [2.0, 0.3, -1.0, 9.0], [0.1, 0.2, 0.3, 9.0], y0)[0], va + y0.double())
    lg = torch.linspace(-30, 30, 121, dtype=torch.float64).view(1, 1, 11, 11)
    assert torch.allclose(R.sigmoid(lg)[0], torch.sigmoid(lg), rtol=1e-15, atol=0)
    a, b = torch.randn(1000, generator=g), torch.randn(1000, generator=g)
    assert torch.equal(R.add_flat(a, b)[0].float(), a + b)                            # the fp64 sum, rounded once, is the fp32 sum


@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('weighted', [False, True])
def test_pixel_and_feature_losses(squared, weighted):
    g = gen(14)
    sr = torch.rand(2, 3, 5, 7, generator=g, dtype=torch.float64)
    hr = torch.rand(2, 3, 5, 7, generator=g, dtype=torch.float64)
    hr[0, 1, 2, 3] = sr[0, 1, 2, 3]                                                   # a == b: the sign gradient there is exactly 0
    wm = torch.rand(2, 1, 5, 7, generator=g, dtype=torch.float64) if weighted else None
    coef = 1.0 / sr.numel()
    s = sr.clone().requires_grad_(True)
    fn = F.mse_loss if squared else F.l1_loss
    w = torch.ones_like(sr) if wm is None else wm.expand_as(sr)
    loss = (fn(s, hr, reduction='none') * w).sum() * coef
    loss.backward()
    l, lmag, gr, gmag = R.l1_loss(sr, hr, coef, wm, squared)
    assert abs(l - float(loss.detach())) <= 1e-15 and abs(lmag - l) <= 1e-15
    assert torch.allclose(gr, s.grad, rtol=0, atol=1e-17) and float(gr[0, 1, 2, 3]) == 0.0 and torch.equal(gmag, gr.abs())
    if not weighted:
        s.grad = None
        loss = fn(s, hr, reduction='sum') * coef
        (loss * 3.0).backward()
        l2, lmag2, ga, _ = R.l1_diff(sr, hr, coef, 3.0 * coef, squared)
        assert abs(l2 - float(loss.detach())) <= 1e-15 and abs(lmag2 - l2) <= 1e-15 and torch.allclose(ga, s.grad, rtol=0, atol=1e-17)


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adam_matches_torch_and_its_error_bound_is_tight(wd):
    g = gen(15)
    n = 1000
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    lr, b1, b2, eps = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8)
    pt = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for gg in grads:
        pt.grad = gg.double().clone()
        opt.step()
    p, m, v, Ep, Em, Ev = R.adam(p0, grads, lr, b1, b2, eps, wd)
    st = opt.state[pt]
    assert torch.allclose(p, pt.detach(), rtol=1e-13, atol=1e-15)
    assert torch.allclose(m, st['exp_avg'], rtol=1e-13, atol=1e-16) and torch.allclose(v, st['exp_avg_sq'], rtol=1e-13, atol=1e-18)
    # the running error bound is a bound: torch's own fp32 Adam sits inside it ...
    p32 = p0.clone().requires_grad_(True)
    o32 = torch.optim.Adam([p32], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for gg in grads:
        p32.grad = gg.clone()
        o32.step()
    assert bool(((p32.detach().double() - p).abs() <= R.U32 * Ep).all())
    # ... and is tighter than the rtol 1e-5 / atol 1e-7 the end-to-end test of the kernel uses
    assert bool((R.U32 * Ep <= 1e-7 + 1e-5 * p.abs()).all()) and float((R.U32 * Ep).max()) < 2e-6
    assert bool((Em >= 0).all()) and bool((Ev >= 0).all())


# ---- the frequency-split, domain-distance-map and DSN loss references -------------------------------------------------------------------
def dot(a, b):
    return float((a.double() * b.double()).sum())


def same_dot(lhs, rhs):
    """<A x, g> == <x, A^T g> to 1e-12 relative"""
    return abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


def nonsym(k, g):
    """a k x k kernel that is no transpose, flip or rotation of itself"""
    w = torch.rand(k, k, generator=g, dtype=torch.float64) + 0.1
    assert not torch.equal(w, w.t()) and not torch.equal(w, w.flip(0)) and not torch.equal(w, w.flip(1)) and not torch.equal(w, w.flip(0, 1))
    return w


@pytest.mark.parametrize('C', [1, 3, 5])
@pytest.mark.parametrize('norm', [0, 1, 2, 3, 5])
def test_dwt_matches_haar_and_its_adjoint(norm, C):
    from oracle.nets import HaarDWT
    g = gen(20)
    x = torch.randn(2, C, 10, 14, generator=g, dtype=torch.float64)
    ll0, hc0 = HaarDWT()(x)
    (ll, llm), (hc, hcm) = R.dwt(x, norm)
    s, off = (0.5 if norm & 1 else 1.0), (0.5 if norm in (1, 3) else 0.0)
    want = hc0 * s + off
    if norm & 2:
        want = (want[:, :C] + want[:, C:2 * C] + want[:, 2 * C:]) / 3.0
    assert torch.allclose(ll, ll0 * s, rtol=0, atol=1e-15) and torch.allclose(hc, want, rtol=0, atol=1e-15)
    assert hc.shape[1] == (C if norm & 2 else 3 * C) and bool((llm >= ll.abs() - 1e-15).all()) and bool((hcm >= hc.abs() - 1e-15).all())
    # the adjoint of the linear part (norm | 4 drops the offset), with both bands, one band and the other
    (lin_ll, _), (lin_hc, _) = R.dwt(x, norm | 4)
    gll, ghc = torch.randn(ll.shape, generator=g, dtype=torch.float64), torch.randn(hc.shape, generator=g, dtype=torch.float64)
    for a, b in ((gll, ghc), (gll, None), (None, ghc)):
        gx, gm = R.dwt_adj(a, b, C, norm)
        lhs = (dot(lin_ll, a) if a is not None else 0.0) + (dot(lin_hc, b) if b is not None else 0.0)
        assert same_dot(lhs, dot(x, gx)) and bool((gm >= gx.abs() - 1e-15).all())
    xr = x.clone().requires_grad_(True)
    l2, h2 = HaarDWT()(xr)
    hs = (h2 * s).view(2, 3, C, 5, 7).sum(1) / 3.0 if norm & 2 else h2 * s
    ((l2 * s * gll).sum() + (hs * ghc).sum()).backward()
    assert torch.allclose(R.dwt_adj(gll, ghc, C, norm)[0], xr.grad, rtol=0, atol=1e-15)


@pytest.mark.parametrize('hw', [(6, 9), (13, 19)])
@pytest.mark.parametrize('k', [5, 9])
def test_lowpass_is_padded_cross_correlation(k, hw):
    from oracle.nets import gaussian_kernel2d
    g = gen(21)
    H, W = hw
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    for w in (nonsym(k, g), gaussian_kernel2d(k).double()):
        low, mag = R.lowpass(x, w)
        want = F.conv2d(x, w.view(1, 1, k, k).repeat(3, 1, 1, 1), None, 1, (k - 1) // 2, 1, 3)
        assert torch.allclose(low, want, rtol=0, atol=1e-14) and bool((mag >= low.abs() - 1e-14).all())
        # a transposed or flipped kernel is a different operator: the non-symmetric w tells them apart
        if not torch.equal(w, w.t()):
            for other in (w.t(), w.flip(0), w.flip(1), w.flip(0, 1)):
                assert float((R.lowpass(x, other.contiguous())[0] - low).abs().max()) > 1e-3
        for nv in (False, True):
            for a_h in (0.25, 1.0):
                gl, gh = torch.randn(x.shape, generator=g, dtype=torch.float64), torch.randn(x.shape, generator=g, dtype=torch.float64)
                lo = R.lowpass(x, w, nv)[0]
                hi = a_h * (x - lo)
                for a, b in ((gl, gh), (gl, None), (None, gh)):
                    gx, gm = R.lowpass_adj(a, b, w, a_h, nv)
                    lhs = (dot(lo, a) if a is not None else 0.0) + (dot(hi, b) if b is not None else 0.0)
                    assert same_dot(lhs, dot(x, gx)) and bool((gm >= gx.abs() - 1e-14).all())


@pytest.mark.parametrize('hw', [(6, 9), (20, 28)])
@pytest.mark.parametrize('k', [5, 17])
def test_normalised_box_is_avgpool_without_the_pad_count(k, hw):
    H, W = hw
    x = torch.randn(2, 1, H, W, generator=gen(22), dtype=torch.float64)
    w = torch.full((k, k), 1.0 / (k * k), dtype=torch.float64)
    low, mag = R.lowpass(x, w, True)
    assert torch.allclose(low, F.avg_pool2d(x, k, 1, (k - 1) // 2, count_include_pad=False), rtol=0, atol=1e-14)
    assert torch.allclose(R.lowpass(x, w, False)[0], F.avg_pool2d(x, k, 1, (k - 1) // 2, count_include_pad=True), rtol=0, atol=1e-14)
    assert torch.allclose(mag, F.avg_pool2d(x.abs(), k, 1, (k - 1) // 2, count_include_pad=False), rtol=0, atol=1e-14)
    if k == 17 and hw == (6, 9):      # the window overhangs on all four sides at once: every pixel is the mean of the whole image
        assert float(R.valid_count(H, W, k).min()) == H * W
        assert torch.allclose(low, x.mean((2, 3), keepdim=True).expand_as(x), rtol=0, atol=1e-14)
    xr = x.clone().requires_grad_(True)
    g = torch.randn(x.shape, generator=gen(23), dtype=torch.float64)
    (F.avg_pool2d(xr, k, 1, (k - 1) // 2, count_include_pad=False) * g).sum().backward()
    assert torch.allclose(R.lowpass_adj(g, None, w, 0.0, True)[0], xr.grad, rtol=0, atol=1e-14)


@pytest.mark.parametrize('hw', [(5, 6), (13, 19)])
def test_lowpass_valid_and_its_adjoint(hw):
    g = gen(24)
    H, W = hw
    k = 5
    w = nonsym(k, g)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    want = F.conv2d(x, w.view(1, 1, k, k).repeat(3, 1, 1, 1), None, 1, 0, 1, 3)
    out, mag = R.lowpass_valid(x.detach(), w)
    assert out.shape == (2, 3, H - 4, W - 4) and torch.allclose(out, want.detach(), rtol=0, atol=1e-14) and bool((mag >= out.abs() - 1e-14).all())
    gg = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (want * gg).sum().backward()
    gx, gm = R.lowpass_valid_adj(gg, w, H, W)
    assert torch.allclose(gx, x.grad, rtol=0, atol=1e-14) and bool((gm >= gx.abs() - 1e-14).all())
    assert same_dot(dot(out, gg), dot(x.detach(), gx))
    assert float((R.lowpass_valid_adj(gg, w.t().contiguous(), H, W)[0] - gx).abs().max()) > 1e-3


@pytest.mark.parametrize('arch,hw', [('nld_s1', (24, 32)), ('nld_s1', (32, 40)), ('nld_s2', (24, 32)), ('nld_s2', (32, 40)), ('FSD', (9, 12))])
def test_ddm_spread_is_the_dataset_step(arch, hw):
    from oracle import dsn_dataset as D
    H, W = hw
    n_h, n_w = D.receptive(H, D.CONVNETS[arch])[0], D.receptive(W, D.CONVNETS[arch])[0]
    d = torch.rand(2, 1, n_h, n_w, generator=gen(25), dtype=torch.float64)
    v, mag, cnt, lay = R.ddm_spread(d, H, W, D.CONVNETS[arch])
    assert torch.equal(v, torch.from_numpy(D.domain_distance_map(d.numpy(), (2, 1, H, W), 'gau', arch)))
    assert lay == (n_h,) + tuple(D.receptive(W, D.CONVNETS[arch]))
    assert bool(torch.isfinite(v).all()) and float(cnt.min()) >= 1 and bool((mag >= v.abs() - 1e-15).all())
    if arch == 'FSD':   # the equivalent form the FSD path uses: the count-normalised 17 x 17 box
        assert torch.allclose(v, R.lowpass(d, torch.full((17, 17), 1.0 / 289, dtype=torch.float64), True)[0], rtol=0, atol=1e-14)


@pytest.mark.parametrize('hw', [(1, 7), (5, 1), (5, 7), (13, 10)])
@pytest.mark.parametrize('f', [2, 3, 4])
def test_bilinear_up_matches_interpolate(f, hw):
    src = torch.randn(2, 1, *hw, generator=gen(26), dtype=torch.float64)
    v, mag = R.bilinear_up(src, f)
    assert torch.allclose(v, F.interpolate(src, scale_factor=f, mode='bilinear', align_corners=False), rtol=0, atol=1e-14)
    assert torch.allclose(mag, F.interpolate(src.abs(), scale_factor=f, mode='bilinear', align_corners=False), rtol=0, atol=1e-14)


@pytest.mark.parametrize('eps', [1e-8, 1e-3])
@pytest.mark.parametrize('mode', [0, 1])
def test_logloss_and_sigmoid_bwd_match_autograd(mode, eps):
    g = gen(27)
    x = (torch.rand(2, 1, 5, 7, generator=g, dtype=torch.float64) * 12.0 - 6.0).requires_grad_(True)
    p = torch.sigmoid(x)
    l = -torch.log(p + eps) if mode == 0 else -torch.log(1.0 - p + eps)
    l.sum().backward()
    lr, pr, gr = R.logloss(x.detach(), mode, eps)
    assert torch.allclose(lr, l.detach(), rtol=1e-14, atol=0) and torch.allclose(pr, p.detach(), rtol=1e-15, atol=0)
    assert torch.allclose(gr, x.grad, rtol=1e-13, atol=0) and bool((gr < 0).all() if mode == 0 else (gr > 0).all())
    z = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    go = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64)
    y = torch.sigmoid(z)
    (y * go).sum().backward()
    v, mag = R.sigmoid_bwd(y.detach(), go)
    assert torch.allclose(v, z.grad, rtol=1e-14, atol=1e-18) and torch.equal(mag, v.abs())
