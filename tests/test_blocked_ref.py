"""CPU checks of oracle/blocked_ref.py, the references tests/test_gpu_elementwise.py, tests/test_gpu_filters.py, tests/test_gpu_norm_gan.py and
tests/test_gpu_lpips_prelu.py trust, against stock torch: they run where no kernel can.  For the normalisation and GAN-loss references and for the
LPIPS / PReLU / crop-gather references also: on the very inputs of the GPU tests (oracle/norm_gan_cases.py, oracle/lpips_prelu_cases.py) stock fp32
arithmetic stays inside every bound and a list of deliberately wrong variants does not."""
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


# ---- the normalisation, gradient-penalty and GAN-loss references ----------------------------------------------------------------------------
from oracle import norm_gan_cases as K  # noqa: E402

SLOPE, EPS = 0.2, 1e-5


def close(got, want, rel=1e-12):
    """agreement to `rel` of the largest magnitude of the tensor"""
    got, want = (got.v if isinstance(got, R.Ev) else got), want.detach()
    return got.shape == want.shape and float((got - want).abs().max()) <= rel * max(float(want.abs().max()), 1e-300)


def _in(x):
    return F.leaky_relu(F.instance_norm(x, eps=EPS), SLOPE)


def _bn(x, group, gamma, beta):
    return torch.cat([F.leaky_relu(F.batch_norm(x[n0:n1], None, None, gamma, beta, True, 0.1, EPS), SLOPE) for n0, n1 in R.groups(x.shape[0], group)])


def _norm_plain(x, dims, gamma=None, beta=None):
    """the normalisation + LeakyReLU in elementary torch operations: F.instance_norm / F.batch_norm hand their saved statistics to their double backward
    as constants, so a derivative of THAT with respect to x (what *_second is) comes out wrong through them; through this form autograd has it all"""
    mu = x.mean(dims, keepdim=True)
    xh = (x - mu) / ((x - mu).pow(2).mean(dims, keepdim=True) + EPS).sqrt()
    return F.leaky_relu(xh if gamma is None else xh * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1), SLOPE)


def _bn_plain(x, group, gamma, beta):
    return torch.cat([_norm_plain(x[n0:n1], (0, 2, 3), gamma, beta) for n0, n1 in R.groups(x.shape[0], group)])


def _first_and_second_order(f, x, t, ga, ga2, params=()):
    """of y = f(x): (y, J^T ga, J t, d <J t, ga2> / dx, d <J t, ga2> / dparams), the tangent taken by the double-backward trick of
    tests/test_gpu_wgan.py: J t = d <J^T v, t> / dv"""
    x = x.clone().requires_grad_(True)
    y = f(x)
    gx, = torch.autograd.grad(y, x, ga, retain_graph=True)
    v = torch.zeros_like(y, requires_grad=True)
    jt_v, = torch.autograd.grad(y, x, v, create_graph=True)
    jt, = torch.autograd.grad(jt_v, v, t, create_graph=True)
    second = torch.autograd.grad((jt * ga2).sum(), (x,) + tuple(params), allow_unused=True)
    return y.detach(), gx, jt.detach(), second[0], second[1:]


@pytest.mark.parametrize('hw', [(1, 3), (7, 10)])
def test_instance_norm_references_match_autograd(hw):
    g = gen(40)
    x = torch.randn(3, 5, *hw, generator=g, dtype=torch.float64) * 1.5 + 0.3
    t, ga, ga2, out0 = (torch.randn(x.shape, generator=g, dtype=torch.float64) for _ in range(4))
    y, gx, jt, _, _ = _first_and_second_order(_in, x, t, ga, ga2)
    y2, gx2, jt2, sec, _ = _first_and_second_order(lambda v: _norm_plain(v, (2, 3)), x, t, ga, ga2)
    assert close(y2, y) and close(gx2, gx) and close(jt2, jt)
    yr, mean, rstd = R.inorm_lrelu_fwd(x, EPS, SLOPE)
    assert close(yr, y) and close(mean, x.mean((2, 3), keepdim=True)) and close(rstd, 1.0 / (x.var((2, 3), unbiased=False, keepdim=True) + EPS).sqrt())
    # the backward-type references read the saved output and rstd
    assert close(R.inorm_lrelu_bwd(y, ga, rstd.v, SLOPE), gx)
    assert close(R.inorm_lrelu_jvp(y, t, rstd.v, SLOPE), jt)
    assert close(R.inorm_second(y, t, ga2, rstd.v, SLOPE), sec) and close(R.inorm_second(y, t, ga2, rstd.v, SLOPE, out0), sec + out0)
    # the forward-mode tangent, directly
    import torch.autograd.forward_ad as fwad
    with fwad.dual_level():
        assert close(R.inorm_lrelu_jvp(y, t, rstd.v, SLOPE), fwad.unpack_dual(_in(fwad.make_dual(x, t))).tangent)
    # at a == +0 and -0: xhat = 0 and LeakyReLU' = slope, as autograd has it for leaky_relu at 0
    a0 = y.clone()
    a0[0, 0, 0, 0], a0[1, 1, 0, 1] = 0.0, -0.0
    lone = torch.zeros_like(ga)
    lone[0, 0, 0, 0], lone[1, 1, 0, 1] = 1.0, 1.0
    jv = R.inorm_lrelu_jvp(a0, lone, rstd.v, SLOPE).v
    cnt = hw[0] * hw[1]
    for idx in ((0, 0, 0, 0), (1, 1, 0, 1)):
        assert abs(float(jv[idx]) - SLOPE * float(rstd.v[idx[0], idx[1], 0, 0]) * (1.0 - 1.0 / cnt)) <= 1e-12 * float(rstd.v.max())


@pytest.mark.parametrize('ng', [(4, 2), (3, 2), (3, 3), (2, 1)])
def test_batch_norm_references_match_autograd(ng):
    N, group = ng
    g = gen(41)
    C = 5
    x = torch.randn(N, C, 7, 10, generator=g, dtype=torch.float64) * 1.5 + 0.3
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) * torch.tensor([1.0, -1.0, 1.0, 1.0, -1.0], dtype=torch.float64)
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    t, ga, ga2, out0 = (torch.randn(x.shape, generator=g, dtype=torch.float64) for _ in range(4))
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y, gx, jt, _, _ = _first_and_second_order(lambda v: _bn(v, group, gm, bt), x, t, ga, ga2, (gm, bt))
    y2, gx2, jt2, sec, (sec_g, sec_b) = _first_and_second_order(lambda v: _bn_plain(v, group, gm, bt), x, t, ga, ga2, (gm, bt))
    assert close(y2, y) and close(gx2, gx) and close(jt2, jt)
    yr, z, mean, rstd, var = R.bnorm_lrelu_fwd(x, group, EPS, SLOPE, gamma, beta)
    G = len(R.groups(N, group))
    assert close(yr, y) and mean.v.shape == (G, C) and G == -(-N // group)
    for gi, (n0, n1) in enumerate(R.groups(N, group)):
        assert close(mean.v[gi], x[n0:n1].mean((0, 2, 3))) and close(var.v[gi], x[n0:n1].var((0, 2, 3), unbiased=False))
        assert close(rstd.v[gi], 1.0 / (x[n0:n1].var((0, 2, 3), unbiased=False) + EPS).sqrt())
    xr = x.clone().requires_grad_(True)
    _bn(xr, group, gm, bt).backward(ga)
    gxr, dg, db, _ = R.bnorm_lrelu_bwd(x, ga, group, SLOPE, gamma, beta, mean.v, rstd.v, 0.37)
    assert close(gxr, gx) and close(dg, 0.37 * gm.grad) and close(db, 0.37 * bt.grad)
    assert close(R.bnorm_lrelu_jvp(x, t, group, SLOPE, gamma, beta, mean.v, rstd.v)[0], jt)
    out, dg2, _ = R.bnorm_second(x, t, ga2, group, SLOPE, gamma, beta, mean.v, rstd.v, None, None, 0.37)
    assert close(out, sec) and close(dg2, 0.37 * sec_g) and (sec_b is None or float(sec_b.abs().max()) == 0.0)     # beta has no term
    d0 = torch.randn(C, generator=g, dtype=torch.float64)
    out, dg2, _ = R.bnorm_second(x, t, ga2, group, SLOPE, gamma, beta, mean.v, rstd.v, out0, d0, 0.37)
    assert close(out, sec + out0) and close(dg2, d0 + 0.37 * sec_g)


@pytest.mark.parametrize('n_hw', [(2, 5, 7), (1, 1, 1)])
def test_running_statistics_are_batchnorm2d_state(n_hw):
    N, H, W = n_hw
    g = gen(42)
    C = 5
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=0.1).double()
    bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64))
    bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    if N * H * W > 1:
        bn.train()(x)
        rm, rv = R.bnorm_running(x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False), N * H * W, 0.1, rm0, rv0)
        assert close(rm, bn.running_mean, 1e-12) and close(rv, bn.running_var, 1e-12) and int(bn.num_batches_tracked) == 1
        assert not close(R.bnorm_running(x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False), N * H * W, 0.1, rm0, rv0, 'biased')[1], bn.running_var, 1e-3)
    else:       # one element per channel (torch refuses to train on it): the correction count / (count - 1) is left out, the variance 0 enters as it is
        rm, rv = R.bnorm_running(x.mean((0, 2, 3)), torch.zeros(C), 1, 0.1, rm0, rv0)
        assert close(rm, 0.9 * rm0 + 0.1 * x.view(C)) and close(rv, 0.9 * rv0)


@pytest.mark.parametrize('target', [1.0, 0.0, 0.9])
def test_gan_loss_types_match_torch(target):
    x = (torch.randn(2, 3, 5, 7, generator=gen(43), dtype=torch.float64) * 3.0).requires_grad_(True)
    tt = torch.full_like(x, target)
    for gan_type, lossf in ((0, lambda: F.binary_cross_entropy_with_logits(x, tt, reduction='none')), (1, lambda: F.mse_loss(x, tt, reduction='none')),
                            (2, lambda: -x if target > 0.5 else x)):
        l = lossf()
        gr, = torch.autograd.grad(l.sum() * 0.3, x)
        lr, grr = R.gan_loss(x.detach(), gan_type, target, 0.3)
        assert close(lr, l) and close(grr, gr)
        # (torch's own mean-reduced criteria: the mean is coef = 1 / numel)
        crit = (torch.nn.BCEWithLogitsLoss(), torch.nn.MSELoss(), None)[gan_type]
        mean = crit(x, tt) if crit else (-x if target > 0.5 else x).mean()
        assert abs(float(lr.v.sum()) / x.numel() - float(mean.detach())) <= 1e-12 * abs(float(mean.detach()))


def _ragan_term_torch(z, t, eps, form):
    if form == 0:
        return F.binary_cross_entropy_with_logits(z, torch.full_like(z, t), reduction='none')
    if form == 2:
        return (z - t) ** 2
    if form == 3:
        return -z if t > 0.5 else z
    if t < 0:
        return z * 0.0
    s = torch.sigmoid(z)
    return -torch.log(s + eps) if t > 0.5 else -torch.log(1.0 - s + eps)


@pytest.mark.parametrize('form,ta,tb', [(0, 1.0, 0.0), (0, 0.9, 0.0), (1, 1.0, 0.0), (1, 0.0, 1.0), (1, 0.0, -1.0), (2, 1.0, 0.0), (3, 1.0, 0.0), (3, 0.0, 1.0)])
def test_ragan_forms_match_autograd_through_the_global_means(form, ta, tb):
    """n_glob = 6 > N = 2: the remote samples enter the per-pixel means, and the LOCAL gradient of the GLOBAL loss holds their terms through the
    means (part_* / n_glob) while their own direct terms stay on their rank"""
    g = gen(44)
    eps, gcoef, NG, NL = 1e-8, 0.3, 6, 2
    a_all, b_all = (torch.randn(NG, 1, 5, 7, generator=g, dtype=torch.float64) * 3.0 for _ in range(2))
    a, b = a_all[:NL].clone().requires_grad_(True), b_all[:NL].clone().requires_grad_(True)
    aa, bb = torch.cat([a, a_all[NL:]]), torch.cat([b, b_all[NL:]])
    za, zb = aa - bb.mean(0, keepdim=True), bb - aa.mean(0, keepdim=True)
    la, lb = _ragan_term_torch(za, ta, eps, form), _ragan_term_torch(zb, tb, eps, form)
    ga, gb = torch.autograd.grad((la.sum() + lb.sum()) * gcoef, (a, b))
    sums_a, sums_b = aa.detach().sum(0, keepdim=True), bb.detach().sum(0, keepdim=True)
    ad, bd = a.detach(), b.detach()
    s0a, s0b = R.ragan_sums(ad, bd)
    assert close(s0a, ad.sum(0, keepdim=True)) and close(s0b, bd.sum(0, keepdim=True))
    (lar, da, sa), (lbr, db, sb) = R.ragan_terms(ad, bd, sums_a, sums_b, NG, form, ta, tb, eps)
    assert close(lar, la[:NL]) and close(lbr, lb[:NL]) and close(sa, torch.sigmoid(za[:NL])) and close(sb, torch.sigmoid(zb[:NL]))
    (_, rda, _), (_, rdb, _) = R.ragan_terms(a_all[NL:], b_all[NL:], sums_a, sums_b, NG, form, ta, tb, eps)
    part_a, part_b = da.v.sum(0, keepdim=True) + rda.v.sum(0, keepdim=True), db.v.sum(0, keepdim=True) + rdb.v.sum(0, keepdim=True)
    gar, gbr = R.ragan_grads(da, db, part_a, part_b, NG, gcoef)
    assert close(gar, ga) and close(gbr, gb)
    if not (form == 1 and tb < 0):        # without the remote samples' share of part_b the gradient is another one
        assert not close(R.ragan_grads(da, db, da.v.sum(0, keepdim=True), db.v.sum(0, keepdim=True), NG, gcoef)[0], ga, 1e-6)


@pytest.mark.parametrize('world', [1, 2])
def test_grad_penalty_matches_autograd(world):
    g = gen(45)
    gr = [(torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64) * 0.05).requires_grad_(True) for _ in range(world)]
    # the gradient of the GLOBAL mean output restricted to a rank's samples is g_r / world
    nrm = torch.cat([t.reshape(-1) for t in gr]).div(world).norm()
    pen = 10.0 * (nrm - 1.0) ** 2
    dg, = torch.autograd.grad(pen, gr[0])
    s = sum(float(R.grad_penalty_sumsq(t.detach()).v) for t in gr)
    assert close(R.grad_penalty_sumsq(gr[0].detach()), (gr[0].detach() ** 2).sum())
    nr, pr, fac = R.grad_penalty_finish(s, 10.0, world)
    assert close(nr, nrm) and close(pr, pen)
    # d pen / d g_0 = fac * g_0 / world: the factor in front of this rank's gradient, its other 1 / world carried by the weight-gradient reductions
    assert close(float(fac.v) * gr[0].detach() / world, dg)
    z = R.grad_penalty_finish(0.0, 10.0, world)
    assert float(z[0].v) == 0.0 and float(z[1].v) == 10.0 and float(z[2].v) == 0.0 and float(z[2].e) == 0.0


# ---- the bounds on the inputs of tests/test_gpu_norm_gan.py: sound (stock fp32 arithmetic meets them) and with teeth (wrong variants do not) --------
EVALS = list(K.evals())
WRONG = ['mean_count-1', 'unbiased', 'no_eps', 'other_row', 'ragged_drop', 'lrelu1_at0', 'factor2', 'dgamma_first', 'biased', 'means_N', 'swap_part',
         'wgan_sign', 'no_world2']


def _worst(got, ref):
    """largest |got - ref| / bound over the outputs; nan counts as outside"""
    worst = 0.0
    for k, r in ref.items():
        q = (got[k].v.double() - r.v).abs() / r.tol()
        worst = max(worst, float('inf') if bool(torch.isnan(q).any()) else float(q.max()))
    return worst


@pytest.mark.parametrize('case', EVALS, ids=[e[0] for e in EVALS])
def test_bounds_are_sound_and_have_teeth(case):
    _, fn, args, wrong = case
    inputs, ref = fn(*args)
    for r in ref.values():
        assert bool(torch.isfinite(r.v).all()) and bool(torch.isfinite(r.e).all()) and bool((r.e >= 0).all())
    with R.fp32_arithmetic():
        inputs32, got = fn(*args)
    assert all(torch.equal(inputs[k], inputs32[k]) for k in inputs if torch.is_tensor(inputs[k]))      # the same inputs
    assert all(g.v.dtype == torch.float32 for g in got.values())
    assert _worst(got, ref) <= 1.0, _worst(got, ref)
    if 'z_margin' in inputs:              # no recomputed z near its LeakyReLU branch (see norm_gan_cases.bn_saved)
        assert inputs['z_margin'] > 1.0
    for w in wrong:
        assert w in WRONG
        assert _worst(fn(*args, wrong=w)[1], ref) > 1.0, w


def test_every_wrong_variant_is_exercised():
    assert {w for e in EVALS for w in e[3]} == set(WRONG)


@pytest.mark.parametrize('hw', K.NORM_HW)
@pytest.mark.parametrize('C', K.NORM_C)
def test_stock_forward_norms_meet_the_bounds(C, hw):
    """F.instance_norm / F.batch_norm + F.leaky_relu in fp32 (torch's own order of summation) on the GPU tests' forward inputs"""
    x = K.in_fwd(C, *hw)
    y, mean, rstd = R.inorm_lrelu_fwd(x, K.EPS, K.SLOPE)
    got = F.leaky_relu(F.instance_norm(x, eps=K.EPS), K.SLOPE)
    assert bool(((got.double() - y.v).abs() <= y.tol()).all())
    assert bool(torch.isfinite(y.v[:, K.CONST]).all()) and bool((y.v[:, K.CONST] == 0).all())          # the constant channel: exactly zero, finite bound
    # ... whose bound is rstd * (the bound of the mean), up to the roundings of the difference and the product
    assert bool((y.tol()[:, K.CONST] <= 1.01 * (rstd.v * mean.tol())[:, K.CONST] + R.TINY32).all())
    for N, group in K.BN_NG:
        i = K.bn_fwd(N, group, C, *hw)
        yb = R.bnorm_lrelu_fwd(i['x'], group, K.EPS, K.SLOPE, i['gamma'], i['beta'])[0]
        got = _bn(i['x'], group, i['gamma'], i['beta'])
        assert bool(((got.double() - yb.v).abs() <= yb.tol()).all())


@pytest.mark.parametrize('hw', K.PIX_HW)
@pytest.mark.parametrize('gan_type', [0, 1])
def test_accumulator_bound_holds_for_an_fp32_sum(gan_type, hw):
    """coef * (fp32 sum of the fp32 terms) + acc0, all in stock fp32, inside the bound the GPU tests put on the loss accumulators"""
    for C in K.PIX_C:
        i, ref = K.ref_gan_loss(gan_type, 1.0, C, *hw)
        coef = K.gan_coefs(C, *hw)[0]
        with R.fp32_arithmetic():
            l32 = K.ref_gan_loss(gan_type, 1.0, C, *hw)[1]['l'].v
        got = torch.tensor(0.25) + torch.tensor(coef) * l32.sum()
        want, bound = R.acc_sum(ref['l'], coef, 0.25, C, (K.PIX_N * hw[0] * hw[1] + 255) // 256)
        assert abs(float(got) - want) <= bound and bound < 1e-5 * abs(want)


def test_every_accumulator_bound_is_tight():
    """every (value, bound) the GPU file applies to a loss / score accumulator: the bound stays below 2e-5 of coef sum |terms| + |acc0|, the scale the
    grid-sum convention L u32 (coef sum |terms| + |acc0|) is relative to (L <= 24 here: 1.5e-6; the rest is the terms' own bounds, largest for the
    -log terms of ragan form 1).  A bound of per cents -- what a saturated sigmoid under -log(1 - s + eps) would make of it -- fails here."""
    def tight(accs, scales):
        for k, (want, bound) in accs.items():
            assert bound <= 2e-5 * scales[k], (k, want, bound, scales[k])
    for C in K.PIX_C:
        for H, W in K.PIX_HW:
            coef, _, scoef = K.gan_coefs(C, H, W)
            for gt in (0, 1, 2):
                for t in K.TARGETS:
                    i, ref = K.ref_gan_loss(gt, t, C, H, W)
                    tight(K.gan_accs(gt, t, C, H, W), dict(loss=coef * float(ref['l'].v.abs().sum()) + abs(K.ACC0['loss']),
                                                           score=scoef * float(i['x'].double().abs().sum()) + abs(K.ACC0['score'])))
    for H, W in K.RAGAN_HW:
        coef, _, scoef = K.gan_coefs(1, H, W)
        for form, ts in K.RAGAN_T.items():
            for ta, tb in ts:
                i, ref = K.ref_ragan(form, ta, tb, H, W)
                tight(K.ragan_accs(form, ta, tb, H, W), dict(loss=coef * float(ref['la'].v.abs().sum() + ref['lb'].v.abs().sum()) + abs(K.ACC0['loss']),
                                                             score_a=scoef * float(ref['score_a'].v.abs().sum()) + abs(K.ACC0['score']),
                                                             score_b=scoef * float(ref['score_b'].v.abs().sum()) + abs(K.ACC0['score_b'])))
                # the gradients' bounds, too, stay first-order small against the largest gradient
                for k in ('ga', 'gb'):
                    assert float(ref[k].tol().max()) <= 1e-4 * float(ref[k].v.abs().max()) + R.TINY32, (form, ta, tb, k)


# ---- LPIPS layers, PReLU slope gradient, crop gather: the references of tests/test_gpu_lpips_prelu.py against stock torch in fp64 -------------------
from oracle import lpips_prelu_cases as K2  # noqa: E402


def _s2d_torch(t, scale, shift):
    """ScalingLayer, zero padding by 2, 4x4 space-to-depth, on an NCHW fp64 image"""
    N, _, H, W = t.shape
    s = t * torch.tensor(scale[:3], dtype=torch.float64).view(1, 3, 1, 1) + torch.tensor(shift[:3], dtype=torch.float64).view(1, 3, 1, 1)
    Hs, Ws = (H + 4) // 4, (W + 4) // 4
    return F.pad(s, (2, 2, 2, 2)).view(N, 3, Hs, 4, Ws, 4).permute(0, 1, 3, 5, 2, 4).reshape(N, 48, Hs, Ws)


DRAWS = [(k, r, c) for k in range(4) for r, c in ((0, 0), (1, 0), (0, 1))]      # the draws of PerceptualLoss.forward: a rotation, then at most one flip


@pytest.mark.parametrize('k_rot,rows,cols', DRAWS + [(1, 1, 1), (2, 1, 1)])
def test_lpips_s2d_symmetry_codes_are_rot90_and_flip(k_rot, rows, cols):
    from dasr_amd.dsn_model import symmetry_code
    code = symmetry_code(k_rot, rows, cols)
    for H, W in ((12, 12), (8, 12)):
        if code & 1 and H != W:
            continue
        i = K2.s2d_inputs(H, W)
        x = i['x'].double().requires_grad_(True)
        t = torch.rot90(x, k_rot, [2, 3])
        t = torch.flip(t, (2,)) if rows else t
        t = torch.flip(t, (3,)) if cols else t
        y = _s2d_torch(t, K2.SCALE4, K2.SHIFT4)
        ref = R.lpips_s2d(i['x'], K2.SCALE4, K2.SHIFT4, code)
        assert close(ref, y, 1e-15)
        border = torch.ones(H + 4, W + 4, dtype=torch.bool)
        border[2:-2, 2:-2] = False
        unblocked = ref.v.view(2, 3, 4, 4, (H + 4) // 4, (W + 4) // 4).permute(0, 1, 4, 2, 5, 3).reshape(2, 3, H + 4, W + 4)
        ebound = ref.e.view(2, 3, 4, 4, (H + 4) // 4, (W + 4) // 4).permute(0, 1, 4, 2, 5, 3).reshape(2, 3, H + 4, W + 4)
        # the padding: exact zero with a zero bound; inside the image the bound is the two roundings' worth, never zero (shift is not)
        assert bool((unblocked[:, :, border] == 0).all()) and bool((ebound[:, :, border] == 0).all()) and bool((ebound[:, :, ~border] > 0).all())
        # the adjoint is the transpose of the linear part: autograd's gradient of <y, gy>, added to what x0 holds
        gx, = torch.autograd.grad((y * i['gy'].double()).sum(), x)
        assert close(R.lpips_s2d_adj(i['gy'], i['x0'], K2.SCALE4, code), i['x0'].double() + gx, 1e-15)
        # <s2d_T(x) - shift part, gy> == <x, adj_T(gy)>
        lin = R.lpips_s2d(i['x'], K2.SCALE4, [0.0] * 4, code).v
        adj = R.lpips_s2d_adj(i['gy'], torch.zeros_like(i['x0']), K2.SCALE4, code).v
        lhs, rhs = float((lin * i['gy'].double()).sum()), float((i['x'].double() * adj).sum())
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_dihedral_codes_cover_the_square_and_only_quarter_turns_are_not_involutions():
    x = torch.arange(144.0).view(1, 1, 12, 12)
    seen = set()
    for xf in range(8):
        U, V = R.dihedral_map(12, 12, xf)
        t = x[:, :, U, V]
        seen.add(tuple(t.flatten().tolist()))
        assert torch.equal(t[:, :, U, V], x) == (xf not in K2.QUARTER_TURNS)
    assert len(seen) == 8


@pytest.mark.parametrize('hw', K2.POOL_HW + [(15, 18)])
def test_maxpool3s2_matches_torch(hw):
    """F.max_pool2d(3, 2) and autograd on tied inputs (ATen, too, hands the gradient to the first maximum in scan order); relu_mask: the gradient
    w.r.t. the pre-activation z of x = relu(z)"""
    g = gen(60)
    z = tied((2, 5, hw[0], hw[1]), g)
    gy = torch.randn(2, 5, (hw[0] - 3) // 2 + 1, (hw[1] - 3) // 2 + 1, generator=g, dtype=torch.float64)
    gx0 = torch.randn(2, 5, hw[0], hw[1], generator=g, dtype=torch.float64)
    for relu in (0, 1):
        zz = z.clone().requires_grad_(True)
        x = torch.relu(zz) if relu else zz
        y = F.max_pool2d(x, 3, 2)
        assert torch.equal(R.maxpool3s2(x.detach())[0], y.detach())
        want, = torch.autograd.grad((y * gy).sum(), zz)
        assert close(R.maxpool3s2_bwd(x.detach(), gy, relu), want, 1e-15)
        assert close(R.maxpool3s2_bwd(x.detach(), gy, relu, gx0), want + gx0, 1e-15)
        if hw != (3, 3):
            assert not close(R.maxpool3s2_bwd(x.detach(), gy, relu, wrong='last_max'), want, 1e-3)


@pytest.mark.parametrize('C', K2.POOL_C)
@pytest.mark.parametrize('hw', K2.POOL_HW)
def test_pool_inputs_hold_the_cases_the_gpu_test_is_about(hw, C):
    i = K2.pool_inputs(C, *hw)
    x = i['x'].double()
    m, am = R._first_max(x, 3, 2)
    Ho, Wo = am.shape[2:]
    cand = torch.stack(R._windows(x, Ho, Wo, 3, 2), -1)
    tied_pos = ((cand == m.unsqueeze(-1)).sum(-1) > 1) & (m > 0)
    assert bool(tied_pos[:, :C].any())                                   # tied maxima at non-zero values
    assert bool((m[:, 0, 0, 0] == 0).all()) and bool((m[:, 1, 0, 0] < 0).all())      # a window all zero, a window all negative
    assert float(x.min()) > -3.4e38 and bool(torch.isfinite(x).all())
    if Ho * Wo > 1:
        # a pixel that is the first maximum of one of its windows and not of another: its gradient is ONE of the window gradients, not their sum
        first = torch.zeros(x.shape, dtype=torch.long)
        member = torch.zeros(x.shape, dtype=torch.long)
        for d in range(9):
            dy, dx = d // 3, d % 3
            first[:, :, dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2] += (am == d).long()
            member[:, :, dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2] += 1
        assert bool(((first >= 1) & (first < member))[:, :C].any()) and bool((first >= 2)[:, :C].any())
    if hw in ((4, 4), (8, 6)):                                           # the last row and column lie in no window: exact zero, zero bound
        gx = R.maxpool3s2_bwd(i['x'], i['gy'], 0)
        assert bool((gx.v[:, :, -1] == 0).all()) and bool((gx.v[:, :, :, -1] == 0).all()) and bool((gx.e[:, :, -1] == 0).all())


def _normalize(t, eps):
    return t / (torch.sqrt((t ** 2).sum(1, keepdim=True)) + eps)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('C', [16, 48])
def test_lpips_head_matches_autograd_through_normalize_tensor(C, relu):
    g = gen(61)
    z = torch.randn(4, C, 5, 7, generator=g, dtype=torch.float64)
    lin = torch.rand(C, generator=g, dtype=torch.float64)
    zz = z.clone().requires_grad_(True)
    f = torch.relu(zz) if relu else zz
    d = _normalize(f[:2], 1e-10) - _normalize(f[2:], 1e-10)
    val = ((d ** 2) * lin.view(1, C, 1, 1)).sum(1, keepdim=True)
    want, = torch.autograd.grad(0.3 * val.sum(), zz)
    rv, rg = R.lpips_head(f[:2].detach(), f[2:].detach(), lin, 1e-10, 0.3, relu)
    assert close(rv, val, 1e-12) and close(rg, want[:2], 1e-9)
    for w in ('no_x0k2', 'eps_in_sqrt'):
        assert not close(R.lpips_head(f[:2].detach(), f[2:].detach(), lin, 1e-2, 0.3, relu, w)[1],
                         R.lpips_head(f[:2].detach(), f[2:].detach(), lin, 1e-2, 0.3, relu)[1].v, 1e-3)


@pytest.mark.parametrize('C', K2.HEAD_C)
def test_lpips_head_contract_at_all_zero_pixels(C):
    """f0 all zero: u = 0, the derivative of the norm is taken as 0 (k2 = 0), so g0 = gcoef 2 w (0 - v) / eps: large, finite, zero bound only where v
    is zero too"""
    i, ref = K2.ref_head(C, 0)
    gc = K2.head_coefs()[1]
    n, y, x = K2.PIX_F0_ZERO
    v = _normalize(i['f'][K2.PAIR_OFF:K2.PAIR_OFF + 2].double(), K2.HEAD_EPS)[n, :, y, x]
    want = gc * 2.0 * i['lin'].double() * (0.0 - v) / K2.HEAD_EPS
    assert bool(torch.isfinite(ref['g0'].v).all()) and close(ref['g0'].v[n, :, y, x], want, 1e-12)
    assert abs(float(ref['val'].v[n, 0, y, x]) - float((i['lin'].double() * v * v).sum())) <= 1e-12
    n, y, x = K2.PIX_BOTH_ZERO
    assert bool((ref['g0'].v[n, :, y, x] == 0).all()) and float(ref['val'].v[n, 0, y, x]) == 0.0 and float(ref['val'].e[n, 0, y, x]) == 0.0
    n, y, x = K2.PIX_TINY            # eps is visible here and nowhere else: r0 is a few 1e-9
    r0 = float(i['f'][n, :, y, x].double().norm())
    assert K2.HEAD_EPS / r0 > 1e-3


def test_lpips_head_accumulator_bound_is_sound_and_tight():
    for C in K2.HEAD_C:
        _, ref = K2.ref_head(C, 0)
        with R.fp32_arithmetic():
            v32 = K2.ref_head(C, 0)[1]['val'].v
        coef = K2.head_coefs()[0]
        got = torch.tensor(K2.HEAD_ACC0) + torch.tensor(coef) * v32.sum()
        want, bound = K2.head_acc(C)
        assert abs(float(got) - want) <= bound and bound <= 2e-5 * (coef * float(ref['val'].v.abs().sum()) + K2.HEAD_ACC0)


def test_prelu_slope_gradient_matches_autograd():
    g = gen(62)
    x = torch.randn(2, 20, 5, 7, generator=g, dtype=torch.float64)
    x[0, 0, 0, 0], x[1, 3, 2, 2] = 0.0, -0.0
    w = torch.randn(2, 20, 5, 7, generator=g, dtype=torch.float64)
    a = torch.tensor([0.2], dtype=torch.float64, requires_grad=True)
    xx = x.clone().requires_grad_(True)
    y = F.prelu(xx, a)
    da, gx = torch.autograd.grad((y * w).sum(), (a, xx))
    ref = R.prelu_grad(y.detach(), gx, 0.2, 0.5)
    assert abs(float(ref.v) - 0.5 * float(da)) <= 1e-12 * float((w * x).abs().sum())
    assert abs(float(ref.v) - 0.5 * float((gx * y.detach())[y.detach() <= 0].sum()) / 0.04) <= 1e-12 * float((w * x).abs().sum())
    part = torch.randn(3, 300, generator=g)
    fin = R.prelu_final(part, K2.FINAL_SLOPES, 0.5)
    for k, s in enumerate(K2.FINAL_SLOPES):
        assert abs(float(fin.v[k]) - 0.5 * float(part[k].double().sum()) / R.f32(s) ** 2) <= 1e-12 * float(part[k].abs().sum()) / s ** 2


@pytest.mark.parametrize('case', K2.PRELU)
@pytest.mark.parametrize('kind', ['f32', 'f16'])
def test_prelu_slope_gradient_is_indifferent_to_the_branch_at_zero(kind, case):
    """at y == +0 and -0 the term gx * y is an exact zero: `y < 0` in place of `y <= 0` is the same function of finite inputs, value and bound alike.
    include/dasr_hip.h documents the entry points as indifferent to it; no test can tell the two apart."""
    i, ref = K2.ref_prelu(*case, kind)
    assert bool((i['y'].double() == 0).any()) and bool((i['gx'].double()[i['y'].double() == 0] != 0).any())
    other = K2.ref_prelu(*case, kind, wrong='y_lt')[1]['d']
    assert torch.equal(other.v, ref['d'].v) and torch.equal(other.e, ref['d'].e)
    # the bound is relative to sum |terms|, and stays small against it
    terms = (i['gx'].double() * i['y'].double())[i['y'].double() <= 0]
    scale = K2.PRELU_SCALE / (K2.PRESCALE if kind == 'f16' else 1.0)
    assert float(ref['d'].tol()) <= 30 * R.U32 * scale * float(terms.abs().sum()) / K2.PRELU_A ** 2


def _crop_cv2(D, C, size):
    """the forward statement: cv2.resize(INTER_LINEAR) of the whole image to vH x vW (half-pixel centres, edge clamp), the window (zero outside the
    view), then hflip, vflip, transpose in that order, zero channels up to C"""
    img = D['img'].double()
    c, H, W = img.shape
    vH, vW = D['vH'], D['vW']
    if (vH, vW) == (H, W):
        view = img
    else:
        view = torch.zeros(c, vH, vW, dtype=torch.float64)
        for vy in range(vH):
            fy = (vy + 0.5) * H / vH - 0.5
            ya = int(torch.floor(torch.tensor(fy)))
            wy = fy - ya
            ya, yb = min(max(ya, 0), H - 1), min(max(ya + 1, 0), H - 1)
            for vx in range(vW):
                fx = (vx + 0.5) * W / vW - 0.5
                xa = int(torch.floor(torch.tensor(fx)))
                wx = fx - xa
                xa, xb = min(max(xa, 0), W - 1), min(max(xa + 1, 0), W - 1)
                view[:, vy, vx] = (1 - wy) * ((1 - wx) * img[:, ya, xa] + wx * img[:, ya, xb]) + wy * ((1 - wx) * img[:, yb, xa] + wx * img[:, yb, xb])
    win = torch.zeros(C, size, size, dtype=torch.float64)
    for y in range(size):
        for x in range(size):
            vy, vx = D['y0'] + y, D['x0'] + x
            if 0 <= vy < vH and 0 <= vx < vW:
                win[:min(c, C), y, x] = view[:min(c, C), vy, vx]
    if D['flags'] & 1:
        win = torch.flip(win, (2,))
    if D['flags'] & 2:
        win = torch.flip(win, (1,))
    if D['flags'] & 4:
        win = win.transpose(1, 2)
    return win


@pytest.mark.parametrize('launch', ['all', 'edge'])
def test_gather_crops_matches_the_cv2_convention(launch):
    i, ref = K2.ref_gather(launch)
    want = torch.stack([_crop_cv2(D, K2.CROP_C, K2.CROP_SIZE) for D in i['descs']])
    assert close(ref['dst'], want, 1e-14)
    assert sorted(D['flags'] for D in K2.crop_descs('all')) == list(range(8))
    # pure crops and the zero fill: exact, zero bound; the resized samples: six roundings of a blend of values in [0, 1] and, per axis, a coordinate
    # below 33 known to three roundings and one of the weight, times a slope of at most 1
    assert bool((ref['dst'].e[i['exact']] == 0).all()) and bool((ref['dst'].e[~i['exact']] > 0).all())
    assert float(ref['dst'].tol().max()) <= (6 + 2 * (3 * 33 + 1)) * R.U32
    if launch == 'all':
        assert bool((ref['dst'].v[1, 1:] == 0).all()) and bool((ref['dst'].v[1, 0] != 0).all())       # channels >= D.C: zero
    else:                                 # part of each window lies outside the view: zero there, the image elsewhere
        for k, D in enumerate(i['descs']):
            out = torch.zeros(K2.CROP_SIZE, K2.CROP_SIZE, dtype=torch.bool)      # the out-of-view mask, from the forward statement: window, flips, transpose
            for y in range(K2.CROP_SIZE):
                for x in range(K2.CROP_SIZE):
                    out[y, x] = not (0 <= D['y0'] + y < D['vH'] and 0 <= D['x0'] + x < D['vW'])
            out = torch.flip(out, (1,)) if D['flags'] & 1 else out
            out = torch.flip(out, (0,)) if D['flags'] & 2 else out
            out = out.t() if D['flags'] & 4 else out
            assert 12 <= int(out.sum()) <= 40 and torch.equal(ref['dst'].v[k, 0] == 0, out)


def test_gather_crops_floorf_across_an_integer_stays_inside_the_bound():
    """22 -> 10 puts the source coordinate of every fifth row ON an integer: the case where fp32 may floor to either side.  Taking the lower cell with a
    weight just below 1 there (what a coordinate rounded downwards gives) moves the fp32 result by less than the bound allows: the interpolant is
    continuous across the cell boundary"""
    hits = [vy for vy in range(10) if ((2 * vy + 1) * 22 - 10) % 20 == 0]
    assert hits == [2, 7]
    _, ref = K2.ref_gather('all')
    with R.fp32_arithmetic():
        plain = K2.ref_gather('all')[1]['dst'].v.double()
        below = K2.ref_gather('all', wrong='floor_below')[1]['dst'].v.double()
    assert not torch.equal(plain, below)
    assert bool(((plain - ref['dst'].v).abs() <= ref['dst'].tol()).all()) and bool(((below - ref['dst'].v).abs() <= ref['dst'].tol()).all())


EVALS2 = list(K2.evals())


@pytest.mark.parametrize('case', EVALS2, ids=[e[0] for e in EVALS2])
def test_lpips_prelu_gather_bounds_are_sound_and_have_teeth(case):
    """on the inputs of tests/test_gpu_lpips_prelu.py: the kernel's expression in stock fp32 meets every bound the GPU file applies, every listed wrong
    variant misses at least one"""
    _, fn, args, wrong = case
    inputs, ref = fn(*args)
    for r in ref.values():
        assert bool(torch.isfinite(r.v).all()) and bool(torch.isfinite(r.e).all()) and bool((r.e >= 0).all())
    with R.fp32_arithmetic():
        inputs32, got = fn(*args)
    assert all(torch.equal(inputs[k], inputs32[k]) for k in inputs if torch.is_tensor(inputs[k]))
    assert all(g.v.dtype == torch.float32 for g in got.values())
    assert _worst(got, ref) <= 1.0, _worst(got, ref)
    for w in wrong:
        assert w in K2.WRONG
        assert _worst(fn(*args, wrong=w)[1], ref) > 1.0, w


def test_every_wrong_variant_of_the_lpips_prelu_gather_cases_is_exercised():
    assert {w for e in EVALS2 for w in e[3]} == set(K2.WRONG)
