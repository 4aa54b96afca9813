"""Plain torch-CPU references of the small kernels of csrc/misc.hip / csrc/gan.hip / csrc/lpips.hip (elementwise, pooling, pixel losses, Adam; the
frequency-split, domain-distance-map and DSN loss kernels; the normalisation, gradient-penalty and GAN-loss kernels; the LPIPS layers, the PReLU
slope gradient and the fp32 crop gather), and the NC16HW16 layout plumbing the GPU tests need.  No device code: tests/test_blocked_ref.py holds every
function here to stock torch on a machine without a GPU; tests/test_gpu_elementwise.py, tests/test_gpu_filters.py, tests/test_gpu_norm_gan.py and
tests/test_gpu_lpips_prelu.py then hold the kernels to these.

Every reference computes in fp64 on NCHW tensors and returns (value, magnitude): `magnitude` is the per-element sum of the absolute values of the
terms the kernel adds up, the quantity a rounding-error bound k * u * magnitude is relative to.  Scalars (a, b, slope, coef, ...) are taken as given:
callers pass the fp32 value the kernel receives (f32())."""
import struct

import numpy as np
import torch

U32 = 2.0 ** -24                          # unit roundoff of fp32
U16 = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}
TINY16 = {'f16': 2.0 ** -25, 'bf16': 0.0}   # half the spacing of f16's subnormals (bf16 shares fp32's exponent range: not reached here)
DTYPE = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}


def f32(v):
    """the fp32 value a float argument has behind the C ABI"""
    return struct.unpack('<f', struct.pack('<f', v))[0]


def r16(x, kind):
    """round to nearest even to f16 / bf16 (torch's .half() / .bfloat16()), returned in that dtype"""
    return x.half() if kind == 'f16' else x.bfloat16()


def err16(v, kind):
    """bound of |round16(v) - v|: u16 |v|, or half a subnormal step"""
    return (U16[kind] * v.abs()).clamp_min(TINY16[kind])


def split16(v, kind):
    """split 16-bit form of an fp32 tensor: hi = round16(v), lo = round16(v - hi)"""
    v = v.float()
    hi = r16(v, kind)
    return hi, r16(v - hi.float(), kind)


# ---- layout: NCHW <-> NC16HW16 [N][K][H][W][16] --------------------------------------------------------------------------------------
def planes(C):
    return (C + 15) // 16


def pack(x, kind='f32', pad=0.0):
    """NCHW -> [N][K][H][W][16] of dtype `kind`; the padding channels hold `pad`"""
    N, C, H, W = x.shape
    K = planes(C)
    xp = torch.full((N, K * 16, H, W), pad, dtype=DTYPE[kind])
    xp[:, :C] = x.to(DTYPE[kind])
    return xp.view(N, K, 16, H, W).permute(0, 1, 3, 4, 2).contiguous()


def unpack(t, C=None):
    """[N][K][H][W][16] -> NCHW (the first C channels), same dtype"""
    N, K, H, W, _ = t.shape
    x = t.permute(0, 1, 4, 2, 3).reshape(N, K * 16, H, W)
    return x if C is None else x[:, :C]


def pack_split(hi, lo, pad=0.0):
    """split tensor: the K hi planes, then the K lo planes"""
    kind = 'f16' if hi.dtype == torch.float16 else 'bf16'
    return torch.cat([pack(hi, kind, pad), pack(lo, kind, pad)], dim=1)


def unpack_split(t, C=None):
    K = t.shape[1] // 2
    return unpack(t[:, :K], C), unpack(t[:, K:], C)


# ---- references ------------------------------------------------------------------------------------------------------------------------------
def lrelu_dash(mask, slope):
    """(P/Leaky)ReLU' read from the activation: 1 where mask > 0, else slope (so at +0 and -0 it is `slope`)"""
    m = mask.double()
    return torch.where(m > 0, torch.ones_like(m), torch.full_like(m, slope))


def axpby(x, a, z=None, b=0.0, mask=None, slope=0.0):
    """(a x + b z) * lrelu'(mask); magnitude (|a x| + |b z|) * |lrelu'|"""
    v, mag = a * x.double(), (a * x.double()).abs()
    if z is not None:
        v, mag = v + b * z.double(), mag + (b * z.double()).abs()
    if mask is not None:
        d = lrelu_dash(mask, slope)
        v, mag = v * d, mag * d.abs()
    return v, mag


def _quads(src):
    s = src.double()
    return [s[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]


def downsum2x(src, mask=None, slope=0.0, out_scale=1.0):
    """adjoint of nearest-x2 upsampling: out_scale * lrelu'(mask) * (sum of every 2x2 block); magnitude: the same of the absolute values"""
    q = _quads(src)
    v, mag = q[0] + q[1] + q[2] + q[3], q[0].abs() + q[1].abs() + q[2].abs() + q[3].abs()
    if mask is not None:
        d = lrelu_dash(mask, slope)
        v, mag = v * d, mag * d.abs()
    return v * out_scale, mag * abs(out_scale)


def pixel_shuffle(src):
    """nn.PixelShuffle(2): dst[c][2y+dy][2x+dx] = src[4c + 2dy + dx][y][x] (pure data movement: dtype kept)"""
    N, C4, H, W = src.shape
    return src.view(N, C4 // 4, 2, 2, H, W).permute(0, 1, 4, 2, 5, 3).reshape(N, C4 // 4, 2 * H, 2 * W)


def pixel_unshuffle(g, mask=None, slope=0.0):
    """adjoint of pixel_shuffle, times lrelu'(mask): (value fp64, magnitude)"""
    N, Cc, H2, W2 = g.shape
    v = g.view(N, Cc, H2 // 2, 2, W2 // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(N, Cc * 4, H2 // 2, W2 // 2).double()
    if mask is not None:
        v = v * lrelu_dash(mask, slope)
    return v, v.abs()


def _windows(t, Ho, Wo, k, s):
    """the k * k candidates of every window in scan order: element (dy, dx) of window (oy, ox) is t[s oy + dy][s ox + dx]"""
    def sl(d, n):
        return slice(d, d + s * (n - 1) + 1 if n > 0 else d, s)
    return [t[:, :, sl(dy, Ho), sl(dx, Wo)] for dy in range(k) for dx in range(k)]


def _first_max(x, k=2, s=2, last=False):
    """x: NCHW fp64 (rows / columns past the last window take no part).  (max, d) per k x k window of stride s (no padding), d = k dy + dx of the
    FIRST maximum in scan order (a later candidate replaces the current one only if it is strictly greater).  last: the LAST maximum instead (a
    deliberately wrong variant)"""
    Ho, Wo = (x.shape[2] - k) // s + 1, (x.shape[3] - k) // s + 1
    cand = _windows(x, Ho, Wo, k, s)
    m, am = cand[0].clone(), torch.zeros(cand[0].shape, dtype=torch.long)
    for d in range(1, k * k):
        up = cand[d] >= m if last else cand[d] > m
        m = torch.where(up, cand[d], m)
        am = torch.where(up, torch.full_like(am, d), am)
    return m, am


def _take(t, am, k=2, s=2):
    """element of the first maximum out of every window of t (any dtype: moved, not computed)"""
    cand = torch.stack(_windows(t, am.shape[2], am.shape[3], k, s), dim=-1)
    return torch.gather(cand, -1, am.unsqueeze(-1)).squeeze(-1)


def maxpool2(x, lo=None):
    """nn.MaxPool2d(2, 2).  Plain tensor: the maximum, in x's dtype.  Split tensor (x = hi, lo): the compared value is hi + lo, the (hi, lo) pair of
    the first maximum is moved unchanged.  Returns (y, y_lo or None, am)."""
    val = x.double() if lo is None else x.double() + lo.double()
    _, am = _first_max(val)
    return _take(x, am), (None if lo is None else _take(lo, am)), am


def maxpool2_bwd(x, gy, lo=None, gy_lo=None, relu_mask=False):
    """gradient of maxpool2: gy goes to the first maximum of its window, every other element of a window gets zero; relu_mask: nothing where the
    pooled maximum is <= 0.  Rows / columns an odd size leaves outside every window are returned as `untouched` (bool [H][W]) and hold zero here.
    Returns (gx, gx_lo or None, untouched)."""
    val = x.double() if lo is None else x.double() + lo.double()
    m, am = _first_max(val)
    Ho, Wo = am.shape[2], am.shape[3]
    keep = torch.ones_like(m, dtype=torch.bool) if not relu_mask else m > 0
    outs = []
    for g in (gy, gy_lo):
        if g is None:
            outs.append(None)
            continue
        gx = torch.zeros(x.shape, dtype=g.dtype)
        for d in range(4):
            gx[:, :, (d >> 1):2 * Ho:2, (d & 1):2 * Wo:2] = torch.where((am == d) & keep, g, torch.zeros_like(g))
        outs.append(gx)
    untouched = torch.ones(x.shape[2], x.shape[3], dtype=torch.bool)
    untouched[:2 * Ho, :2 * Wo] = False
    return outs[0], outs[1], untouched


def affine4(x, scale, shift, y0=None):
    """y = x * scale[c] + shift[c] (+ y0 when accumulating) per channel; magnitude |x scale| + |shift| (+ |y0|)"""
    C = x.shape[1]
    sc = torch.tensor([f32(s) for s in scale[:C]], dtype=torch.float64).view(1, C, 1, 1)
    sh = torch.tensor([f32(s) for s in shift[:C]], dtype=torch.float64).view(1, C, 1, 1)
    v, mag = x.double() * sc + sh, (x.double() * sc).abs() + sh.abs()
    if y0 is not None:
        v, mag = v + y0.double(), mag + y0.double().abs()
    return v, mag


def l1_diff(a, b, coef, gcoef, squared=False):
    """feature loss between two tensors: loss = coef * sum |a - b| (squared: (a - b)^2), ga = gcoef * sign(a - b) (squared: 2 gcoef (a - b)).
    Returns (loss, coef * sum |terms|, ga, |ga|)."""
    d = a.double() - b.double()
    t = d * d if squared else d.abs()
    ga = 2.0 * gcoef * d if squared else gcoef * torch.sign(d)
    return float(coef * t.sum()), float(abs(coef) * t.sum()), ga, ga.abs()


def l1_loss(sr, hr, coef, wm=None, squared=False):
    """pixel loss: loss = coef * sum wm |sr - hr| (squared: wm (sr - hr)^2), grad = coef wm sign(sr - hr) (squared: 2 coef wm (sr - hr)); wm is
    [N][1][H][W] or None.  Returns (loss, coef * sum |terms|, grad, |grad|)."""
    d = sr.double() - hr.double()
    w = torch.ones_like(d) if wm is None else wm.double().expand_as(d)
    t = w * d * d if squared else w * d.abs()
    g = 2.0 * coef * w * d if squared else coef * w * torch.sign(d)
    return float(coef * t.sum()), float(abs(coef) * t.abs().sum()), g, g.abs()


def sigmoid(x):
    v = 1.0 / (1.0 + torch.exp(-x.double()))
    return v, v.abs()


def add_flat(y, x):
    v = y.double() + x.double()
    return v, y.double().abs() + x.double().abs()


def adam(p, grads, lr, beta1, beta2, eps, wd):
    """torch.optim.Adam (L2 weight decay, no amsgrad) over the gradient list `grads`, one step each, from zero moments, in fp64:
        g' = g + wd p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    Returns (p, m, v, Ep, Em, Ev): the E* are first-order running error bounds, in units of the unit roundoff u, of an evaluation that rounds every
    operation of the expression above once (fused or not), the constants 1 - b1, 1 - b2, lr / (1 - b1^t), 1 / sqrt(1 - b2^t) included:
        fl(x op y) = (x op y)(1 + d), |d| <= u, so an operation adds |result| to the bound and passes its operands' bounds through its derivative."""
    p = p.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    Ep, Em, Ev = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    c1, c2 = 1.0 - beta1, 1.0 - beta2
    for t, g in enumerate(grads, 1):
        g = g.double()
        gd, Eg = g, torch.zeros_like(p)
        if wd != 0.0:
            gd = g + wd * p
            Eg = abs(wd) * Ep + (wd * p).abs() + gd.abs()                                # product, sum
        m_new = beta1 * m + c1 * gd
        Em = beta1 * Em + c1 * Eg + (beta1 * m).abs() + 2.0 * (c1 * gd).abs() + m_new.abs()    # b1 m; 1 - b1 and its product; sum
        v_new = beta2 * v + c2 * gd * gd
        Ev = beta2 * Ev + 2.0 * c2 * gd.abs() * Eg + (beta2 * v).abs() + 3.0 * c2 * gd * gd + v_new.abs()   # b2 v; 1 - b2 and two products; sum
        m, v = m_new, v_new
        ss, isb = lr / (1.0 - beta1 ** t), 1.0 / (1.0 - beta2 ** t) ** 0.5
        rt = v.sqrt()
        den = rt * isb + eps
        # sqrt passes half the relative error of v; then its own rounding, the constant, the product, the sum
        Eden = isb * Ev / (2.0 * rt).clamp_min(1e-300) + 3.0 * rt * isb + den
        q = m / den
        upd = ss * q
        Eupd = ss * (Em / den + q.abs() * Eden / den) + 3.0 * upd.abs()                   # quotient, the constant, the product
        p = p - upd
        Ep = Ep + Eupd + p.abs()
    return p, m, v, Ep, Em, Ev


# ---- frequency split: Haar DWT, depthwise low-pass ----------------------------------------------------------------------------------------
def _blocks(x):
    """the four elements [[a, b], [c, d]] of every 2x2 block"""
    s = x.double()
    return s[:, :, 0::2, 0::2], s[:, :, 0::2, 1::2], s[:, :, 1::2, 0::2], s[:, :, 1::2, 1::2]


def dwt(x, norm=0):
    """level-1 Haar analysis (oracle/nets.py::HaarDWT): LL = (a+b+c+d)/2, LH = (a+b-c-d)/2, HL = (a-b+c-d)/2, HH = (a-b-c+d)/2.
    norm bit 0: LL * 0.5, bands * 0.5 + 0.5; bit 1: the 'sum' format, hc = (LH + HL + HH) / 3 in C channels instead of [LH | HL | HH] in 3C;
    bit 2: the linear part only (no + 0.5).  Returns ((ll, magnitude), (hc, magnitude))."""
    a, b, c, d = _blocks(x)
    s = 0.5 * (0.5 if norm & 1 else 1.0)
    off = 0.5 if (norm & 1) and not (norm & 4) else 0.0
    mag = (a.abs() + b.abs() + c.abs() + d.abs()) * s
    ll = (a + b + c + d) * s
    bands = [(a + b - c - d) * s + off, (a - b + c - d) * s + off, (a - b - c + d) * s + off]
    if norm & 2:
        return (ll, mag), ((bands[0] + bands[1] + bands[2]) / 3.0, mag + off)
    return (ll, mag), (torch.cat(bands, 1), torch.cat([mag + off] * 3, 1))


def dwt_adj(gll, ghc, C, norm=0):
    """adjoint of the linear part of dwt: gx = DWT^T (gll, ghc); gll / ghc None: zero.  Returns (gx [N][C][2 H2][2 W2], magnitude)."""
    ref = gll if gll is not None else ghc
    N, _, H2, W2 = ref.shape
    zero = torch.zeros(N, C, H2, W2, dtype=torch.float64)
    l = zero if gll is None else gll.double()
    if ghc is None:
        lh = hl = hh = zero
    elif norm & 2:
        lh = hl = hh = ghc.double() / 3.0
    else:
        lh, hl, hh = ghc.double()[:, :C], ghc.double()[:, C:2 * C], ghc.double()[:, 2 * C:]
    s = 0.5 * (0.5 if norm & 1 else 1.0)
    gx, mag = torch.zeros(N, C, 2 * H2, 2 * W2, dtype=torch.float64), torch.zeros(N, C, 2 * H2, 2 * W2, dtype=torch.float64)
    for (dy, dx), (s1, s2, s3) in {(0, 0): (1, 1, 1), (0, 1): (1, -1, -1), (1, 0): (-1, 1, -1), (1, 1): (-1, -1, 1)}.items():
        gx[:, :, dy::2, dx::2] = s * (l + s1 * lh + s2 * hl + s3 * hh)
        mag[:, :, dy::2, dx::2] = s * (l.abs() + lh.abs() + hl.abs() + hh.abs())
    return gx, mag


def valid_count(H, W, k):
    """[H][W]: how many taps of the k x k window centred at (y, x) lie inside the image"""
    r = (k - 1) // 2
    ny = torch.tensor([min(y + r, H - 1) - max(y - r, 0) + 1 for y in range(H)], dtype=torch.float64)
    nx = torch.tensor([min(x + r, W - 1) - max(x - r, 0) + 1 for x in range(W)], dtype=torch.float64)
    return ny.view(H, 1) * nx.view(1, W)


def lowpass(x, w, norm_valid=False):
    """depthwise k x k cross-correlation with zero padding r = (k - 1) / 2: out[y, x] = sum w[ky, kx] * in[y + ky - r, x + kx - r];
    norm_valid: divided by the in-image fraction of the window (count / k^2; with the uniform w = 1 / k^2 this is AvgPool2d(count_include_pad=False)).
    Returns (low, sum |w * in| with the same normaliser)."""
    k = w.shape[0]
    r = (k - 1) // 2
    N, C, H, W = x.shape
    xp = torch.zeros(N, C, H + 2 * r, W + 2 * r, dtype=torch.float64)
    xp[:, :, r:r + H, r:r + W] = x.double()
    out, mag = torch.zeros(N, C, H, W, dtype=torch.float64), torch.zeros(N, C, H, W, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            t = float(w[ky, kx]) * xp[:, :, ky:ky + H, kx:kx + W]
            out, mag = out + t, mag + t.abs()
    if norm_valid:
        frac = valid_count(H, W, k) / float(k * k)
        out, mag = out / frac, mag / frac
    return out, mag


def _lowpass_t(g, w, norm_valid):
    """adjoint of lowpass for any w: every output pixel (y, x) of the forward op hands w[ky, kx] * g[y, x] (over ITS normaliser) back to the
    input pixel (y + ky - r, x + kx - r) it read"""
    k = w.shape[0]
    r = (k - 1) // 2
    N, C, H, W = g.shape
    gd = g.double()
    if norm_valid:
        gd = gd / (valid_count(H, W, k) / float(k * k))
    gp, mp = torch.zeros(N, C, H + 2 * r, W + 2 * r, dtype=torch.float64), torch.zeros(N, C, H + 2 * r, W + 2 * r, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            t = float(w[ky, kx]) * gd
            gp[:, :, ky:ky + H, kx:kx + W] += t
            mp[:, :, ky:ky + H, kx:kx + W] += t.abs()
    return gp[:, :, r:r + H, r:r + W], mp[:, :, r:r + H, r:r + W]


def lowpass_adj(g_low, g_high, w, a_h, norm_valid=False):
    """adjoint of x -> (low(x), a_h * (x - low(x))): gx = low^T(g_low) + a_h * (g_high - low^T(g_high)); either gradient may be None (zero).
    Returns (gx, magnitude)."""
    ref = g_low if g_low is not None else g_high
    gx, mag = torch.zeros(ref.shape, dtype=torch.float64), torch.zeros(ref.shape, dtype=torch.float64)
    if g_low is not None:
        gx, mag = _lowpass_t(g_low, w, norm_valid)
    if g_high is not None:
        t, tm = _lowpass_t(g_high, w, norm_valid)
        gx, mag = gx + a_h * (g_high.double() - t), mag + abs(a_h) * (g_high.double().abs() + tm)
    return gx, mag


def lowpass_valid(x, w):
    """un-padded k x k cross-correlation: out[y, x] = sum w[ky, kx] * in[y + ky, x + kx], (H - k + 1) x (W - k + 1).  Returns (out, sum |w * in|)."""
    k = w.shape[0]
    N, C, H, W = x.shape
    Ho, Wo = H - k + 1, W - k + 1
    xd = x.double()
    out, mag = torch.zeros(N, C, Ho, Wo, dtype=torch.float64), torch.zeros(N, C, Ho, Wo, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            t = float(w[ky, kx]) * xd[:, :, ky:ky + Ho, kx:kx + Wo]
            out, mag = out + t, mag + t.abs()
    return out, mag


def lowpass_valid_adj(g, w, H, W):
    """the adjoint of lowpass_valid for any w: gx[y + ky, x + kx] += w[ky, kx] * g[y, x].  Returns (gx [H][W], magnitude)."""
    k = w.shape[0]
    N, C, Ho, Wo = g.shape
    assert (Ho, Wo) == (H - k + 1, W - k + 1)
    gx, mag = torch.zeros(N, C, H, W, dtype=torch.float64), torch.zeros(N, C, H, W, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            t = float(w[ky, kx]) * g.double()
            gx[:, :, ky:ky + Ho, kx:kx + Wo] += t
            mag[:, :, ky:ky + Ho, kx:kx + Wo] += t.abs()
    return gx, mag


# ---- domain-distance map ---------------------------------------------------------------------------------------------------------------
def ddm_spread(d, H, W, convnet):
    """the scatter form of oracle/dsn_dataset.py: every value of d [N][1][n_h][n_w] added over its receptive-field window, divided by the same
    spread of ones; (jump, rf, start) of the walk over the WIDTH serve both axes.  Returns (map, spread of |d| / count, count, (n_h, n_w, jump, rf,
    start))."""
    from oracle.dsn_dataset import receptive, spread
    lay_h, lay_w = receptive(H, convnet), receptive(W, convnet)
    dn = d.double().numpy()
    assert dn.shape[1:] == (1, lay_h[0], lay_w[0]), (dn.shape, lay_h, lay_w)
    shape = (dn.shape[0], 1, H, W)
    cnt = spread(np.ones_like(dn), shape, lay_h, lay_w)
    with np.errstate(invalid='ignore', divide='ignore'):
        v, mag = spread(dn, shape, lay_h, lay_w) / cnt, spread(np.abs(dn), shape, lay_h, lay_w) / cnt
    return torch.from_numpy(v), torch.from_numpy(mag), torch.from_numpy(cnt), (lay_h[0],) + tuple(lay_w)


def bilinear_up(src, f):
    """F.interpolate(mode='bilinear', align_corners=False) of [N][1][h][w] by the integer factor f: source coordinate (o + 0.5) / f - 0.5, clamped at
    0, the upper neighbour clamped at the last index.  Returns (value, sum of weight * |corner|)."""
    N, _, h, w = src.shape
    s = src.double()

    def axis(n_in):
        c = ((torch.arange(n_in * f, dtype=torch.float64) + 0.5) / f - 0.5).clamp_min(0.0)
        i0 = c.floor().long().clamp_max(n_in - 1)
        i1 = (i0 + 1).clamp_max(n_in - 1)
        return i0, i1, c - i0.double()
    y0, y1, ly = axis(h)
    x0, x1, lx = axis(w)
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    out, mag = 0.0, 0.0
    for yi, wy in ((y0, 1.0 - ly), (y1, ly)):
        for xi, wx in ((x0, 1.0 - lx), (x1, lx)):
            t = (wy * wx) * s[:, :, yi][:, :, :, xi]
            out, mag = out + t, mag + t.abs()
    return out, mag


# ---- DSN losses -------------------------------------------------------------------------------------------------------------------------
def logloss(x, mode, eps):
    """-log losses on p = sigmoid(logit): mode 0 l = -log(p + eps), mode 1 l = -log(1 - p + eps).  Returns (l, p, dl/dlogit) per pixel."""
    v = x.double()
    p = 1.0 / (1.0 + torch.exp(-v))
    dp = p * (1.0 - p)
    if mode == 0:
        return -torch.log(p + eps), p, -dp / (p + eps)
    return -torch.log(1.0 - p + eps), p, dp / (1.0 - p + eps)


def sigmoid_bwd(y, g):
    """backward of y = sigmoid(z): gz = g * y * (1 - y)"""
    v = g.double() * y.double() * (1.0 - y.double())
    return v, v.abs()


# ---- normalisation, gradient-penalty and GAN-loss kernels (first half of csrc/gan.hip) ------------------------------------------------------
# These references return Ev pairs: the fp64 value `v` and, beside it, `e`: a running first-order bound of the error of an fp32 evaluation of the
# same expression, in units of the unit roundoff u32 (as adam's E* above): fl(x op y) = (x op y)(1 + d), |d| <= u, so every operation adds the
# magnitude of its result and passes its operands' bounds on through its derivative (second-order products of two bounds are kept: they matter where
# a difference cancels).  A fused multiply-add rounds once where two roundings are counted: the bound holds either way.  Division and sqrtf are
# correctly rounded (1); expf, logf and log1pf are accurate to 1 ulp = 2 u of their result (the allowance of tests/test_gpu_filters.py for
# dasr_logloss).  A sum is counted along the kernel's own chain: Ev.sum(dims, L) adds L u sum |terms|, L = the longest chain of roundings behind
# the total.  What the kernels READ from memory (stats, a, x, gamma, beta, sums, part) is an input here, widened from the fp32 values: never
# recomputed, so that a LeakyReLU branch is decided from the same bits on both sides.
# `wrong=`: the deliberately wrong variants tests/test_blocked_ref.py uses to show that the bounds have teeth; None everywhere else.
TINY32 = 2.0 ** -126                      # smallest normal fp32: the absolute allowance for a result that underflows (flushed or subnormal)


def _t64(x):
    return x.double() if torch.is_tensor(x) else torch.tensor(float(x), dtype=torch.float64)


class Ev:
    __slots__ = ('v', 'e')

    def __init__(self, v, e=None):
        self.v = _t64(v)
        self.e = torch.zeros_like(self.v) if e is None else _t64(e) + torch.zeros_like(self.v)

    @staticmethod
    def of(x):
        """an exact input (or an Ev as it is)"""
        return x if isinstance(x, Ev) else Ev(x)

    @staticmethod
    def rounded(c):
        """a constant the kernel computes with one rounding (1.f / count, 1.f / slope, 1.f - momentum)"""
        return Ev(c, abs(c))

    def _bin(self, v, e_in):
        return Ev(v, e_in + v.abs() + U32 * e_in)     # the propagated bound, one rounding of the result (and of what the bound adds to it)

    def __add__(self, o):
        o = Ev.of(o)
        return self._bin(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Ev.of(o)
        return self._bin(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = Ev.of(o)
        return self._bin(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + U32 * self.e * o.e)

    __radd__, __rmul__ = __add__, __mul__

    def __rsub__(self, o):
        return Ev.of(o) - self

    def __truediv__(self, o):
        o = Ev.of(o)
        q = self.v / o.v
        return self._bin(q, (self.e + q.abs() * o.e) / o.v.abs())

    def __rtruediv__(self, o):
        return Ev.of(o) / self

    def __neg__(self):
        return Ev(-self.v, self.e)

    def abs(self):
        return Ev(self.v.abs(), self.e)

    def relu(self):
        return Ev(self.v.clamp_min(0.0), self.e)

    def sqrt(self):
        r = self.v.sqrt()
        return Ev(r, self.e / (2.0 * r) + r)

    def exp(self):
        r = self.v.exp()
        return Ev(r, self.e * r + 2.0 * r)

    def log(self, floor=None):
        """of a positive argument.  Not the linearisation e / v: with d = u32 e the evaluated argument lies in [v - d, v + d], and in [floor, v + d]
        when the caller knows a floor of it (s + eps >= eps (1 - u) for any fp32 s >= 0), so the result moves by at most log1p(d / v) upwards and
        -log1p(-d / v) or log(v / floor) downwards (no bound, inf, where d >= v and there is no floor)"""
        r = self.v.log()
        d = U32 * self.e
        down = torch.where(d < self.v, -torch.log1p(-(d / self.v).clamp_max(1.0 - 1e-16)), torch.full_like(r, float('inf')))
        if floor is not None:
            down = torch.minimum(down, (self.v / floor).log().clamp_min(0.0))
        return Ev(r, torch.maximum(torch.log1p(d / self.v), down) / U32 + 2.0 * r.abs())

    def over_plus(self, c):
        """v / (v + c) for v >= 0 and a constant c > 0, as ONE function of v: numerator and denominator carry the same error of v, which a quotient
        of two independently bounded operands would count twice and against each other.  d/dv = c / (v + c)^2, largest at the lower end of the
        interval of v; then the sum (1) and the quotient (1)"""
        r = self.v / (self.v + c)
        lo = (self.v - U32 * self.e).clamp_min(0.0)
        return Ev(r, self.e * c / (lo + c) ** 2 + 2.0 * r.abs())

    def log1p(self):
        r = self.v.log1p()
        return Ev(r, self.e / (1.0 + self.v).abs() + 2.0 * r.abs())

    def sum(self, dims, L):
        """the total over `dims` (kept), reached through at most L roundings per term"""
        return Ev(self.v.sum(dims, keepdim=True), self.e.sum(dims, keepdim=True) + L * self.v.abs().sum(dims, keepdim=True))

    def where(self, cond, other):
        other = Ev.of(other)
        return Ev(torch.where(cond, self.v, other.v + torch.zeros_like(self.v)), torch.where(cond, self.e, other.e + torch.zeros_like(self.e)))

    def __getitem__(self, i):
        return Ev(self.v[i], self.e[i])

    def tol(self):
        """the bound |fp32 evaluation - v| <= u32 e (+ the underflow allowance)"""
        return U32 * self.e + TINY32


class F32(Ev):
    """the same interface evaluated in stock torch fp32 (no bound): under fp32_arithmetic() every reference above runs in it, which is how
    tests/test_blocked_ref.py shows that plain fp32 arithmetic in another order of summation meets the bounds"""
    __slots__ = ()

    def __init__(self, v, e=None):
        self.v = v.float() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float32)
        self.e = torch.zeros_like(self.v)

    def _bin(self, v, e_in):
        return F32(v)

    def sum(self, dims, L):
        return F32(self.v.sum(dims, keepdim=True))


class _arithmetic:
    kind = None

    def __enter__(self):
        self.prev = globals()['Ev']
        globals()['Ev'] = self.kind or _Ev64

    def __exit__(self, *exc):
        globals()['Ev'] = self.prev


class fp32_arithmetic(_arithmetic):
    kind = F32


class fp64_arithmetic(_arithmetic):
    """(inside fp32_arithmetic: what builds INPUTS stays in fp64)"""


def ev_cat(parts, dim=0):
    return Ev(torch.cat([p.v for p in parts], dim), torch.cat([p.e for p in parts], dim))


_Ev64 = Ev


def lane_chain(count_per_lane):
    """roundings behind a sum of the norm kernels (one workgroup, 64 pixel lanes per channel quad): the lane's own terms, four xor-butterfly steps
    over lane bits 2..5, three adds over the four waves"""
    return count_per_lane + 4 + 3


def _lrelu_ev(v, slope):
    """LeakyReLU of a COMPUTED value: where |v| is within its own bound the fp32 evaluation may take the other branch; both results then lie within
    that bound of zero and of each other, so the bound passes with factor 1 there"""
    out = v.where(v.v > 0, v * slope)
    near = v.v.abs() <= U32 * v.e
    return Ev(out.v, torch.where(near, v.e + out.v.abs(), out.e))


def _norm_stats(X, dims, cnt, T, eps, wrong=None, stat_rows=None):
    """two-pass statistics over `dims` (kept) as the forward kernels take them: mean = sum / cnt; var = sum (x - mean)^2 / cnt (biased); rstd =
    1 / sqrt(var + eps).  sum (x - m')^2 / cnt = var + (m' - mean)^2 EXACTLY for any m': the error of the computed mean enters the variance in
    second order only, which is what is added here (a first-order pass through 2 |d| would not see that the d sum to zero)."""
    L = lane_chain(T)
    Xs = X if stat_rows is None else X[stat_rows]
    inv = Ev.rounded(1.0 / (cnt - 1 if wrong == 'mean_count-1' else cnt))
    mean = Xs.sum(dims, L) * inv
    d0 = Xs - mean.v                                   # (x - mean) with the exact mean: one rounding
    inv_v = Ev.rounded(1.0 / (cnt - 1 if wrong == 'unbiased' else cnt))
    var = (d0 * d0).sum(dims, L) * inv_v
    var = Ev(var.v, var.e + U32 * mean.e * mean.e * (1.0 + U32 * L))
    rstd = 1.0 / (var + (0.0 if wrong == 'no_eps' else eps)).sqrt()
    return mean, var, rstd


def inorm_lrelu_fwd(x, eps, slope, wrong=None):
    """nn.InstanceNorm2d(affine=False, eps) + LeakyReLU.  Returns (y, mean, rstd) as Ev; mean / rstd [N][C][1][1]."""
    N, C, H, W = x.shape
    X = Ev(x)
    mean, var, rstd = _norm_stats(X, (2, 3), H * W, (H * W + 63) // 64, eps, wrong)
    return _lrelu_ev((X - mean) * rstd, slope), mean, rstd


def _xhat_from_a(a, slope, wrong=None):
    """xhat from the saved output a = lrelu(xhat), and LeakyReLU' there: a > 0 ? (a, 1) : (a / slope, slope) -- at a == +0 and -0 the slope branch"""
    A = Ev(a)
    pos = a.double() >= 0 if wrong == 'lrelu1_at0' else a.double() > 0
    return pos, A.where(pos, A * Ev.rounded(1.0 / slope))


def inorm_lrelu_bwd(a, ga, rstd, slope, wrong=None):
    """gx = rstd (gy - mean gy - xhat mean(gy xhat)), gy = ga lrelu'(a); rstd [N][C][1][1] as the forward stored it"""
    N, C, H, W = a.shape
    L, inv = lane_chain((H * W + 63) // 64), Ev.rounded(1.0 / (H * W))
    pos, xh = _xhat_from_a(a, slope, wrong)
    G = Ev(ga)
    gy = G.where(pos, G * slope)
    m1, m2 = gy.sum((2, 3), L) * inv, (gy * xh).sum((2, 3), L) * inv
    return Ev(rstd) * ((gy - m1) - xh * m2)


def inorm_lrelu_jvp(a, t, rstd, slope, wrong=None):
    """out = lrelu'(a) rstd (t - mean t - xhat mean(t xhat))"""
    N, C, H, W = a.shape
    L, inv = lane_chain((H * W + 63) // 64), Ev.rounded(1.0 / (H * W))
    pos, xh = _xhat_from_a(a, slope, wrong)
    T_ = Ev(t)
    m1, m2 = T_.sum((2, 3), L) * inv, (T_ * xh).sum((2, 3), L) * inv
    lp = Ev(torch.where(pos, torch.ones_like(xh.v), torch.full_like(xh.v, slope)))
    return (lp * Ev(rstd)) * ((T_ - m1) - xh * m2)


def _second(xh, w, T_, r2, dims, L, inv, out0, wrong=None):
    """out0 - r2 [xhat k0 + pz (w - mw) + pw (t - mz)], k0 = mean(w t) - mean w mean t - 3 mean(w xhat) mean(xhat t)"""
    mw, mz, pw, pz, qq = (s.sum(dims, L) * inv for s in (w, T_, w * xh, xh * T_, w * T_))
    k0 = (qq - mw * mz) - ((2.0 if wrong == 'factor2' else 3.0) * pw) * pz
    return Ev.of(out0) - r2 * ((xh * k0 + pz * (w - mw)) + pw * (T_ - mz))


def inorm_second(a, t, ga, rstd, slope, out0=None, wrong=None):
    """the adjoint of z -> J(z) t for fixed t, upstream w = lrelu'(a) ga; out0: what `accumulate` adds to (None: zero)"""
    N, C, H, W = a.shape
    L, inv = lane_chain((H * W + 63) // 64), Ev.rounded(1.0 / (H * W))
    pos, xh = _xhat_from_a(a, slope, wrong)
    G, R_ = Ev(ga), Ev(rstd)
    w = G.where(pos, G * slope)
    return _second(xh, w, Ev(t), R_ * R_, (2, 3), L, inv, torch.zeros_like(xh.v) if out0 is None else out0, wrong)


# BatchNorm2d in training mode: groups of `group` consecutive images (the last may be ragged), statistics rows [G][C]
def groups(N, group):
    return [(n0, min(N, n0 + group)) for n0 in range(0, N, group)]


def _chan(p, C):
    return _t64(p)[:C].view(1, C, 1, 1)


def bnorm_lrelu_fwd(x, group, eps, slope, gamma, beta, wrong=None):
    """Returns (y [N][C][H][W], z = gamma xhat + beta, mean, rstd, var [G][C]) as Ev"""
    N, C, H, W = x.shape
    X, gm, bt = Ev(x), _chan(gamma, C), _chan(beta, C)
    ys, zs, st = [], [], []
    for n0, n1 in groups(N, group):
        # wrong 'ragged_drop': the images of a ragged last group never enter any statistics (they are normalised with the previous group's)
        rows = slice(n0 - group, n0) if wrong == 'ragged_drop' and n1 - n0 < group else slice(n0, n1)
        nst = rows.stop - rows.start
        mean, var, rstd = _norm_stats(X, (0, 2, 3), nst * H * W, nst * ((H * W + 63) // 64), eps, wrong, rows)
        z = ((X[n0:n1] - mean) * rstd) * gm + bt
        zs.append(z)
        ys.append(_lrelu_ev(z, slope))
        st.append((mean, rstd, var))
    return (ev_cat(ys), ev_cat(zs)) + tuple(ev_cat([s[i] for s in st])[:, :, 0, 0] for i in range(3))


def _bn_group(x, mean, rstd, gamma, beta, g, n0, n1, wrong=None):
    """xhat and z = gamma xhat + beta of group g, recomputed from the saved x and the statistics rows as the backward kernels do"""
    C = x.shape[1]
    row = (mean.shape[0] - 1 - g) if wrong == 'other_row' else g
    R_ = Ev(_t64(rstd)[row].view(1, C, 1, 1))
    xh = (Ev(x[n0:n1]) - _t64(mean)[g].view(1, C, 1, 1)) * R_
    return xh, xh * _chan(gamma, C) + _chan(beta, C), R_


def bnorm_lrelu_bwd(x, ga, group, slope, gamma, beta, mean, rstd, pscale=1.0, wrong=None):
    """per group: gx = gamma rstd (gz - mean gz - xhat mean(gz xhat)), gz = ga lrelu'(z); dgamma = pscale sum over ALL groups of sum gz xhat,
    dbeta = pscale sum gz.  Returns (gx, dgamma [C], dbeta [C], z)."""
    N, C, H, W = x.shape
    gm = _chan(gamma, C)
    outs, zs, dg, db = [], [], Ev(torch.zeros(1, C, 1, 1)), Ev(torch.zeros(1, C, 1, 1))
    for g, (n0, n1) in enumerate(groups(N, group)):
        cnt, L = (n1 - n0) * H * W, lane_chain((n1 - n0) * ((H * W + 63) // 64))
        inv = Ev.rounded(1.0 / cnt)
        xh, z, R_ = _bn_group(x, mean, rstd, gamma, beta, g, n0, n1, wrong)
        G = Ev(ga[n0:n1])
        gz = G.where(z.v > 0, G * slope)
        t1, t2 = gz.sum((0, 2, 3), L), (gz * xh).sum((0, 2, 3), L)
        if g == 0 or wrong != 'dgamma_first':
            db, dg = (t1 if g == 0 else db + t1), (t2 if g == 0 else dg + t2)      # (0 + t is exact)
        outs.append((gm * R_) * ((gz - t1 * inv) - xh * (t2 * inv)))
        zs.append(z)
    return ev_cat(outs), (dg * pscale)[0, :, 0, 0], (db * pscale)[0, :, 0, 0], ev_cat(zs)


def bnorm_lrelu_jvp(x, t, group, slope, gamma, beta, mean, rstd, wrong=None):
    """out = lrelu'(z) gamma rstd (t - mean t - xhat mean(xhat t)).  Returns (out, z)."""
    N, C, H, W = x.shape
    gm = _chan(gamma, C)
    outs, zs = [], []
    for g, (n0, n1) in enumerate(groups(N, group)):
        cnt, L = (n1 - n0) * H * W, lane_chain((n1 - n0) * ((H * W + 63) // 64))
        inv = Ev.rounded(1.0 / cnt)
        xh, z, R_ = _bn_group(x, mean, rstd, gamma, beta, g, n0, n1, wrong)
        T_ = Ev(t[n0:n1])
        o = (gm * R_) * ((T_ - T_.sum((0, 2, 3), L) * inv) - xh * ((T_ * xh).sum((0, 2, 3), L) * inv))
        outs.append(o.where(z.v > 0, o * slope))
        zs.append(z)
    return ev_cat(outs), ev_cat(zs)


def bnorm_second(x, t, ga, group, slope, gamma, beta, mean, rstd, out0=None, dgamma0=None, pscale=1.0, wrong=None):
    """u = lrelu'(z) ga, w = gamma u: out as inorm_second with group means; dgamma = dgamma0 + pscale sum over groups of
    rstd count (mean(u t) - mean u mean t - mean(u xhat) mean(xhat t)).  Returns (out, dgamma [C], z)."""
    N, C, H, W = x.shape
    gm = _chan(gamma, C)
    outs, zs, dg = [], [], None
    for g, (n0, n1) in enumerate(groups(N, group)):
        cnt, L = (n1 - n0) * H * W, lane_chain((n1 - n0) * ((H * W + 63) // 64))
        inv = Ev.rounded(1.0 / cnt)
        xh, z, R_ = _bn_group(x, mean, rstd, gamma, beta, g, n0, n1, wrong)
        T_, G = Ev(t[n0:n1]), Ev(ga[n0:n1])
        u = G.where(z.v > 0, G * slope)
        mu, mz, pu, pz, qu = (s.sum((0, 2, 3), L) * inv for s in (u, T_, u * xh, xh * T_, u * T_))
        d = (R_ * float(cnt)) * ((qu - mu * mz) - pu * pz)
        if g == 0 or wrong != 'dgamma_first':
            dg = d if dg is None else dg + d
        mw, pw = gm * mu, gm * pu
        k0 = ((gm * qu) - mw * mz) - ((2.0 if wrong == 'factor2' else 3.0) * pw) * pz
        w = u * gm
        o0 = torch.zeros_like(xh.v) if out0 is None else out0[n0:n1]
        outs.append(Ev.of(o0) - (R_ * R_) * ((xh * k0 + pz * (w - mw)) + pw * (T_ - mz)))
        zs.append(z)
    dg = (dg * pscale)[0, :, 0, 0]
    return ev_cat(outs), (dg if dgamma0 is None else Ev(_t64(dgamma0)[:C]) + dg), ev_cat(zs)


def bnorm_running(mean, var, count, momentum, rmean0, rvar0, wrong=None):
    """nn.BatchNorm2d's running statistics after one training-mode forward: r = (1 - momentum) r + momentum * (mean | UNBIASED variance =
    biased * count / (count - 1); count 1: the biased one)"""
    keep = Ev.rounded(1.0 - momentum)
    corr = Ev.rounded(1.0 if wrong == 'biased' else float(count) / float(count - 1 if count > 1 else 1))
    return keep * Ev(rmean0) + Ev(mean) * momentum, keep * Ev(rvar0) + (Ev(var) * momentum) * corr


def _sigmoid_ev(z):
    return 1.0 / (1.0 + (-z).exp())


def _bce_ev(z, t):
    """max(z, 0) - z t + log1p(exp(-|z|))"""
    return (z.relu() - z * t) + (-z.abs()).exp().log1p()


def gan_loss(x, gan_type, target, gcoef, wrong=None):
    """GANLoss(gan_type) against a constant target, per element: 0 BCE-with-logits (d = sigmoid(x) - t), 1 (x - t)^2 (d = 2 (x - t)), 2 -x for t > 0.5
    else x (d = -+1).  Returns (l, gcoef * d) as Ev; the score term is x itself."""
    X = Ev(x)
    if gan_type == 0:
        return _bce_ev(X, target), gcoef * (_sigmoid_ev(X) - target)
    if gan_type == 1:
        d = X - target
        return d * d, (gcoef * 2.0) * d
    sgn = -1.0 if (target > 0.5) != (wrong == 'wgan_sign' and target <= 0.5) else 1.0
    return Ev(sgn * X.v), Ev(torch.full_like(X.v, gcoef * sgn))


def _rel_term(z, t, eps, form):
    """(loss, d loss / dz, score) of one relativistic term, forms as dasr_ragan's"""
    s = _sigmoid_ev(z)
    if form == 0:
        return _bce_ev(z, t), s - t, s
    if form == 2:
        d = z - t
        return d * d, 2.0 * d, s
    if form == 3:
        q = -1.0 if t > 0.5 else 1.0
        return Ev(q * z.v, z.e), Ev(torch.full_like(z.v, q)), s
    if t < 0:
        return Ev(torch.zeros_like(z.v)), Ev(torch.zeros_like(z.v)), s
    if t > 0.5:
        return -(s + eps).log(eps * (1.0 - U32)), -(s * (1.0 - s)) / (s + eps), s
    # (the kernel's s (1 - s) / (1 - s + eps): the same three roundings behind s and 1 - s, in another order)
    return -((1.0 - s) + eps).log(eps * (1.0 - U32)), s * (1.0 - s).over_plus(eps), s


def ragan_sums(a, b):
    """stage 0: per pixel sum_n a, sum_n b of this rank's N samples ([N][1][H][W] -> [1][1][H][W])"""
    return Ev(a).sum((0,), a.shape[0]), Ev(b).sum((0,), b.shape[0])


def ragan_terms(a, b, sums_a, sums_b, n_glob, form, ta, tb, eps, wrong=None):
    """stage 1 / 2, per local sample and pixel: za = a - sums_b / n_glob, zb = b - sums_a / n_glob and their terms.  sums_*: the GLOBAL per-pixel sums
    [1][1][H][W] as read from memory.  Returns ((la, da, sa), (lb, db, sb)) as Ev [N][1][H][W]."""
    inv = Ev.rounded(1.0 / (a.shape[0] if wrong == 'means_N' else n_glob))
    ma, mb = Ev(sums_a) * inv, Ev(sums_b) * inv
    return _rel_term(Ev(a) - mb, ta, eps, form), _rel_term(Ev(b) - ma, tb, eps, form)


def ragan_grads(da, db, part_a, part_b, n_glob, gcoef, wrong=None):
    """stage 2: ga = gcoef (da - part_b / n_glob), gb = gcoef (db - part_a / n_glob); part_*: the GLOBAL per-pixel sums of da / db as read from memory"""
    inv = Ev.rounded(1.0 / n_glob)
    if wrong == 'swap_part':
        part_a, part_b = part_b, part_a
    return gcoef * (da - Ev(part_b) * inv), gcoef * (db - Ev(part_a) * inv)


def grad_penalty_sumsq(g):
    """sum of squares over all images and channels: C products and adds per pixel thread, the wave butterfly (6), the four waves (2), then the
    non-zero workgroup partials in order (adding a zero partial is exact)"""
    N, C, H, W = g.shape
    G = Ev(g)
    return (G * G).sum((0, 1, 2, 3), C + 6 + 2 + (N * H * W + 255) // 256)[0, 0, 0, 0]


def grad_penalty_finish(s, weight, world=1, wrong=None):
    """from the (all-reduced) sum of squares s: nrm = sqrt(s / world^2), pen = weight (nrm - 1)^2, factor = 2 weight (nrm - 1) / nrm / world (0 at nrm 0)"""
    s = Ev.of(s)
    if world != 1:
        inv_w = Ev.rounded(1.0 / world)
        s = s if wrong == 'no_world2' else (s * inv_w) * inv_w
    else:
        inv_w = Ev(1.0)
    nrm = s.sqrt() if float(s.v) > 0 else Ev(0.0)
    d = nrm - 1.0
    pen = (weight * d) * d
    fac = ((((2.0 * weight) * d) / nrm) * inv_w) if float(nrm.v) > 0 else Ev(0.0)
    return nrm, pen, fac


def grid_chain(nblocks):
    """roundings behind a loss accumulator once a workgroup has its thread sums: wave butterfly (6), four waves (3), grid_sum_commit's per-thread
    loop over ceil(nblocks / 256) partials, butterfly (6), (a + b) + (c + d) (2), * coef (1), the add into the accumulator (1)"""
    return 6 + 3 + (nblocks + 255) // 256 + 6 + 2 + 1 + 1


def acc_sum(terms, coef, acc0, per_thread, nblocks):
    """acc0 + coef * sum(terms) as a loss / score accumulator holds it: (value, bound).  The per-term bounds, summed, plus the grid-sum convention of
    tests/test_gpu_elementwise.py::test_l1_diff: L u32 (coef sum |terms| + |acc0|), L = the thread's own `per_thread` terms and the grid chain."""
    L = per_thread + grid_chain(nblocks)
    want = acc0 + coef * float(terms.v.sum())
    return want, U32 * abs(coef) * float(terms.e.sum()) + L * U32 * (abs(coef) * float(terms.v.abs().sum()) + abs(acc0)) + TINY32


# ---- LPIPS layers (csrc/lpips.hip), PReLU slope gradient (second half of csrc/gan.hip), fp32 crop gather (csrc/misc.hip) ----------------------
# tests/test_gpu_lpips_prelu.py holds the kernels to these on the inputs of oracle/lpips_prelu_cases.py.
def _ev_map(x, fn):
    """a data movement applied to value and bound alike"""
    return Ev(fn(x.v), fn(x.e))


def dihedral_map(H, W, xf):
    """index maps (U, V) [H][W] of dasr_lpips_s2d's symmetry code: T(x)[i][j] = x[U[i][j]][V[i][j]], (u, v) = (i, j), swapped if bit 0, then
    u -> H-1-u if bit 1, v -> W-1-v if bit 2 (transposing codes need H == W)"""
    assert not (xf & 1) or H == W
    i, j = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    u, v = (j, i) if xf & 1 else (i, j)
    return (H - 1 - u if xf & 2 else u), (W - 1 - v if xf & 4 else v)


def _chan3(p):
    return torch.tensor([f32(s) for s in p[:3]], dtype=torch.float64).view(1, 3, 1, 1)


def lpips_s2d(x, scale, shift, xf=0, wrong=None):
    """mode 0: the symmetry T, then scale[c] * T(x) + shift[c] (2 roundings), zero padding by 2 applied to the SCALED image, 4x4 space-to-depth:
    x [N][3][H][W] -> [N][48][(H+4)/4][(W+4)/4], channel 16 c + 4 by + bx = pixel (4Y + by - 2, 4X + bx - 2) of colour c; exact +0 in the padding"""
    N, _, H, W = x.shape
    U, V = dihedral_map(H, W, xf)
    tx = x.double()[:, :, U, V]
    pad = lambda t: torch.nn.functional.pad(t, (2, 2, 2, 2))
    if wrong == 'border_shift':           # zero padding in front of the affine map: a border pixel holds shift[c]
        s = Ev(pad(tx)) * _chan3(scale) + _chan3(shift)
    else:
        s = _ev_map(Ev(tx) * _chan3(scale) + _chan3(shift), pad)
    Hs, Ws = (H + 4) // 4, (W + 4) // 4
    order = (0, 1, 5, 3, 2, 4) if wrong == 'block_xy' else (0, 1, 3, 5, 2, 4)
    return _ev_map(s, lambda t: t.reshape(N, 3, Hs, 4, Ws, 4).permute(*order).reshape(N, 48, Hs, Ws))


def lpips_s2d_adj(gy, x0, scale, xf=0, wrong=None):
    """mode 1: x0[c][u][v] + scale[c] * gy[the slot pixel (u, v) went to] (2 roundings): the gradient of T(x)[i][j] goes back to x[U[i][j]][V[i][j]]"""
    N, _, H, W = x0.shape
    Hs, Ws = (H + 4) // 4, (W + 4) // 4
    g = gy.double().reshape(N, 3, 4, 4, Hs, Ws).permute(0, 1, 4, 2, 5, 3).reshape(N, 3, 4 * Hs, 4 * Ws)[:, :, 2:2 + H, 2:2 + W]
    U, V = dihedral_map(H, W, xf)
    if wrong == 'adj_forward_map':        # reads through the forward map where its inverse is due (the same thing unless T is a quarter turn)
        back = g[:, :, U, V]
    else:
        back = torch.zeros_like(g)
        back[:, :, U, V] = g
    return Ev(x0) + Ev(back) * _chan3(scale)


def maxpool3s2(x):
    """nn.MaxPool2d(3, 2): (the maximum in x's dtype, d = 3 dy + dx of the first maximum in scan order)"""
    _, am = _first_max(x.double(), 3, 2)
    return _take(x, am, 3, 2), am


def maxpool3s2_bwd(x, gy, relu_mask, gx0=None, wrong=None):
    """gx[iy][ix] = sum of gy over the (at most 2 x 2) windows whose FIRST maximum the pixel is, added in the kernel's order (window rows, then
    columns, ascending: the first add is to zero and exact, three more, one for `accumulate`); relu_mask: zero where x <= 0; gx0: what accumulate
    adds to.  A row / column no window covers gets zero."""
    N, C, H, W = x.shape
    _, am = _first_max(x.double(), 3, 2, last=wrong == 'last_max')
    Ho, Wo = am.shape[2], am.shape[3]
    g = gy.double()
    # slot (a, b): a = 0 the upper of the two window rows a pixel can belong to (dy = 2), a = 1 the lower (dy = 0 or 1); b likewise for columns
    slots = [[torch.zeros(N, C, H, W, dtype=torch.float64) for _ in range(2)] for _ in range(2)]
    for d in range(9):
        dy, dx = d // 3, d % 3
        slots[int(dy < 2)][int(dx < 2)][:, :, dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2] += torch.where(am == d, g, torch.zeros_like(g))
    acc = ((Ev(slots[0][0]) + Ev(slots[0][1])) + Ev(slots[1][0])) + Ev(slots[1][1])
    if relu_mask:
        keep = x.double() >= 0 if wrong == 'relu_ge' else x.double() > 0
        acc = acc.where(keep, 0.0)
    return acc if gx0 is None else acc + Ev(gx0)


def _sqrt0(q):
    """sqrt of a sum of squares that may be EXACTLY zero (every term zero, bound zero): 0 with bound 0"""
    r = q.sqrt()
    zero = q.v == 0
    assert bool((q.e[zero] == 0).all())
    return Ev(torch.where(zero, torch.zeros_like(r.v), r.v), torch.where(zero, torch.zeros_like(r.e), r.e))


def lpips_head(f0, f1, lin, eps, gcoef, relu_mask, wrong=None):
    """one LPIPS layer per pixel, as the kernel evaluates it (sums over the C channels: chains of C adds):
        q_k = sum f_k^2; r0 = sqrt(q0); s_k = sqrt(q_k) + eps; i_k = 1 / s_k; d = f0 i0 - f1 i1; val = sum (w d) d; dot = sum ((2 w) d) f0
        k2 = dot / ((r0 s0) s0), 0 where r0 == 0 (the derivative of the norm taken as 0 at the origin); g0 = gcoef (((2 w) d) i0 - f0 k2),
        zero where f0 <= 0 when relu_mask.
    Returns (val [N][1][H][W], g0 [N][C][H][W]) as Ev."""
    C = f0.shape[1]
    X0, X1, Wt = Ev(f0), Ev(f1), lin.double().view(1, C, 1, 1)
    q0, q1 = (X0 * X0).sum((1,), C), (X1 * X1).sum((1,), C)
    r0 = _sqrt0(q0)
    if wrong == 'eps_in_sqrt':
        s0, s1 = (q0 + eps).sqrt(), (q1 + eps).sqrt()
    else:
        s0, s1 = r0 + eps, _sqrt0(q1) + eps
    i0, i1 = 1.0 / s0, 1.0 / s1
    d = X0 * i0 - X1 * i1
    val = ((d * Wt) * d).sum((1,), C)
    dot = ((d * (2.0 * Wt)) * X0).sum((1,), C)
    den = (s0 * s0) * s0 if wrong == 'k2_s0cubed' else (r0 * s0) * s0
    k2 = (dot / den).where(r0.v > 0, 0.0)
    g0 = (d * (2.0 * Wt)) * i0
    if wrong != 'no_x0k2':
        g0 = g0 - X0 * k2
    g0 = g0 * gcoef
    if relu_mask:
        g0 = g0.where((f1 if wrong == 'relu_f1' else f0).double() > 0, 0.0)
    return val, g0


# roundings behind a workgroup's total once its 256 threads hold their sums in double (whose own error, a few 2^-53, rounds into the first): the
# cast to fp32 (1), the wave butterfly (6), the four waves (3)
BLOCK_CHAIN = 1 + 6 + 3


def prelu_grad(y, gx, a, scale, wrong=None):
    """dL/da of a shared PReLU slope from the layer output y and gx = dL/dx: scale * sum_{y <= 0} gx y / a^2.  Every term is rounded to fp32 once
    (exact for f16 inputs), both stages sum per thread in double and finish with BLOCK_CHAIN roundings, then scale * tot (1), a * a (1), the
    division (1): all of it relative to sum |terms|.  At y == +0 and -0 the term is an exact zero: `y <= 0` and `y < 0` give the same value for
    finite gx (wrong 'y_lt' shows it)."""
    take = y.double() < 0 if wrong == 'y_lt' else y.double() <= 0
    if wrong == 'skip_plane':
        take = take.clone()
        take[-1, -16:] = False
    tot = (Ev(gx) * Ev(y)).where(take, 0.0).sum((0, 1, 2, 3), 2 * BLOCK_CHAIN)[0, 0, 0, 0]
    A = Ev(a)
    return (tot * scale) / (A if wrong == 'div_a' else A * A)


def prelu_final(partial, slopes, scale, wrong=None):
    """the second stage alone: partial [count][nblocks] -> scale * sum / a_k^2 per row"""
    tot = Ev(partial).sum((1,), BLOCK_CHAIN)[:, 0]
    A = Ev(torch.tensor([f32(s) for s in slopes], dtype=torch.float64))
    return (tot * scale) / (A if wrong == 'div_a' else A * A)


def _crop_axis(v, n_src, n_view, wrong=None):
    """cv2.INTER_LINEAR source coordinate f = (v + 0.5) n_src / n_view - 0.5 of view index v, from exact integer arithmetic: (floor(f), f - floor(f),
    delta): delta bounds |fp32 f - f| (the division, the product and the difference of the kernel's expression) plus one rounding of the weight"""
    v = v.long()
    num = 2 * v * n_src if wrong == 'no_half_pixel' else (2 * v + 1) * n_src - n_view
    den = 2 * n_view
    i0 = torch.div(num, den, rounding_mode='floor')
    f = (_Ev64(v.double() + 0.5) * (_Ev64(float(n_src)) / _Ev64(float(n_view)))) - 0.5
    return i0, (num - i0 * den).double() / den, U32 * f.e + U32


def _crop_fp32(img, vy, vx, vH, vW, below):
    """the kernel's own bilinear expression in stock fp32; below: where the exact coordinate is an integer, floorf is taken to have landed on the
    other side of it (index one lower, weight the largest fp32 below 1)"""
    _, H, W = img.shape
    one = torch.tensor(1.0)

    def axis(v, n_src, n_view):
        f = (v.float() + 0.5) * (torch.tensor(float(n_src)) / torch.tensor(float(n_view))) - 0.5
        i0 = torch.floor(f)
        w = f - i0
        if below:
            hit = ((2 * v.long() + 1) * n_src - n_view) % (2 * n_view) == 0
            i0, w = torch.where(hit, i0 - 1.0, i0), torch.where(hit, torch.tensor(1.0 - 2.0 ** -24), w)
        i0 = i0.long()
        return i0.clamp(0, n_src - 1), (i0 + 1).clamp(0, n_src - 1), w
    ya, yb, wy = axis(vy, H, vH)
    xa, xb, wx = axis(vx, W, vW)
    s = img.float()
    return (one - wy) * ((one - wx) * s[:, ya, xa] + wx * s[:, ya, xb]) + wy * ((one - wx) * s[:, yb, xa] + wx * s[:, yb, xb])


def gather_crops(descs, C, size, wrong=None):
    """dasr_gather_crops: sample k = the size x size window at (y0, x0) of image `img` [c][H][W] -- resized bilinearly to vH x vW first when that
    differs from H x W (cv2.INTER_LINEAR: half-pixel centres, edge clamp) -- then hflip (flags bit 0), vflip (bit 1), transpose (bit 2), in that
    order; zero for channels >= c and wherever the window leaves the view.  descs: dicts(img, vH, vW, y0, x0, flags).
    Returns (dst [n][C][size][size] as Ev, exact [n][C][size][size] bool: pure data movement or zero fill).  The bound of a resized sample: the six
    roundings of the blend, relative to the sum of weight * |corner|, plus the fp32 error of each source coordinate times the steepest slope of the
    (continuous, piecewise linear) interpolant over the cells on both sides of the coordinate -- which also covers a floorf that lands across an integer.
    wrong 'floor_below' (fp32 arithmetic only) plays exactly that."""
    fp32 = Ev is F32
    n = len(descs)
    val, err = torch.zeros(n, C, size, size, dtype=torch.float64), torch.zeros(n, C, size, size, dtype=torch.float64)
    exact = torch.ones(n, C, size, size, dtype=torch.bool)
    ys, xs = torch.meshgrid(torch.arange(size), torch.arange(size), indexing='ij')
    for k, D in enumerate(descs):
        img, fl = D['img'], D['flags']
        c, H, W = img.shape
        ci, cj = ys, xs
        if wrong == 'flip_order':         # flips undone in front of the transpose
            ci, cj = (size - 1 - ci if fl & 2 else ci), (size - 1 - cj if fl & 1 else cj)
            ci, cj = (cj, ci) if fl & 4 else (ci, cj)
        else:
            ci, cj = (cj, ci) if fl & 4 else (ci, cj)
            ci, cj = (size - 1 - ci if fl & 2 else ci), (size - 1 - cj if fl & 1 else cj)
        vy, vx = D['y0'] + ci, D['x0'] + cj
        inside = (vy >= 0) & (vy < D['vH']) & (vx >= 0) & (vx < D['vW'])
        vy, vx = vy.clamp(0, D['vH'] - 1), vx.clamp(0, D['vW'] - 1)
        s = img.double()
        cc = min(c, C)
        if (D['vH'], D['vW']) == (H, W):
            val[k, :cc] = torch.where(inside, s[:cc, vy, vx], torch.zeros(()).double())
            continue
        exact[k, :cc] = ~inside
        if fp32:
            val[k, :cc] = torch.where(inside, _crop_fp32(img, vy, vx, D['vH'], D['vW'], wrong == 'floor_below')[:cc].double(), torch.zeros(()).double())
            continue
        ya, wy, dy = _crop_axis(vy, H, D['vH'], wrong)
        xa, wx, dx = _crop_axis(vx, W, D['vW'], wrong)

        def px(yi, xi):
            ok = ((yi >= 0) & (yi < H) & (xi >= 0) & (xi < W)) if wrong == 'no_clamp' else torch.ones_like(inside)
            return torch.where(ok, s[:, yi.clamp(0, H - 1), xi.clamp(0, W - 1)], torch.zeros(()).double())
        v, mag = 0.0, 0.0
        for yi, a in ((ya, 1.0 - wy), (ya + 1, wy)):
            for xi, b in ((xa, 1.0 - wx), (xa + 1, wx)):
                t = (a * b) * px(yi, xi)
                v, mag = v + t, mag + t.abs()
        cl = lambda yi, xi: s[:, yi.clamp(0, H - 1), xi.clamp(0, W - 1)]
        Ly = torch.stack([(cl(ya + r + 1, xa + q) - cl(ya + r, xa + q)).abs() for r in (-1, 0, 1) for q in (-1, 0, 1, 2)]).max(0).values
        Lx = torch.stack([(cl(ya + r, xa + q + 1) - cl(ya + r, xa + q)).abs() for r in (-1, 0, 1, 2) for q in (-1, 0, 1)]).max(0).values
        e = (6.0 * mag + (dy * Ly + dx * Lx) / U32)
        val[k, :cc] = torch.where(inside, v[:cc], torch.zeros(()).double())
        err[k, :cc] = torch.where(inside, e[:cc], torch.zeros(()).double())
    return Ev(val, err), exact
