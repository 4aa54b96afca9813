"""Plain torch-CPU references of the small kernels of csrc/misc.hip / csrc/gan.hip (elementwise, pooling, pixel losses, Adam; the frequency-split,
domain-distance-map and DSN loss kernels), and the NC16HW16 layout plumbing the GPU tests need.  No device code: tests/test_blocked_ref.py holds every
function here to stock torch on a machine without a GPU; tests/test_gpu_elementwise.py and tests/test_gpu_filters.py then hold the kernels to these.

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


def _first_max(x):
    """x: NCHW fp64 (H, W may be odd: the last row / column takes no part).  (max, d) per 2x2 window, d = 2 dy + dx of the FIRST maximum in scan
    order (a later candidate replaces the current one only if it is strictly greater)"""
    Ho, Wo = x.shape[2] // 2, x.shape[3] // 2
    xc = x[:, :, :2 * Ho, :2 * Wo]
    cand = [xc[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
    m, am = cand[0].clone(), torch.zeros(cand[0].shape, dtype=torch.long)
    for d in (1, 2, 3):
        up = cand[d] > m
        m = torch.where(up, cand[d], m)
        am = torch.where(up, torch.full_like(am, d), am)
    return m, am


def _take(t, am):
    """element of the first maximum out of every 2x2 window of t (any dtype: moved, not computed)"""
    Ho, Wo = am.shape[2], am.shape[3]
    tc = t[:, :, :2 * Ho, :2 * Wo]
    cand = torch.stack([tc[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)], dim=-1)
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
