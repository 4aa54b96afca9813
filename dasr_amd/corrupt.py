"""The two corruptions of codes/DSN/add_corruptions.py on 8-bit RGB images: rounded Gaussian noise (utils.py:20-22) and the round trip through a JPEG file
(add_corruptions.py:49-54: Image.save(path, 'JPEG', quality=q), Image.open, remove).

The file is decoded right after it is encoded, so the entropy coder is a lossless no-op and is left out.  What remains is integer work per 8 x 8 block and per pixel,
stated once on the host in numpy (jpeg_roundtrip_ref, gaussian_noise_ref: what the tests pin everything to) and once in HIP (csrc/corrupt.hip: jpeg_roundtrip,
gaussian_noise on uint8 device tensors, no host synchronisation).  `python -m dasr_amd.add_corruptions` runs them on folders.

jpeg_roundtrip_ref is baseline JPEG as PIL writes an RGB image by default with libjpeg-turbo: 4:2:0, the slow-integer ("islow") DCT of jfdctint.c / jidctint.c, the
h2v2 "fancy" (triangle) chroma up-sampling of jdsample.c, bit for bit (tests/golden/jpeg_roundtrip.npz holds PIL's own outputs).

gaussian_noise_ref draws from a counter-based generator of this project's own (Philox4x32-10 and Box-Muller in fp64), a function of (seed, image index, element index)
only.  It is NOT numpy's stream: the reference never seeds its generator (utils.py:20-22 calls np.random.normal unseeded), so there is no stream to be equal to."""
import numpy as np

# ---- quantisation tables: Annex K of ITU-T T.81, natural (row-major) order -----------------------------------------------------------
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def check_quality(quality):
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError('the JPEG quality must be an integer in 1 .. 100, got %r' % (quality,))
    return q


def quant_tables(quality):
    """(luminance, chrominance) int64 [8, 8] of jpeg_set_quality(quality, force_baseline)"""
    q = min(100, max(1, int(quality)))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(b, dtype=np.int64).reshape(8, 8) * s + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one pass of jfdctint.c along the last axis of d [..., 8]"""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    o = [None] * 8
    o[0] = (t10 + t11) << PASS1_BITS if first else _descale(t10 + t11, PASS1_BITS)
    o[4] = (t10 - t11) << PASS1_BITS if first else _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F_0_541
    o[2] = _descale(z1 + t13 * F_0_765, n)
    o[6] = _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _idct_pass(c, first):
    """one pass of jidctint.c along the last axis of c [..., 8]"""
    c = [c[..., k] for k in range(8)]
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS + 3
    z1 = (c[2] + c[6]) * F_0_541
    t2, t3 = z1 - c[6] * F_1_847, z1 + c[2] * F_0_765
    t0, t1 = (c[0] + c[4]) << CONST_BITS, (c[0] - c[4]) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, n) for v in o], axis=-1)


def _code_plane(p, Q):
    """p int64 [h, w], h and w multiples of 8 -> the decoded plane: per 8 x 8 block forward DCT, quantise, dequantise, inverse DCT"""
    h, w = p.shape
    b = (p - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)                       # [by, bx, row, col]
    c = _fdct_pass(_fdct_pass(b, True).swapaxes(-1, -2), False).swapaxes(-1, -2)            # rows, then columns: 8 x the DCT
    q = np.sign(c) * ((np.abs(c) + ((8 * Q) >> 1)) // (8 * Q)) * Q
    d = _idct_pass(_idct_pass(q.swapaxes(-1, -2), True).swapaxes(-1, -2), False)            # columns, then rows
    return np.clip(d + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w)


def _pad(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode='edge')


def jpeg_roundtrip_ref(img_u8_hwc, quality):
    """uint8 [H, W, 3] RGB -> what Image.save(buf, 'JPEG', quality=quality) followed by Image.open gives back, in integer arithmetic only.  Any H, W >= 1."""
    quality = check_quality(quality)
    img = np.asarray(img_u8_hwc)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError('the image must be uint8 [H, W, 3], got %s %s' % (img.dtype, img.shape))
    H, W = img.shape[:2]
    QY, QC = quant_tables(quality)
    R, G, B = (img[..., k].astype(np.int64) for k in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    Wp = -(-W // 16) * 16
    h, w = -(-H // 2), -(-W // 2)
    Yd = _code_plane(_pad(Y, -(-H // 8) * 8, Wp), QY)

    def chroma(P):
        P = _pad(P, 2 * h, Wp)                                                              # columns to a multiple of 16, at most one repeated row
        bias = np.tile(np.array([1, 2], dtype=np.int64), Wp // 4)
        a = (P[0::2, 0::2] + P[0::2, 1::2] + P[1::2, 0::2] + P[1::2, 1::2] + bias) >> 2
        d = _code_plane(_pad(a, -(-h // 8) * 8, Wp // 2), QC)[:h, :w]                        # the last AVERAGED row repeated down to a multiple of 8
        if w <= 2:
            return np.repeat(np.repeat(d, 2, axis=0), 2, axis=1)[:H, :W]
        up, down = np.concatenate([d[:1], d[:-1]]), np.concatenate([d[1:], d[-1:]])
        v = np.empty((2 * h, w), dtype=np.int64)
        v[0::2], v[1::2] = 3 * d + up, 3 * d + down
        left, right = np.concatenate([v[:, :1], v[:, :-1]], axis=1), np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
        o = np.empty((2 * h, 2 * w), dtype=np.int64)
        o[:, 0::2], o[:, 1::2] = (3 * v + left + 8) >> 4, (3 * v + right + 7) >> 4          # (at the two ends left / right is the sample itself: 4 v + 8, 4 v + 7)
        return o[:H, :W]
    Yd, cb, cr = Yd[:H, :W], chroma(Cb) - 128, chroma(Cr) - 128
    out = np.stack([Yd + ((91881 * cr + 32768) >> 16), Yd + ((-22554 * cb - 46802 * cr + 32768) >> 16), Yd + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- noise: Philox4x32-10 + Box-Muller --------------------------------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter = four uint32 arrays (or ints), key = two; returns four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def normal_ref(n, seed, index):
    """the n standard normal samples (float64) of image `index` under `seed`: element e is output e % 4 of the group e // 4"""
    n, seed, index = int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(index)
    if not 0 <= index < 1 << 32:
        raise ValueError('the image index must lie in 0 .. 2^32 - 1, got %d' % index)
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    x = philox4x32((g & _M32, g >> np.uint64(32), np.full(g.shape, index, dtype=np.uint64), np.zeros(g.shape, dtype=np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
    z = np.empty((g.size, 4), dtype=np.float64)
    for k in (0, 2):
        u1, u2 = (x[k].astype(np.float64) + 1.0) * 2.0 ** -32, x[k + 1].astype(np.float64) * 2.0 ** -32
        r, a = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        z[:, k], z[:, k + 1] = r * np.cos(a), r * np.sin(a)
    return z.reshape(-1)[:n]


def gaussian_noise_ref(img_u8, std, seed, index):
    """clip(img + rint(std z), 0, 255) with z = normal_ref in H, W, C order (rint: ties to even).  The generator is this project's own counter-based one (module
    docstring), not numpy's: the reference's utils.gaussian_noise is unseeded, so no stream exists that the files could be equal to."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8:
        raise ValueError('the image must be uint8, got %s' % img.dtype)
    z = normal_ref(img.size, seed, index).reshape(img.shape)
    return np.clip(img.astype(np.float64) + np.rint(float(std) * z), 0, 255).astype(np.uint8)


# ---- device entry points (csrc/corrupt.hip) ----------------------------------------------------------------------------------------------
def plane_bytes(H, W):
    """bytes of the decoded planes of one H x W image between dasr_jpeg_blocks and dasr_jpeg_merge: Y [ceil8(H)][ceil8(W)], then Cb and Cr [ceil8(ceil(H / 2))][ceil16(W) / 2]"""
    r8 = lambda v: -(-v // 8) * 8
    return r8(H) * r8(W) + 2 * r8(-(-H // 2)) * (-(-W // 16) * 8)


def _images(img, what):
    import torch
    if not torch.is_tensor(img) or img.device.type != 'cuda' or img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3 or 0 in img.shape:
        raise ValueError('%s runs a HIP kernel on a uint8 device tensor [H, W, 3] or [N, H, W, 3]; got %s' % (
            what, '%s %s on %s' % (img.dtype, tuple(img.shape), img.device) if torch.is_tensor(img) else type(img).__name__))
    x = img.contiguous()
    return x, (1 if x.dim() == 3 else x.shape[0]), x.shape[-3], x.shape[-2]


def jpeg_roundtrip(img, quality):
    """jpeg_roundtrip_ref on the device: uint8 [H, W, 3] or [N, H, W, 3] -> a new tensor of that shape.  Two launches on the current stream (dasr_jpeg_blocks,
    dasr_jpeg_merge) around one workspace of plane_bytes(H, W) per image; no host synchronisation."""
    import torch
    from . import _lib
    from .engine import _stream
    quality = check_quality(quality)
    x, N, H, W = _images(img, 'jpeg_roundtrip')
    planes = torch.empty(N * plane_bytes(H, W), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    L = _lib.lib()
    _lib.check(L.dasr_jpeg_blocks(x.data_ptr(), N, H, W, quality, planes.data_ptr(), _stream()), 'dasr_jpeg_blocks')
    _lib.check(L.dasr_jpeg_merge(planes.data_ptr(), N, H, W, out.data_ptr(), _stream()), 'dasr_jpeg_merge')
    return out


def gaussian_noise(img, std, seed, index):
    """gaussian_noise_ref on the device: uint8 [H, W, 3] (image `index`) or [N, H, W, 3] (images index, index + 1, ...) -> a new tensor.  One dasr_noise_u8 launch on
    the current stream; no host synchronisation."""
    import torch
    from . import _lib
    from .engine import _stream
    x, N, H, W = _images(img, 'gaussian_noise')
    std, seed, index = float(std), int(seed) & 0xFFFFFFFFFFFFFFFF, int(index)
    if not std >= 0.0 or std == float('inf'):
        raise ValueError('the standard deviation must be finite and not negative, got %r' % (std,))
    if not 0 <= index or index + N > 1 << 32:
        raise ValueError('the image indices must lie in 0 .. 2^32 - 1, got %d .. %d' % (index, index + N - 1))
    out = torch.empty_like(x)
    _lib.check(_lib.lib().dasr_noise_u8(x.data_ptr(), out.data_ptr(), N, H * W * 3, std, seed - (1 << 64) if seed >> 63 else seed, index, _stream()), 'dasr_noise_u8')
    return out
