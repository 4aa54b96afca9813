"""PNG files from 8-bit images that are resident on the device, without LZ77: the per-row filter, a dynamic-Huffman deflate block per strip of rows and the packing
of the strips into one buffer run on the MI355X (csrc/png.hip); the host adds the container (signature, IHDR, IDAT, IEND), the combined Adler-32 and the chunk CRCs.

The stream of one image (what every inflater reads, PIL bit for bit):
    78 01 | strip 0 | strip 1 | ... | 03 00 | Adler-32
A strip is strip_rows(W) whole rows (the last one of an image may be shorter), at most 65 535 filtered bytes.  Every row is filtered on its own with the type (None, Sub,
Up, Average, Paeth; bpp 3) whose filtered bytes have the smallest sum of min(b, 256 - b), ties to the lowest type; the row above a strip's first row is the row above it in
the image.  A strip is one deflate block, BFINAL 0, BTYPE 10: a Huffman code (lengths <= 15, Huffman-optimal unless the tree is deeper than 15) for the 257 symbols
"byte value" and "end of block", two distance codes of one bit each (what zlib's Z_HUFFMAN_ONLY streams declare), the code lengths written one by one with a
code-length code of at most 7 bits (no run symbols 16-18).  An empty stored block (three zero bits, padding, 00 00 FF FF: zlib's Z_SYNC_FLUSH) byte-aligns the strip, so
strips are coded independently and concatenated.  A strip that would be larger coded than stored is one stored block.  `03 00` is an empty final fixed-Huffman block:
no strip is special.

filter_ref / strip_stats_ref / encode_ref state all of this in numpy and pure Python and need no device (the tests pin the kernels to them: the filtered bytes,
histograms and Adler partials bit for bit; the files by what they inflate and decode to, since two Huffman constructions may break ties differently).
encode_batch / write_batch run it on uint8 device tensors: one descriptor upload, five launches, two read-backs per batch.

`fmt` names what a batch holds: 'rgb' (the default) interleaved RGB [H, W, 3]; 'bgr' interleaved BGR [H, W, 3] as util.tensor2img / metrics.tensor2img_device return it, written as
the RGB file of the channel-reversed image (the filter kernel reads the bytes in file order, nothing is permuted in memory); 'grey' one channel [H, W], colour type 0, one
byte per pixel (rows of 1 + W filtered bytes, W <= 65 534).

FileWriter is the sink every driver hands its images to, one at a time or all products of a file at once.  Device mode: the device stages per call on the current stream,
the container, the CRCs and the file write on its thread pool.  Host mode: save_host (PIL) on the pool or, without threads, on the caller's thread.  Either way a bounded
number of calls is outstanding and close() waits for every file."""
import collections
import heapq
import struct
import time
import zlib

import numpy as np

STRIP_TARGET = 32768        # filtered bytes a strip aims at (a strip fits one stored block: <= 65 535)
MAX_STRIP_BYTES = 65535
MAX_WIDTH = 21844           # (1 + 3 W <= 65 535)
ADLER_MOD = 65521
MAX_BITS, MAX_CL_BITS = 15, 7
N_SYMS = 257                # byte values and end-of-block; no length symbol is ever used
HDR_WORDS = 64              # DASR_PNG_HDR_WORDS
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
SIGNATURE = b'\x89PNG\r\n\x1a\n'
HOST_PATH = "PIL's Image.save"
FORMATS = {'rgb': (0, 3), 'bgr': (1, 3), 'grey': (2, 1)}   # fmt -> (DASR_PNG_RGB / _BGR / _GREY, bytes per pixel)
MAX_WRITER_THREADS = 16
DEVICE_NOTE = '--device_png: the PNG files are encoded on the device (filter, Huffman-only deflate), the host adds the container and the checksums'


def _format(fmt):
    if fmt not in FORMATS:
        raise ValueError("fmt: expected 'rgb', 'bgr' or 'grey', got %r" % (fmt,))
    return FORMATS[fmt]


def max_width(fmt='rgb'):
    """the widest image of a format: a row of 1 + bpp W filtered bytes fits one strip"""
    return (MAX_STRIP_BYTES - 1) // _format(fmt)[1]


def strip_rows(W, fmt='rgb'):
    """rows of a strip of an image W pixels wide"""
    return max(1, STRIP_TARGET // (1 + _format(fmt)[1] * int(W)))


def photo(h, w, seed):
    """the test image: six sinusoids per channel around 128 and Gaussian noise of deviation 2"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.zeros((h, w, 3))
    for c in range(3):
        for k in range(6):
            fy, fx, ph = rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), rng.uniform(0, 6.28)
            a[..., c] += rng.uniform(10, 40) * np.sin(fy * y + fx * x + ph)
    a += 128 + rng.normal(0, 2.0, a.shape)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


# ---- the filter ----------------------------------------------------------------------------------------------------------------------
def _check_image(img, fmt='rgb'):
    img = np.asarray(img)
    bpp = _format(fmt)[1]
    if img.dtype != np.uint8 or img.ndim != (3 if bpp == 3 else 2) or (bpp == 3 and img.shape[2] != 3) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError('the image must be uint8 %s, got %s %s' % ('[H, W, 3]' if bpp == 3 else '[H, W]', img.dtype, img.shape))
    if img.shape[1] > max_width(fmt):
        raise ValueError('an image %d pixels wide has rows above %d filtered bytes (W > %d): encode it on the host (%s)' % (img.shape[1], MAX_STRIP_BYTES, max_width(fmt), HOST_PATH))
    return img


def filter_ref(img, fmt='rgb'):
    """uint8 [H, W, 3] ('grey': [H, W]) -> uint8 [H, 1 + bpp W]: the filter type of every row and its filtered bytes (its bytes in C order are the stream that is deflated).
    'bgr': the rows of the channel-reversed image"""
    img = _check_image(img, fmt)
    if fmt == 'bgr':
        img = img[:, :, ::-1]
    H, W = img.shape[:2]
    bpp = _format(fmt)[1]
    x = img.reshape(H, bpp * W).astype(np.int32)
    a = np.concatenate([np.zeros((H, bpp), np.int32), x[:, :-bpp]], axis=1)      # left
    b = np.concatenate([np.zeros((1, bpp * W), np.int32), x[:-1]], axis=0)       # up: zeros above the first row
    c = np.concatenate([np.zeros((H, bpp), np.int32), b[:, :-bpp]], axis=1)      # up-left
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255      # [5, H, bpp W]
    cost = np.minimum(cand, 256 - cand).sum(axis=2)                              # [5, H]
    types = np.argmin(cost, axis=0)                                              # (the first minimum: the lowest type)
    out = np.empty((H, 1 + bpp * W), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(H)]
    return out


def strip_stats_ref(filtered, fmt='rgb'):
    """filtered uint8 [H, 1 + bpp W] -> (histograms uint32 [n_strips, 257] with end-of-block = 1, Adler partials uint32 [n_strips, 2]): per strip of n bytes b_0 .. b_(n-1),
    s1 = sum b_i mod 65521 and s2 = sum (n - i) b_i mod 65521 (Adler-32 run from s1 = s2 = 0)"""
    H, stride = filtered.shape
    rows = strip_rows((stride - 1) // _format(fmt)[1], fmt)
    hist, adler = [], []
    for r0 in range(0, H, rows):
        b = filtered[r0:r0 + rows].reshape(-1).astype(np.int64)
        hist.append(np.concatenate([np.bincount(b, minlength=256), [1]]))
        adler.append((int(b.sum()) % ADLER_MOD, int((np.arange(b.size, 0, -1) * b).sum()) % ADLER_MOD))
    return np.array(hist, dtype=np.uint32), np.array(adler, dtype=np.uint32)


def adler_combine(partials, lengths):
    """the Adler-32 of the concatenated strips from their partial pairs: s2 += n s1 + B, s1 += A, from (1, 0)"""
    A, B, n = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (np.asarray(partials)[:, 0], np.asarray(partials)[:, 1], lengths))
    s1_before = 1 + np.concatenate([[0], np.cumsum(A)[:-1]])
    s1 = (1 + int(A.sum())) % ADLER_MOD
    s2 = int(((n * (s1_before % ADLER_MOD)) % ADLER_MOD + B).sum()) % ADLER_MOD
    return (s2 << 16) | s1


# ---- Huffman codes ---------------------------------------------------------------------------------------------------------------------
def huffman_lengths(freq, max_bits):
    """code lengths [len(freq)] of a complete prefix code for the symbols with freq > 0: a heapq Huffman tree; where it is deeper than max_bits the counts per length are
    repaired (one code taken from the longest length, one moved a level down, until the Kraft sum is 1) and handed out again by frequency.  Fewer than two used symbols:
    two codes of one bit, as zlib pads a tree."""
    freq = [int(f) for f in freq]
    used = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    lens = [0] * len(freq)
    if len(used) < 2:
        s = used[0][1] if used else 0
        lens[s] = lens[1 if s == 0 else 0] = 1
        return lens
    heap = [(f, k, None) for k, (f, s) in enumerate(used)]          # (weight, tie: leaves before internal nodes, children)
    heapq.heapify(heap)
    tie = len(used)
    while len(heap) > 1:
        x, y = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (x[0] + y[0], tie, (x, y)))
        tie += 1
    num = [0] * (max_bits + 1)
    stack = [(heap[0], 0)]
    while stack:
        (w, k, kids), d = stack.pop()
        if kids is None:
            num[min(d, max_bits)] += 1
        else:
            stack += [(kids[0], d + 1), (kids[1], d + 1)]
    total = sum(num[i] << (max_bits - i) for i in range(1, max_bits + 1))
    while total != 1 << max_bits:
        num[max_bits] -= 1
        for i in range(max_bits - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
    j = len(used)
    for i in range(1, max_bits + 1):                                # the most frequent symbols get the shortest codes
        for _ in range(num[i]):
            j -= 1
            lens[used[j][1]] = i
    return lens


def canonical_codes(lens):
    """RFC 1951 section 3.2.2: codes of one length are consecutive in symbol order, shorter codes precede longer ones"""
    count = [0] * (max(lens) + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * len(count), 0
    for bits in range(1, len(count)):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def _rev(code, n):
    return int(format(code, '0%db' % n)[::-1], 2) if n else 0


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, 'little')


def block_header(lens):
    """the bits of a dynamic block up to its first symbol (BFINAL 0, BTYPE 10, HLIT, HDIST, HCLEN, the code-length code, the 257 + 2 code lengths) as (_Bits, HCLEN)"""
    seq = list(lens) + [1, 1]
    clfreq = [0] * 19
    for l in seq:
        clfreq[l] += 1
    cllens = huffman_lengths(clfreq, MAX_CL_BITS)
    clcodes = canonical_codes(cllens)
    ncl = max(4, max(k + 1 for k, s in enumerate(CL_ORDER) if cllens[s]))
    w = _Bits()
    w.put(0, 1)
    w.put(2, 2)
    w.put(len(lens) - 257, 5)
    w.put(1, 5)
    w.put(ncl - 4, 4)
    for s in CL_ORDER[:ncl]:
        w.put(cllens[s], 3)
    for l in seq:
        w.put(_rev(clcodes[l], cllens[l]), cllens[l])
    return w, ncl - 4


def deflate_strip_ref(b):
    """the bytes of one strip: b uint8 [n], 1 <= n <= 65 535"""
    b = np.asarray(b, dtype=np.uint8).reshape(-1)
    n = b.size
    hist = np.concatenate([np.bincount(b, minlength=256), [1]])
    lens = huffman_lengths(hist, MAX_BITS)
    codes = canonical_codes(lens)
    w, _ = block_header(lens)
    body = int((hist * np.array(lens)).sum())
    if (w.n + body + 3 + 7) // 8 + 4 > n + 5:
        return b'\x00' + struct.pack('<HH', n, n ^ 0xFFFF) + b.tobytes()
    L = np.array(lens, dtype=np.int64)
    R = np.array([_rev(c, l) for c, l in zip(codes, lens)], dtype=np.int64)
    sym = np.concatenate([b.astype(np.int64), [256]])
    bits = ((R[sym][:, None] >> np.arange(MAX_BITS)) & 1).astype(np.uint8)
    keep = np.arange(MAX_BITS)[None, :] < L[sym][:, None]
    stream = np.concatenate([np.unpackbits(np.frombuffer(w.bytes(), np.uint8), bitorder='little')[:w.n], bits[keep], np.zeros(3, np.uint8)])
    return np.packbits(stream, bitorder='little').tobytes() + b'\x00\x00\xff\xff'


# ---- the container ---------------------------------------------------------------------------------------------------------------------
def _chunk_parts(kind, parts):
    """[length, type, data parts ..., CRC] of one chunk"""
    crc = zlib.crc32(kind)
    for p in parts:
        crc = zlib.crc32(p, crc)
    return [struct.pack('>I', sum(len(p) for p in parts)), kind] + list(parts) + [struct.pack('>I', crc)]


def file_parts(H, W, strips, adler, fmt='rgb'):
    """the pieces of the PNG file of an H x W image whose packed strips are `strips` (bytes-like) and whose combined Adler-32 is `adler`: colour type 2 (RGB), for 'grey' 0"""
    ihdr = struct.pack('>IIBBBBB', W, H, 8, 2 if _format(fmt)[1] == 3 else 0, 0, 0, 0)
    return [SIGNATURE] + _chunk_parts(b'IHDR', [ihdr]) + _chunk_parts(b'IDAT', [b'\x78\x01', strips, b'\x03\x00', struct.pack('>I', adler)]) + _chunk_parts(b'IEND', [])


def encode_ref(img, fmt='rgb'):
    """uint8 [H, W, 3] ('grey': [H, W]) -> the bytes of its PNG file, on the host"""
    f = filter_ref(img, fmt)
    H, W = f.shape[0], (f.shape[1] - 1) // _format(fmt)[1]
    rows = strip_rows(W, fmt)
    strips = [f[r0:r0 + rows].reshape(-1) for r0 in range(0, H, rows)]
    _, adler = strip_stats_ref(f, fmt)
    return b''.join(file_parts(H, W, b''.join(deflate_strip_ref(s) for s in strips), adler_combine(adler, [s.size for s in strips]), fmt))


# ---- the device path (csrc/png.hip) ------------------------------------------------------------------------------------------------------
IMAGE_DESC = np.dtype([('src', '<u8'), ('pitch', '<i8'), ('H', '<i4'), ('W', '<i4'), ('first_strip', '<i4'), ('n_strips', '<i4')])   # dasr_png_image
STRIP_DESC = np.dtype([('image', '<i4'), ('row0', '<i4'), ('rows', '<i4'), ('n', '<i4'), ('filt_off', '<i8'), ('slot_off', '<i8')])  # dasr_png_strip


def _check_grey_tensor(k, t):
    import torch
    what = 'images[%d]' % k
    if not torch.is_tensor(t):
        raise ValueError('%s: expected a uint8 device tensor [H, W], got %s' % (what, type(t).__name__))
    if t.device.type != 'cuda' or t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError('%s: expected a uint8 device tensor [H, W] (8-bit grey), got %s %s on %s' % (what, t.dtype, tuple(t.shape), t.device))
    H, W = int(t.shape[0]), int(t.shape[1])
    if (W > 1 and t.stride(1) != 1) or (H > 1 and t.stride(0) < W):   # (the stride of a dimension of size 1 says nothing)
        raise ValueError('%s: pixels must be consecutive bytes (stride(1) == 1, rows that do not overlap), got strides %s' % (what, tuple(t.stride())))
    if W > max_width('grey'):
        raise ValueError('%s: %d pixels wide, rows above %d filtered bytes (W > %d): encode it on the host (%s)' % (what, W, MAX_STRIP_BYTES, max_width('grey'), HOST_PATH))
    return H, W


def _check_tensor(k, t, fmt='rgb'):
    import torch
    if _format(fmt)[1] == 1:
        return _check_grey_tensor(k, t)
    what, order = 'images[%d]' % k, fmt.upper()
    if not torch.is_tensor(t):
        raise ValueError('%s: expected a uint8 device tensor [H, W, 3], got %s' % (what, type(t).__name__))
    if t.device.type != 'cuda' or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError('%s: expected a uint8 device tensor [H, W, 3] (8-bit %s), got %s %s on %s' % (what, order, t.dtype, tuple(t.shape), t.device))
    H, W = int(t.shape[0]), int(t.shape[1])
    if t.stride(2) != 1 or t.stride(1) != 3 or (H > 1 and t.stride(0) < 3 * W):
        raise ValueError('%s: pixels must be interleaved %s bytes (stride(1) == 3, stride(2) == 1, rows that do not overlap), got strides %s' % (what, order, tuple(t.stride())))
    if W > MAX_WIDTH:
        raise ValueError('%s: %d pixels wide, rows above %d filtered bytes (W > %d): encode it on the host (%s)' % (what, W, MAX_STRIP_BYTES, MAX_WIDTH, HOST_PATH))
    return H, W


class Plan:
    """the descriptors of one batch: host arrays, their one upload, and the sizes of the work buffers"""

    def __init__(self, images, fmt='rgb'):
        import torch
        self.fmt = fmt
        self.fmt_code, bpp = _format(fmt)
        sizes = [_check_tensor(k, t, fmt) for k, t in enumerate(images)]
        if any(t.device != images[0].device for t in images):
            raise ValueError('images: all tensors of a batch must be on one device')
        self.device = images[0].device
        self.sizes = sizes
        strips, self.images = [], np.zeros(len(images), IMAGE_DESC)
        filt_off = slot_off = 0
        for k, (t, (H, W)) in enumerate(zip(images, sizes)):
            rows, stride = strip_rows(W, fmt), 1 + bpp * W
            first = len(strips)
            for r0 in range(0, H, rows):
                r = min(rows, H - r0)
                strips.append((k, r0, r, r * stride, filt_off, slot_off))
                filt_off += -(-r * stride // 16) * 16
                slot_off += -(-(r * stride + 16) // 4) * 4
            self.images[k] = (t.data_ptr(), t.stride(0) if H > 1 else bpp * W, H, W, first, len(strips) - first)
        self.strips = np.array(strips, dtype=STRIP_DESC)
        self.filt_bytes, self.slot_bytes = filt_off, slot_off
        blob = np.concatenate([self.images.view(np.uint8), self.strips.view(np.uint8)])
        self.dev = torch.from_numpy(blob).to(self.device)                       # the one descriptor upload of the batch
        self.images_dev, self.strips_dev = self.dev.data_ptr(), self.dev.data_ptr() + self.images.nbytes
        self.n_images, self.n_strips = len(images), len(strips)

    def host(self):
        return self.images.ctypes.data, self.strips.ctypes.data


def filter_batch(images, plan=None, fmt='rgb'):
    """stage 1 (dasr_png_filter_fmt; `fmt` of a given plan is the plan's) on the current stream -> (plan, filtered bytes uint8 [plan.filt_bytes]: strip s at plan.strips['filt_off'][s], histograms uint32
    [n_strips, 257], meta).  meta is the int64 buffer of the batch's first read-back: status, total bytes, n_images + 1 offsets, then the Adler partials as uint32 pairs."""
    import torch
    from . import _lib
    from .engine import _stream
    plan = plan or Plan(images, fmt)
    dev = plan.device
    filt = torch.empty(plan.filt_bytes, dtype=torch.uint8, device=dev)
    hist = torch.empty((plan.n_strips, N_SYMS), dtype=torch.int32, device=dev)
    meta = torch.zeros(plan.n_images + 3 + plan.n_strips, dtype=torch.int64, device=dev)
    ih, sh = plan.host()
    _lib.check(_lib.lib().dasr_png_filter_fmt(plan.images_dev, ih, plan.n_images, plan.strips_dev, sh, plan.n_strips, filt.data_ptr(), plan.filt_bytes, hist.data_ptr(),
                                              meta.data_ptr() + 8 * (plan.n_images + 3), plan.fmt_code, _stream()), 'dasr_png_filter_fmt')
    return plan, filt, hist, meta


def codes_batch(hist):
    """stage 2 (dasr_png_codes) on the current stream: hist int32 / uint32 device tensor [n, 257] -> (lengths uint8 [n, 257], canonical codes int16 [n, 257], block
    headers int32 [n, 64]: bits, bits of the coded symbols, HLIT | HDIST << 8 | HCLEN << 16, 0, then the header's bits LSB first)"""
    import torch
    from . import _lib
    from .engine import _stream
    if not torch.is_tensor(hist) or hist.device.type != 'cuda' or hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[1] != N_SYMS or not hist.is_contiguous():
        raise ValueError('hist: expected a contiguous int32 device tensor [n, %d]' % N_SYMS)
    n = hist.shape[0]
    lens = torch.empty((n, N_SYMS), dtype=torch.uint8, device=hist.device)
    codes = torch.empty((n, N_SYMS), dtype=torch.int16, device=hist.device)
    hdr = torch.empty((n, HDR_WORDS), dtype=torch.int32, device=hist.device)
    _lib.check(_lib.lib().dasr_png_codes(hist.data_ptr(), n, lens.data_ptr(), codes.data_ptr(), hdr.data_ptr(), _stream()), 'dasr_png_codes')
    return lens, codes, hdr


def _encode_device(images, times=None, fmt='rgb'):
    """stages 1-4 and the two read-backs -> (plan, meta int64 host array, packed bytes uint8 host array).  `times`: a dict that receives the seconds of 'plan' (the tables
    and their upload), 'kernels', 'readback_meta' and 'readback_bytes'; the stream is then synchronised in between, which an ordinary call does not do."""
    import torch
    from . import _lib
    from .engine import _stream
    from .imgio import tick
    L = _lib.lib()
    t0 = time.perf_counter()
    plan = Plan(images, fmt)
    t0 = tick(times, 'plan', t0, True)
    plan, filt, hist, meta = filter_batch(images, plan)
    lens, codes, hdr = codes_batch(hist)
    dev = plan.device
    slots = torch.empty(plan.slot_bytes, dtype=torch.uint8, device=dev)
    sizes = torch.empty(plan.n_strips, dtype=torch.int32, device=dev)
    ws = torch.empty(plan.n_strips, dtype=torch.int64, device=dev)
    out = torch.empty(plan.slot_bytes, dtype=torch.uint8, device=dev)
    ih, sh = plan.host()
    _lib.check(L.dasr_png_emit(plan.strips_dev, sh, plan.n_strips, filt.data_ptr(), plan.filt_bytes, lens.data_ptr(), codes.data_ptr(), hdr.data_ptr(), slots.data_ptr(),
                               plan.slot_bytes, sizes.data_ptr(), meta.data_ptr(), _stream()), 'dasr_png_emit')
    _lib.check(L.dasr_png_pack_fmt(plan.images_dev, ih, plan.n_images, plan.strips_dev, sh, plan.n_strips, sizes.data_ptr(), slots.data_ptr(), plan.slot_bytes, ws.data_ptr(),
                                   out.data_ptr(), plan.slot_bytes, meta.data_ptr(), plan.fmt_code, _stream()), 'dasr_png_pack_fmt')
    t0 = tick(times, 'kernels', t0, True)
    m = meta.cpu().numpy()                                                       # read-back 1: status, sizes and offsets, Adler partials
    if m[0] != 0:
        raise _lib.DasrHipError('the device PNG encoder reported status %d: a strip did not fit its slot' % m[0])
    t0 = tick(times, 'readback_meta', t0, True)
    packed = out[:int(m[1])].cpu().numpy()                                       # read-back 2: the bytes
    tick(times, 'readback_bytes', t0, True)
    return plan, m, packed


def _assemble(plan, m, packed, k):
    """the pieces of file k"""
    H, W = plan.sizes[k]
    first, cnt = int(plan.images['first_strip'][k]), int(plan.images['n_strips'][k])
    adler = m[plan.n_images + 3:].view(np.uint32).reshape(-1, 2)[first:first + cnt]
    return file_parts(H, W, memoryview(packed[int(m[2 + k]):int(m[3 + k])]), adler_combine(adler, plan.strips['n'][first:first + cnt]), plan.fmt)


def encode_batch(images, times=None, fmt='rgb'):
    """uint8 device tensors [H, W, 3] (views with any row stride; stride(1) == 3 and stride(2) == 1; 'grey': [H, W], stride(1) == 1) -> the bytes of their PNG files.  Stages 1-4 run on the current
    stream for the whole batch; the container, the Adler-32 and the chunk CRCs are made on the host.  `times`: see _encode_device."""
    images = list(images)
    if not images:
        return []
    plan, m, packed = _encode_device(images, times, fmt)
    return [b''.join(_assemble(plan, m, packed, k)) for k in range(len(images))]


def _write(plan, m, packed, k, path):
    with open(path, 'wb') as f:
        f.writelines(_assemble(plan, m, packed, k))
    return path


def write_batch(images, paths, pool, times=None, fmt='rgb'):
    """encode_batch straight into files: returns one future per image (its result is the path); the container, the CRCs (zlib.crc32 releases the GIL) and the write of
    every file run on `pool`"""
    images, paths = list(images), list(paths)
    if len(images) != len(paths):
        raise ValueError('paths: %d paths for %d images' % (len(paths), len(images)))
    if not images:
        return []
    plan, m, packed = _encode_device(images, times, fmt)
    return [pool.submit(_write, plan, m, packed, k, p) for k, p in enumerate(paths)]


def save_host(array, path, fmt='rgb', compress_level=6):
    """THE host saver: uint8 [H, W, 3] ('grey': [H, W]) -> a PNG file at `path`, whatever its extension, through PIL at zlib level `compress_level` (6 is PIL's default; the
    pixels do not depend on it).  'bgr': the RGB file of the channel-reversed image, as encode_batch writes it.  Returns the path."""
    from PIL import Image
    array = np.asarray(array)
    if array.dtype != np.uint8 or array.ndim != (3 if _format(fmt)[1] == 3 else 2):
        raise ValueError("the image must be uint8 %s for fmt %r, got %s %s" % ('[H, W, 3]' if fmt != 'grey' else '[H, W]', fmt, array.dtype, array.shape))
    array = np.ascontiguousarray(array[:, :, ::-1] if fmt == 'bgr' else array)   # (a slice of a larger image is copied here, on the thread that encodes it)
    Image.fromarray(array).save(path, 'PNG', compress_level=compress_level)
    return path


class FileWriter:
    """the sink every driver hands its 8-bit images to: `with FileWriter(device, threads) as w: w.write(image, path, fmt)`.
    device=True: `image` is a uint8 device tensor; a call is ONE write_batch on the current stream and returns once its two read-backs are done (until then the call holds
    the tensors; afterwards the caller may reuse them); the container, the CRCs and the file write run on the writer's own pool of at most 16 threads.
    device=False: `image` is a host uint8 array, or a device tensor that is read back here, on the caller's thread; every image is one save_host job at `compress_level` on
    the pool -- with threads=0 on the caller's thread, before write() returns.
    At most `max_pending` (default 2 x threads) CALLS are outstanding: beyond that a call waits for the oldest.  close() (or leaving the block) waits for all of them and
    raises the first failure, so a driver cannot return before its files are complete.  `paths`: every path handed over, in submission order.  `waited`: the seconds the
    caller has spent waiting for the pool.  `times`: a dict the caller may set (per file, say) that receives the seconds of the hand-over ('device_png': the batch's tables,
    launches and read-backs; 'submit' in host mode) and 'encode_wait'.  `note`: printed once by a device-mode writer (None: the driver logs its own line)."""

    def __init__(self, device, threads=4, max_pending=None, compress_level=6, note=DEVICE_NOTE, save=save_host):
        from concurrent.futures import ThreadPoolExecutor
        self.device = bool(device)
        self.threads = 0 if int(threads) <= 0 and not self.device else max(1, min(int(threads), MAX_WRITER_THREADS))
        self.max_pending = 2 * self.threads if max_pending is None else int(max_pending)
        self.compress_level, self._save = compress_level, save
        self._pool = ThreadPoolExecutor(max_workers=self.threads) if self.threads else None
        self._pending = collections.deque()                         # the futures of one call each
        self._error, self._closed = None, False
        self.paths, self.waited, self.times = [], 0.0, None
        if self.device and note:
            print(note)

    def _add(self, key, seconds):
        if self.times is not None:
            self.times[key] = self.times.get(key, 0.0) + seconds
        return seconds

    def _wait_until(self, keep):
        while len(self._pending) > keep:
            t0 = time.perf_counter()
            for fut in self._pending.popleft():
                try:
                    fut.result()
                except Exception as e:
                    if self._error is None:
                        self._error = e
            self.waited += self._add('encode_wait', time.perf_counter() - t0)

    def write_many(self, images, paths, fmt='rgb'):
        if self._closed:
            raise ValueError('FileWriter.write after close()')
        images, paths = list(images), list(paths)
        if len(images) != len(paths):
            raise ValueError('paths: %d paths for %d images' % (len(paths), len(images)))
        t0, jobs = time.perf_counter(), []
        if self.device:
            jobs = write_batch(images, paths, self._pool, fmt=fmt)
        else:
            for a, p in zip(images, paths):
                a = a.cpu().numpy() if hasattr(a, 'cpu') else a
                if self._pool is None:
                    self._save(a, p, fmt, self.compress_level)
                else:
                    jobs.append(self._pool.submit(self._save, a, p, fmt, self.compress_level))
        self.paths += paths
        self._add('device_png' if self.device else 'submit', time.perf_counter() - t0)
        if jobs:
            self._pending.append(jobs)
            self._wait_until(self.max_pending)

    def write(self, image, path, fmt='rgb'):
        self.write_many([image], [path], fmt)

    def close(self):
        if self._closed:
            return
        self._closed = True
        self._wait_until(0)
        if self._pool is not None:
            self._pool.shutdown(wait=True)
        if self._error is not None:
            raise self._error

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
            return False
        try:                                                        # the block failed: finish what was handed over, its own failure is the one that is raised
            self.close()
        except Exception:
            pass
        return False


def DeviceWriter(threads=4):
    """FileWriter in device mode without the note: what the option-file drivers and the tests of the device path construct"""
    return FileWriter(True, threads, note=None)
