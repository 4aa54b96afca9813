"""MATLAB's bicubic imresize of 8-bit images on the device, as the dataset preparation needs it (reference: codes/SRN/scripts/generate_mod_LR_bic.m:50-64, MATLAB only):

    img   = im2double(window)                  byte / 255.0
    im_LR = imresize(img, 1 / s, 'bicubic')    antialiased; written through imwrite: q(x) = min(255, max(0, floor(x * 255 + 0.5)))
    im_B  = imresize(im_LR, s, 'bicubic')      of the DOUBLE image, not of the written file

down_windows_u8 makes im_LR for a list of equally sized windows of one decoded image resident in device memory in ONE launch (csrc/imgio.hip: dasr_windows_down_u8; the
mirror edge is the window's edge, so the LR image of a sub-image is what MATLAB makes of the sub-image file), upsample is imresize(x, s) of planes in one launch
(dasr_imresize_up), to fp32 planes, added onto fp32 planes (backproject.reverse_filter) or quantised to interleaved bytes (im_B).  Nothing is synchronised.
down_windows_fp64 / upsample_fp64 / quantise are the restatements on the host in float64 the tests compare against (data.imresize_matlab per window).
`python -m dasr_amd.prepare_data` runs both on folders of PNG files."""
import torch

from . import _lib
from .engine import _stream
from .imgio import down_table_ptrs, up_tap_table, upload

SCALES = (2, 3, 4)
DOWN_TILE = (8, 32)         # LR outputs per workgroup of windows_down_u8_kernel (DASR_WD_TILE_H / _W of include/dasr_hip.h; tests/test_prepare_data_host.py compares)
UP_TILE = (16, 64)          # output samples per workgroup of imresize_up_kernel (DASR_UP_TILE_H / _W)
UP_F32, UP_F32_ACC, UP_U8 = 0, 1, 2   # DASR_UP_*


def _scale(s):
    if s not in SCALES:
        raise ValueError('the scale must be one of %s, got %r' % (SCALES, s))
    return int(s)


def _windows(shape, origins, size, s):
    """the checked (H, W, [(y0, x0)], hh, ww) of a window list on an image of `shape` [H, W, 3]: ValueError for what the kernel would refuse"""
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError('the image must be uint8 [H, W, 3], got %s' % (tuple(shape),))
    H, W = int(shape[0]), int(shape[1])
    hh, ww = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    origins = [(int(y), int(x)) for y, x in origins]
    if not origins:
        raise ValueError('no windows given')
    if hh <= 0 or ww <= 0 or hh % s or ww % s:
        raise ValueError('the window size %d x %d is not a positive multiple of the scale %d' % (hh, ww, s))
    for y0, x0 in origins:
        if y0 < 0 or x0 < 0 or y0 + hh > H or x0 + ww > W:
            raise ValueError('the %d x %d window at (%d, %d) does not lie inside the %d x %d image' % (hh, ww, y0, x0, H, W))
    return H, W, origins, hh, ww


def down_windows_u8(img_u8_dev, origins, size, s, want_f64=True):
    """the bicubic LR images of windows of one decoded image: img_u8_dev uint8 [H, W, 3] on the device (contiguous), origins [(y0, x0)] the top-left corners, size the
    common window size (an int, or (hh, ww); multiples of s), s in {2, 3, 4}.  Returns (lr_u8 uint8 [n, hh / s, ww / s, 3], lr_f64 float64 [n, 3, hh / s, ww / s] or None
    without want_f64).  One dasr_windows_down_u8 launch on the current stream behind one asynchronous descriptor upload; no host synchronisation."""
    s = _scale(s)
    if not torch.is_tensor(img_u8_dev) or img_u8_dev.device.type != 'cuda' or img_u8_dev.dtype != torch.uint8 or not img_u8_dev.is_contiguous():
        raise ValueError('down_windows_u8 runs a HIP kernel on a contiguous uint8 device image; got %s' % (
            '%s on %s' % (img_u8_dev.dtype, img_u8_dev.device) if torch.is_tensor(img_u8_dev) else type(img_u8_dev).__name__))
    H, W, origins, hh, ww = _windows(img_u8_dev.shape, origins, size, s)
    n, dev = len(origins), img_u8_dev.device
    host = (_lib.WindowDesc * n)(*[_lib.WindowDesc(y0, x0) for y0, x0 in origins])
    block, (off,) = upload(dev, host)
    lr_u8 = torch.empty((n, hh // s, ww // s, 3), dtype=torch.uint8, device=dev)
    lr_f64 = torch.empty((n, 3, hh // s, ww // s), dtype=torch.float64, device=dev) if want_f64 else None
    _lib.check(_lib.lib().dasr_windows_down_u8(img_u8_dev.data_ptr(), H, W, block.data_ptr() + off, host, n, hh, ww, s, *down_table_ptrs(hh, ww, s, dev), lr_u8.data_ptr(),
                                               lr_f64.data_ptr() if want_f64 else None, _stream()), 'dasr_windows_down_u8')
    return lr_u8, lr_f64


def upsample(x, s, out='f32', into=None):
    """MATLAB's imresize(x, s) (bicubic, no antialiasing) of device planes x [N, C, h, w], fp32 or fp64, s in {2, 3, 4}, one dasr_imresize_up launch on the current
    stream.  out 'f32': a new fp32 tensor [N, C, s h, s w] -- or, with `into` (a contiguous fp32 device tensor of that shape), into = (float)((double)into + up(x)) in
    place with one rounding, returned; out 'u8': uint8 [N, s h, s w, C], q(up(x)) interleaved as an image file holds it."""
    s = _scale(s)
    if not torch.is_tensor(x) or x.device.type != 'cuda' or x.dtype not in (torch.float32, torch.float64) or x.dim() != 4:
        raise ValueError('upsample runs a HIP kernel on fp32 or fp64 device planes [N, C, h, w]; got %s' % (
            '%s %s on %s' % (x.dtype, tuple(x.shape), x.device) if torch.is_tensor(x) else type(x).__name__))
    if out not in ('f32', 'u8') or (into is not None and out != 'f32'):
        raise ValueError("upsample: out is 'f32' or 'u8' (`into` with 'f32' only), got %r" % (out,))
    x = x.detach().contiguous()
    N, C, h, w = x.shape
    if into is not None:
        if into.dtype != torch.float32 or into.device != x.device or tuple(into.shape) != (N, C, s * h, s * w) or not into.is_contiguous():
            raise ValueError('upsample: `into` must be a contiguous fp32 tensor %s on %s, got %s %s on %s' % (
                (N, C, s * h, s * w), x.device, into.dtype, tuple(into.shape), into.device))
        dst, mode = into, UP_F32_ACC
    elif out == 'u8':
        dst, mode = torch.empty((N, s * h, s * w, C), dtype=torch.uint8, device=x.device), UP_U8
    else:
        dst, mode = torch.empty((N, C, s * h, s * w), dtype=torch.float32, device=x.device), UP_F32
    tables = [t.data_ptr() for n in (h, w) for t in up_tap_table(n, s, x.device)]
    _lib.check(_lib.lib().dasr_imresize_up(x.data_ptr(), int(x.dtype == torch.float64), N, C, h, w, s, *tables, dst.data_ptr(), mode, _stream()), 'dasr_imresize_up')
    return dst


def quantise(x):
    """q(x) = min(255, max(0, floor(x * 255 + 0.5))) of a float64 tensor, every step in float64: MATLAB's imwrite of a double image (im2uint8); uint8"""
    return torch.floor(x.to(torch.float64) * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8)


def down_windows_fp64(img_u8, origins, size, s):
    """down_windows_u8 on the host in float64: img_u8 uint8 [H, W, 3] (numpy array or CPU tensor).  Per window imresize_matlab(window / 255.0, 1 / s), then q.
    Returns (uint8 [n, hh / s, ww / s, 3], float64 [n, 3, hh / s, ww / s])."""
    from .data import imresize_matlab
    s = _scale(s)
    img = torch.as_tensor(img_u8)
    _, _, origins, hh, ww = _windows(img.shape, origins, size, s)
    f64 = torch.stack([imresize_matlab(img[y0:y0 + hh, x0:x0 + ww].permute(2, 0, 1).to(torch.float64) / 255.0, 1.0 / s) for y0, x0 in origins])
    return quantise(f64).permute(0, 2, 3, 1).contiguous(), f64


def upsample_fp64(x, s):
    """imresize(x, s) of planes [N, C, h, w] (or [C, h, w]) on the host in float64"""
    from .data import imresize_matlab
    s = _scale(s)
    x = x.detach().cpu().to(torch.float64)
    if x.dim() == 3:
        return imresize_matlab(x, float(s))
    N, C, h, w = x.shape
    return imresize_matlab(x.reshape(N * C, h, w), float(s)).reshape(N, C, s * h, s * w)
