"""Device-side image quality of the SRN validation / evaluation drivers (opt-in: top-level option `device_metrics: true`).

What `test.evaluate` / `train.validate` otherwise do on the host with numpy (train.sr_and_scores: util.tensor2img, then util.host_scores;
reference codes/SRN/utils/util.py:180-204, :236-291, data/util.py:169-190) runs here on csrc/metrics.hip: the fp32 SR / HR images the trainer holds
after test() are quantised to uint8 on the device, the squared-error sums (integer for RGB, fp64 for Y) and the fp64 SSIM means are formed there,
and ONE small read-back per call brings them to the host, where PSNR is formed in double with util.calculate_psnr's formula.  Numerics: DESIGN.md.

Also the numbers of the folder evaluator (dasr_amd/dsn_evaluate.py; reference codes/DSN/evaluate.py:44-46, scikit-image's compare_psnr / compare_ssim) on two
uint8 device images: pair_metrics_u8, with its own kernels for the 7 x 7 box SSIM and the channel sums.
"""
import logging
import math

import torch

from . import _lib, imgio, util
from .engine import _stream

SSIM_WINDOW = 11
_bufs = {}


def _as_batch(t):
    """fp32 contiguous [N, C, H, W] view of a 4-D batch, a 3-D image or a 2-D plane"""
    if t.dim() == 2:
        t = t[None, None]
    elif t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[1] not in (1, 3):
        raise TypeError('expected [N, 3|1, H, W], [3|1, H, W] or [H, W], got shape %s' % (tuple(t.shape),))
    return t.detach().float().contiguous()


def tensor2img_device(t, min_max=(0, 1)):
    """util.tensor2img on the device: [1, 3|1, H, W] / [3|1, H, W] / [H, W] fp32 device tensor -> uint8 device tensor, HWC BGR for 3 channels, HW for one,
    byte for byte what the host function returns.  (A batch of several images is the host function's make_grid case and stays there.)"""
    t = t.squeeze()
    if t.dim() not in (2, 3):
        raise TypeError('tensor2img_device takes one image (3D or 2D after squeeze()); the make_grid case of a batch stays on util.tensor2img. '
                        'Received dimension: {:d}'.format(t.dim()))
    x = _as_batch(t)
    n, c, h, w = x.shape
    out = torch.empty((h, w, c) if c == 3 else (h, w), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().dasr_tensor2img_u8(x.data_ptr(), n, c, h, w, float(min_max[0]), float(min_max[1]), out.data_ptr(), None, None, _stream()),
               'dasr_tensor2img_u8')
    return out


def _buffers(shape, crop, device):
    """per (shape, crop, device): the two planar uint8 images, the partial-sum workspace and the result words.
    res (int64 words): [0, N) integer squared-error sums, [N, 2N) fp64 Y squared-error sums, [2N, 3N) SSIM, [3N, 4N) SSIM_Y, word 4N: the two int32 NaN counts (SR, HR)"""
    key = (tuple(shape), crop, str(device))
    b = _bufs.get(key)
    if b is None:
        n, c, h, w = shape
        ws_bytes = _lib.lib().dasr_img_ws_bytes(n, c, h, w, crop)
        if ws_bytes < 0:
            raise _lib.DasrHipError('dasr_img_ws_bytes refuses N %d C %d H %d W %d crop %d' % (n, c, h, w, crop))
        b = (torch.empty(shape, dtype=torch.uint8, device=device), torch.empty(shape, dtype=torch.uint8, device=device),
             torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=device), torch.zeros(4 * n + 1, dtype=torch.int64, device=device))
        _bufs[key] = b
    return b


def _psnr(sse, count):
    """util.calculate_psnr from the sum of squared differences"""
    mse = float(sse) / count
    if mse == 0:
        return float('inf')
    return 20 * math.log10(255.0 / math.sqrt(mse))


def _host_metrics(sr, hr, crop, ssim, y, min_max):
    """the drivers' host sequence (util.host_scores), image by image: where the device SSIM has no valid region the host function decides what happens"""
    out = {}
    for i in range(sr.shape[0]):
        for k, v in util.host_scores(util.tensor2img(sr[i], min_max=min_max), util.tensor2img(hr[i], min_max=min_max), crop, ssim, y).items():
            out.setdefault(k, []).append(v)
    return out


def batch_metrics(sr, hr, crop, ssim=True, y=True, min_max=(0, 1)):
    """dict of lists (one entry per image of the batch) of Python floats: 'psnr', 'ssim' (if `ssim`), and for 3 channels 'psnr_y' (if `y`) and
    'ssim_y' (if both), of the uint8 images tensor2img makes of `sr` and `hr`, each cropped by `crop` pixels per side.  One device -> host
    synchronisation.  A cropped side under 11 pixels with `ssim`: the host functions are used for the whole call."""
    sr, hr = _as_batch(sr), _as_batch(hr)
    if sr.shape != hr.shape:
        raise ValueError('SR %s and HR %s must have the same shape' % (tuple(sr.shape), tuple(hr.shape)))
    n, c, h, w = sr.shape
    crop = int(crop)
    ch, cw = h - 2 * crop, w - 2 * crop
    if crop < 0 or ch < 1 or cw < 1:
        raise ValueError('crop %d leaves nothing of a %d x %d image' % (crop, h, w))
    if ssim and (ch < SSIM_WINDOW or cw < SSIM_WINDOW):
        return _host_metrics(sr, hr, crop, ssim, y, min_max)
    if not (sr.is_cuda and hr.is_cuda and sr.device == hr.device):
        raise _lib.DasrHipError('batch_metrics needs both images on one GPU (the host path is dasr_amd.util)')
    L, st = _lib.lib(), _stream()
    y = bool(y) and c == 3
    with torch.cuda.device(sr.device):
        pa, pb, ws, res = _buffers(sr.shape, crop, sr.device)
        r0, ws_bytes = res.data_ptr(), ws.numel() * 8
        lo, hi = float(min_max[0]), float(min_max[1])
        _lib.check(L.dasr_tensor2img_u8(sr.data_ptr(), n, c, h, w, lo, hi, None, pa.data_ptr(), r0 + 32 * n, st), 'dasr_tensor2img_u8')
        _lib.check(L.dasr_tensor2img_u8(hr.data_ptr(), n, c, h, w, lo, hi, None, pb.data_ptr(), r0 + 32 * n + 4, st), 'dasr_tensor2img_u8')
        _lib.check(L.dasr_img_sse(pa.data_ptr(), pb.data_ptr(), n, c, h, w, crop, r0, (r0 + 8 * n) if y else None, ws.data_ptr(), ws_bytes, st), 'dasr_img_sse')
        if ssim:
            _lib.check(L.dasr_img_ssim(pa.data_ptr(), pb.data_ptr(), n, c, h, w, crop, 0, r0 + 16 * n, ws.data_ptr(), ws_bytes, st), 'dasr_img_ssim')
            if y:
                _lib.check(L.dasr_img_ssim(pa.data_ptr(), pb.data_ptr(), n, c, h, w, crop, 1, r0 + 24 * n, ws.data_ptr(), ws_bytes, st), 'dasr_img_ssim')
        host = res.cpu()   # the one synchronisation
    f64 = host.view(torch.float64)
    nan_sr, nan_hr = host[4 * n:].view(torch.int32).tolist()
    if nan_sr or nan_hr:
        logging.getLogger('base').warning('image metrics: %d NaN in the SR image(s), %d in the HR image(s) (quantised to 0)' % (nan_sr, nan_hr))
    out = {'psnr': [_psnr(v, c * ch * cw) for v in host[:n].tolist()]}
    if ssim:
        out['ssim'] = f64[2 * n:3 * n].tolist()
    if y:
        out['psnr_y'] = [_psnr(v, ch * cw) for v in f64[n:2 * n].tolist()]
        if ssim:
            out['ssim_y'] = f64[3 * n:4 * n].tolist()
    return out


# ---- the folder evaluator's numbers (codes/DSN/evaluate.py:44-46; CLI: dasr_amd/dsn_evaluate.py) ------------------------------------------------------------
BOX_WINDOW = 7


def psnr_from_sse(sse, count):
    """skimage's compare_psnr of two uint8 images from the integer sum of their squared differences over `count` samples: 10 log10(255^2 / mse)"""
    if sse == 0:
        return float('inf')
    return 10.0 * math.log10(255.0 ** 2 / (float(sse) / count))


def psnr_col_from_sums(sums_a, sums_b, pixels):
    """compare_psnr(img.mean(1).mean(0) / 255., gt.mean(1).mean(0) / 255.) from the integer channel sums: float vectors in [0, 1] have data range 1, so
    10 log10(1 / mse) with mse the mean over the channels of the squared difference of the mean colours"""
    mse = sum((sa / pixels / 255.0 - sb / pixels / 255.0) ** 2 for sa, sb in zip(sums_a, sums_b)) / len(sums_a)
    if mse == 0:
        return float('inf')
    return 10.0 * math.log10(1.0 / mse)


def u8_planes(hwc):
    """decoded bytes on the device, uint8 [H, W, 3] -> (fp32 planar [3, H, W] = byte / 255 correctly rounded, uint8 planar [3, H, W]), both by kernels:
    dasr_u8_to_planar (imgio.planar_f32), then dasr_tensor2img_u8 on its output (rint(float32(u / 255) * 255) == u for all 256 bytes, tests/test_evaluate_host.py)"""
    if hwc.dtype != torch.uint8 or hwc.dim() != 3 or hwc.shape[2] != 3 or not hwc.is_cuda:
        raise TypeError('expected a uint8 [H, W, 3] device tensor, got %s %s on %s' % (hwc.dtype, tuple(hwc.shape), hwc.device))
    h, w = hwc.shape[:2]
    with torch.cuda.device(hwc.device):
        f = imgio.planar_f32(hwc.contiguous())
        u = torch.empty((3, h, w), dtype=torch.uint8, device=hwc.device)
        _lib.check(_lib.lib().dasr_tensor2img_u8(f.data_ptr(), 1, 3, h, w, 0.0, 1.0, None, u.data_ptr(), None, _stream()), 'dasr_tensor2img_u8')
    return f, u


def pair_metrics_u8(a, b, border=0, lpips=None):
    """{'psnr', 'psnr_col', 'ssim'} (Python floats) of two planar uint8 device images [3|1, H, W] with `border` pixels removed from every side, as
    codes/DSN/evaluate.py forms them with scikit-image: PSNR of the bytes, PSNR of the mean colours, SSIM with the 7 x 7 uniform window and the sample
    covariance.  The squared-error sum, the channel sums and the SSIM mean are formed on the device (dasr_img_sse, dasr_img_channel_sums, dasr_img_ssim_box);
    ONE read-back brings the result words to the host, where the two PSNRs are formed in double.  `lpips`: a device scalar (LPIPSAlexHIP.distance) that
    rides in the same read-back and is returned as 'lpips'.  A region under 7 x 7: ValueError."""
    if a.dim() == 4 and a.shape[0] == 1:
        a = a[0]
    if b.dim() == 4 and b.shape[0] == 1:
        b = b[0]
    if a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.dim() != 3 or a.shape[0] not in (1, 3) or a.shape != b.shape:
        raise TypeError('expected two uint8 [3|1, H, W] images of one shape, got %s %s / %s %s' % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    c, h, w = a.shape
    border = int(border)
    ch, cw = h - 2 * border, w - 2 * border
    if border < 0 or ch < BOX_WINDOW or cw < BOX_WINDOW:
        raise ValueError('border %d leaves %d x %d of a %d x %d image: under the %d x %d window of the SSIM' % (border, ch, cw, h, w, BOX_WINDOW, BOX_WINDOW))
    if not (a.is_cuda and b.is_cuda and a.device == b.device):
        raise _lib.DasrHipError('pair_metrics_u8 needs both images on one GPU')
    a, b = a.contiguous(), b.contiguous()
    L, st = _lib.lib(), _stream()
    with torch.cuda.device(a.device):
        ws_bytes = L.dasr_img_ws_bytes(1, c, h, w, border)
        if ws_bytes < 0:
            raise _lib.DasrHipError('dasr_img_ws_bytes refuses C %d H %d W %d crop %d' % (c, h, w, border))
        ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=a.device)
        res = torch.zeros(3 + 2 * c, dtype=torch.int64, device=a.device)   # words: sse, ssim (fp64), c sums of a, c sums of b, lpips (fp64)
        r0, args = res.data_ptr(), (1, c, h, w, border)
        _lib.check(L.dasr_img_sse(a.data_ptr(), b.data_ptr(), *args, r0, None, ws.data_ptr(), ws_bytes, st), 'dasr_img_sse')
        _lib.check(L.dasr_img_ssim_box(a.data_ptr(), b.data_ptr(), *args, r0 + 8, ws.data_ptr(), ws_bytes, st), 'dasr_img_ssim_box')
        _lib.check(L.dasr_img_channel_sums(a.data_ptr(), *args, r0 + 16, ws.data_ptr(), ws_bytes, st), 'dasr_img_channel_sums')
        _lib.check(L.dasr_img_channel_sums(b.data_ptr(), *args, r0 + 16 + 8 * c, ws.data_ptr(), ws_bytes, st), 'dasr_img_channel_sums')
        if lpips is not None:
            res[2 + 2 * c:].view(torch.float64).copy_(lpips.detach().reshape(1))
        host = res.cpu()   # the one synchronisation
    words, f64 = host.tolist(), host.view(torch.float64)
    out = {'psnr': psnr_from_sse(words[0], c * ch * cw), 'psnr_col': psnr_col_from_sums(words[2:2 + c], words[2 + c:2 + 2 * c], ch * cw),
           'ssim': float(f64[1])}
    if lpips is not None:
        out['lpips'] = float(f64[2 + 2 * c])
    return out


def image_metrics(sr, hr, crop, ssim=True, y=True, min_max=(0, 1)):
    """batch_metrics for image 0 of the batch (what get_current_visuals hands the drivers): dict of Python floats"""
    sr, hr = _as_batch(sr), _as_batch(hr)
    return {k: v[0] for k, v in batch_metrics(sr[:1], hr[:1], crop, ssim=ssim, y=y, min_max=min_max).items()}
