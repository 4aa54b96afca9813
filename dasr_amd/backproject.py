"""Iterative back-projection of an SR image onto its LR input (reference: codes/SRN/scripts/back_projection/backprojection.m, MATLAB only; the usual ESRGAN / BasicSR
post-process that makes the SR image consistent with the LR image it came from).  `maxIter` times:

    d  = LR - imresize(SR, 1 / s)                      (bicubic, antialiased)
    SR = SR + conv2(imresize(d, s), p, 'same')         (bicubic; p the squared, renormalised 5 x 5 Gaussian of sigma 1)

back_project runs it on the device, two launches per iteration (csrc/imgio.hip: dasr_bp_residual, dasr_bp_update) and no host synchronisation;
back_project_fp64 is the restatement on the host in float64 the tests compare against.  The option key `"back_projection"` (options.back_projection_iters) puts it
behind test() / test_x8() of the SRN models, `python -m dasr_amd.back_projection` runs it on folders of PNG files (main_bp.m).

reverse_filter / reverse_filter_fp64, at the end, are the second post-process the reference ships (main_reverse_filter.m): the same residual, up-sampled without the
Gaussian (csrc/imgio.hip: dasr_imresize_up); `--reverse_filter` of the folder CLI."""
import ctypes as C
import math

import torch

from . import _lib
from .engine import _stream
from .imgio import down_table_ptrs, up_tap_table

DEFAULT_ITERS = 20          # main_bp.m:7
SCALES = (2, 3, 4)
RES_TILE = (8, 32)          # LR outputs per workgroup of bp_residual_kernel (DASR_BP_RES_TILE_H / _W of include/dasr_hip.h; tests/test_back_projection_host.py compares)
UPD_TILE = (16, 64)         # SR samples per workgroup of bp_update_kernel (DASR_BP_UPD_TILE_H / _W)

_U5 = None


def gaussian_u5():
    """the 5 weights u_i = exp(-i^2) / sum_j exp(-j^2), i = -2 .. 2, as a list of floats: backprojection.m:6-8's p = fspecial('gaussian', 5, 1) .^ 2, renormalised, is
    outer(u, u) (exp(-(x^2 + y^2) / 2)^2 = exp(-x^2) exp(-y^2); tests/test_back_projection_host.py pins the equality to 1e-15)"""
    e = [math.exp(-float(i * i)) for i in range(-2, 3)]
    t = math.fsum(e)
    return [v / t for v in e]


def gaussian_p():
    """the 5 x 5 kernel of backprojection.m:6-8 as MATLAB forms it, float64"""
    r = torch.arange(-2, 3, dtype=torch.float64)
    p = torch.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / 2.0)   # :6  fspecial('gaussian', 5, 1) ...
    p = p / p.sum()                                              #     ... which normalises its kernel
    p = p ** 2                                                   # :7  p = p.^2
    return p / p.sum()                                           # :8  p = p./sum(p(:))


def scale_of(sr_shape, lr_shape):
    """the integer s in {2, 3, 4} with sr = [1, C, s h, s w] for lr = [1, C, h, w]; anything else is a ValueError naming the shapes"""
    sr_shape, lr_shape = tuple(sr_shape), tuple(lr_shape)
    what = 'back_project takes sr [1, C, s h, s w] and lr [1, C, h, w] with one s in {2, 3, 4}, got sr %s and lr %s' % (sr_shape, lr_shape)
    if len(sr_shape) != 4 or len(lr_shape) != 4 or sr_shape[0] != 1 or lr_shape[0] != 1:
        raise ValueError(what + ': one image at a time')
    if sr_shape[1] != lr_shape[1] or sr_shape[1] < 1:
        raise ValueError(what + ': the channel counts differ')
    (H, W), (h, w) = sr_shape[2:], lr_shape[2:]
    if h < 1 or w < 1 or H % h or W % w or H // h != W // w or H // h not in SCALES:
        raise ValueError(what + ': the size ratio is not one integer of %s on both axes' % (SCALES,))
    return H // h


def _u5():
    """gaussian_u5 as the host array dasr_bp_update takes (made once)"""
    global _U5
    if _U5 is None:
        _U5 = (C.c_double * 5)(*gaussian_u5())
    return C.cast(_U5, C.c_void_p)


def _tables(H, W, s, device):
    return down_table_ptrs(H, W, s, device), [t.data_ptr() for n in (H // s, W // s) for t in up_tap_table(n, s, device)]


def _checked(sr, lr):
    for name, t in (('sr', sr), ('lr', lr)):
        if not torch.is_tensor(t) or t.device.type != 'cuda' or t.dtype != torch.float32:
            raise ValueError('back_project runs HIP kernels on fp32 device tensors; %s is %s' % (
                name, '%s on %s' % (t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    if sr.device != lr.device:
        raise ValueError('back_project: sr is on %s, lr on %s' % (sr.device, lr.device))
    return scale_of(sr.shape, lr.shape)


def residual(sr, lr):
    """d = lr - (float)imresize(sr, 1 / s), one launch (dasr_bp_residual): [1, C, h, w] fp32"""
    s = _checked(sr, lr)
    sr, lr = sr.detach().contiguous(), lr.detach().contiguous()
    _, c, H, W = sr.shape
    d = torch.empty_like(lr)
    down, _ = _tables(H, W, s, sr.device)
    _lib.check(_lib.lib().dasr_bp_residual(sr.data_ptr(), lr.data_ptr(), c, H, W, s, *down, d.data_ptr(), _stream()), 'dasr_bp_residual')
    return d


def update_(sr, d):
    """sr += conv2(imresize(d, s), p, 'same') in place on the contiguous fp32 device tensor sr, one launch (dasr_bp_update); returns sr"""
    s = _checked(sr, d)
    if not sr.is_contiguous():
        raise ValueError('update_ works in place on a contiguous tensor')
    d = d.detach().contiguous()
    _, c, h, w = d.shape
    _, up = _tables(s * h, s * w, s, sr.device)
    _lib.check(_lib.lib().dasr_bp_update(sr.data_ptr(), d.data_ptr(), c, h, w, s, *up, _u5(), _stream()), 'dasr_bp_update')
    return sr


def back_project(sr, lr, iters=DEFAULT_ITERS):
    """`iters` iterations of backprojection.m on the device: sr [1, C, s h, s w], lr [1, C, h, w], fp32 device tensors, s in {2, 3, 4} taken from the shapes.  Returns a
    new tensor; the inputs are left as they are; iters == 0 returns a bit-equal copy.  No clamp (MATLAB clamps only in imwrite; here tensor2img does).  Every iteration
    is two launches on the current stream and nothing is synchronised.  A batch above 1, unequal channel counts or a size ratio that is not one integer of
    {2, 3, 4} on both axes: ValueError naming the shapes."""
    s = _checked(sr, lr)
    iters = int(iters)
    if iters < 0:
        raise ValueError('back_project: iters must be >= 0, got %d' % iters)
    out = sr.detach().clone(memory_format=torch.contiguous_format)
    if iters == 0:
        return out
    lr = lr.detach().contiguous()
    _, c, H, W = out.shape
    d = torch.empty_like(lr)
    down, up = _tables(H, W, s, out.device)
    L, st, u5 = _lib.lib(), _stream(), _u5()
    for _ in range(iters):
        _lib.check(L.dasr_bp_residual(out.data_ptr(), lr.data_ptr(), c, H, W, s, *down, d.data_ptr(), st), 'dasr_bp_residual')
        _lib.check(L.dasr_bp_update(out.data_ptr(), d.data_ptr(), c, H // s, W // s, s, *up, u5, st), 'dasr_bp_update')
    return out


def upsample_conv_fp64(d, s):
    """conv2(imresize(d, s), p, 'same') of a [C, h, w] tensor in float64: what one dasr_bp_update adds to sr"""
    from .data import imresize_matlab
    p = gaussian_p()
    up = imresize_matlab(d.to(torch.float64), float(s))                      # :15 im_diff = imresize(im_diff, [row_h, col_h], 'bicubic')
    c, H, W = up.shape
    pad = torch.zeros((c, H + 4, W + 4), dtype=torch.float64)                # :16-18 conv2(., p, 'same'): zeros beyond the image (p is symmetric: correlation)
    pad[:, 2:-2, 2:-2] = up
    acc = torch.zeros_like(up)
    for a in range(5):
        for b in range(5):
            acc += p[a, b] * pad[:, a:a + H, b:b + W]
    return acc


def back_project_fp64(sr, lr, iters=DEFAULT_ITERS, trace=None):
    """backprojection.m line by line on the host, all float64: sr [1, C, s h, s w] (or [C, s h, s w]) and lr likewise, any float dtype, CPU.  Returns the float64 image in
    the shape of sr.  `trace`: a list that receives max|lr - imresize(sr_k, 1 / s)| in front of every iteration and after the last one.  Slow (dense resampling
    matrices): for tests and for scripts/back_projection_ab.py."""
    from .data import imresize_matlab
    batched = sr.dim() == 4
    s = scale_of(sr.shape if batched else (1,) + tuple(sr.shape), lr.shape if lr.dim() == 4 else (1,) + tuple(lr.shape))
    im_l = (lr[0] if lr.dim() == 4 else lr).detach().cpu().to(torch.float64)     # :10 im_l = double(im_l)
    im_h = (sr[0] if batched else sr).detach().cpu().to(torch.float64).clone()   # :11 im_h = double(im_h)
    for _ in range(int(iters)):                                                  # :12 for ii = 1:maxIter
        im_l_s = imresize_matlab(im_h, 1.0 / s)                                  # :13 im_l_s = imresize(im_h, [row_l, col_l], 'bicubic')
        im_diff = im_l - im_l_s                                                  # :14 im_diff = im_l - im_l_s
        if trace is not None:
            trace.append(float(im_diff.abs().max()))
        im_h = im_h + upsample_conv_fp64(im_diff, s)                             # :15-18
    if trace is not None:
        trace.append(float((im_l - imresize_matlab(im_h, 1.0 / s)).abs().max()))
    return im_h[None] if batched else im_h


def reverse_filter(sr, lr, iters=DEFAULT_ITERS):
    """`iters` iterations of the reverse filter (codes/SRN/scripts/back_projection/main_reverse_filter.m:18-22) on the device:

        J = imresize(LR, s);   out = out + (J - imresize(imresize(out, 1 / s), s))

    Bicubic up-sampling is linear, so J - up(down(out)) = up(LR - down(out)): every iteration is dasr_bp_residual (d = lr - down(out)) and one dasr_imresize_up that adds
    up(d) onto out with one rounding; J is never formed.  The contract is back_project's: sr [1, C, s h, s w], lr [1, C, h, w], fp32 device tensors, s in {2, 3, 4} from
    the shapes; a new tensor, the inputs left as they are, iters == 0 a bit-equal copy, no clamp, nothing synchronised, ValueError naming the shapes."""
    from .bicubic import upsample
    s = _checked(sr, lr)
    iters = int(iters)
    if iters < 0:
        raise ValueError('reverse_filter: iters must be >= 0, got %d' % iters)
    out = sr.detach().clone(memory_format=torch.contiguous_format)
    if iters == 0:
        return out
    lr = lr.detach().contiguous()
    _, c, H, W = out.shape
    d = torch.empty_like(lr)
    down, _ = _tables(H, W, s, out.device)
    L, st = _lib.lib(), _stream()
    for _ in range(iters):
        _lib.check(L.dasr_bp_residual(out.data_ptr(), lr.data_ptr(), c, H, W, s, *down, d.data_ptr(), st), 'dasr_bp_residual')
        upsample(d, s, into=out)
    return out


def reverse_filter_fp64(sr, lr, iters=DEFAULT_ITERS, literal=True):
    """main_reverse_filter.m:18-22 on the host, all float64: sr [1, C, s h, s w] (or [C, s h, s w]) and lr likewise, any float dtype, CPU.  `literal`: the MATLAB lines
    as they stand, J formed once; otherwise the form the device runs, out + up(lr - down(out)).  Returns the float64 image in the shape of sr."""
    from .data import imresize_matlab
    batched = sr.dim() == 4
    s = scale_of(sr.shape if batched else (1,) + tuple(sr.shape), lr.shape if lr.dim() == 4 else (1,) + tuple(lr.shape))
    im_lr = (lr[0] if lr.dim() == 4 else lr).detach().cpu().to(torch.float64)
    im_out = (sr[0] if batched else sr).detach().cpu().to(torch.float64).clone()
    J = imresize_matlab(im_lr, float(s))                                                              # :18 J = imresize(im_LR, 4, 'bicubic')
    for _ in range(int(iters)):                                                                       # :20 for m = 1:max_iter
        if literal:
            im_out = im_out + (J - imresize_matlab(imresize_matlab(im_out, 1.0 / s), float(s)))       # :21
        else:
            im_out = im_out + imresize_matlab(im_lr - imresize_matlab(im_out, 1.0 / s), float(s))
    return im_out[None] if batched else im_out
