"""fp64 model of dasr_conv and of dasr_pack_weights, its operand producer, as include/dasr_hip.h documents them.  Plain torch on the CPU, no device
code: tests/test_conv_ref.py holds the model to stock torch (F.conv2d, F.interpolate, autograd) on a machine without a GPU; tests/test_gpu_conv.py
then holds the kernels of csrc/conv.hip to the model, element by element.

The model computes what the kernel is MEANT to compute: the operands rounded as the header states (the lo*lo term of the split precisions is absent
here too), every product and sum after that in fp64.  What separates a correct kernel from `ref` is then its fp32 accumulation and the fp32
roundings of its epilogue, which the caller bounds with
    S = sum |w_t| |x_t|  over exactly the products the kernel forms,  and  L = the number of products behind one accumulator.
Layout helpers and roundings come from oracle/blocked_ref.py."""
import torch

from .blocked_ref import r16, split16

KIND = {1: 'bf16', 2: 'f16', 3: 'bf16', 4: 'f16'}   # 16-bit operand format per dasr_conv_params::prec


def c16(c):
    return (c + 15) // 16 * 16


# ---- dasr_pack_weights ---------------------------------------------------------------------------------------------------------------------------
def pack_weights(params_flat, cout, cin_pad, ntaps, segs, tapmap=None, src_ntaps=None, tapmasks=None):
    """The fp32 value of every packed weight BEFORE its rounding, W[cout][cin_pad][ntaps] (the MFMA-fragment order is a layout, not arithmetic).
    Arguments as engine.PackRegistry.add: segs = up to five (src_off, src_cout, src_cin, cin_start, cin_len, src_c0, transpose) over the flat fp32
    parameter buffer; tapmap: packed tap -> source tap (-1: none; default identity, reversed when the segments are transposed); tapmasks: packed tap
    t = fp32 sum, in ascending source-tap order, of the source taps whose bits are set.  cin_pad counts REAL channels (a split-tensor pack passes
    its K real chunks, not the 3K virtual ones).  Channels no segment feeds are zero; where segments overlap the later one wins."""
    assert len(segs) <= 5 and ntaps <= 32
    src_ntaps = src_ntaps or ntaps
    if tapmap is None:
        tapmap = [ntaps - 1 - t for t in range(ntaps)] if (segs and segs[0][6]) else list(range(ntaps))
    flat = params_flat.detach().float().cpu()
    W = torch.zeros(cout, cin_pad, ntaps, dtype=torch.float32)
    for (off, s_cout, s_cin, c_start, c_len, s_c0, tr) in segs:
        src = flat[off:off + s_cout * s_cin * src_ntaps].view(s_cout, s_cin, src_ntaps)
        if not tr:   # W[oc][c_start + ci] = src[oc][s_c0 + ci]
            blk = src[:cout, s_c0:s_c0 + c_len]
        else:        # W[oc][c_start + ci] = src[ci][s_c0 + oc], ci < src_cout
            blk = src[:c_len, s_c0:s_c0 + cout].transpose(0, 1)
        taps = torch.zeros(blk.shape[0], blk.shape[1], ntaps, dtype=torch.float32)
        for t in range(ntaps):
            m = tapmasks[t] if (tapmasks is not None and t < len(tapmasks) and t < 16) else 0
            if m:
                acc = torch.zeros(blk.shape[0], blk.shape[1], dtype=torch.float32)
                for k in range(min(src_ntaps, 16)):
                    if m & (1 << k):
                        acc = acc + blk[:, :, k]          # fp32, ascending tap order
                taps[:, :, t] = acc
            elif t < len(tapmap) and tapmap[t] >= 0:
                taps[:, :, t] = blk[:, :, tapmap[t]]
        W[:blk.shape[0], c_start:c_start + blk.shape[1]] = taps
    return W


# ---- dasr_conv -----------------------------------------------------------------------------------------------------------------------------------
def _patches(x, kh, stride, pad, pad_x, ups, Hout, Wout):
    """x NCHW fp64 on the Hin x Win grid -> [N][C][kh * kh][Hout][Wout]: the input element under tap (ky, kx) of output pixel (oy, ox), zero outside
    the (up-sampled) image"""
    if ups:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)   # nearest x2: pixel (y, x) reads (y >> 1, x >> 1)
    N, C, HL, WL = x.shape
    bot = max(0, (Hout - 1) * stride - pad + kh - HL)
    right = max(0, (Wout - 1) * stride - pad_x + kh - WL)
    xp = torch.nn.functional.pad(x, (pad_x, right, pad, bot))
    out = torch.empty(N, C, kh * kh, Hout, Wout, dtype=x.dtype)
    for ky in range(kh):
        for kx in range(kh):
            out[:, :, ky * kh + kx] = xp[:, :, ky:ky + (Hout - 1) * stride + 1:stride, kx:kx + (Wout - 1) * stride + 1:stride]
    return out


def _sub(t, Hout, Wout, out_stride, out_oy, out_ox):
    """the part of a full-resolution tensor an output sub-grid addresses"""
    if t is None:
        return None
    t = t.double()
    if out_stride > 1:
        t = t[:, :, out_oy::out_stride, out_ox::out_stride]
    assert t.shape[2] >= Hout and t.shape[3] >= Wout, (t.shape, Hout, Wout)
    return t[:, :, :Hout, :Wout]


def conv_detail(w, bias, x, Hout, Wout, prec=3, kh=3, stride=1, pad=1, pad_x=-1, ups=0, x_lo=None, in_scale=0.0, rounding=True,
                in_stride=1, in_oy=0, in_ox=0, Hin=None, Win=None,
                act=0, slope=0.0, mask=None, alpha=1.0, res1=None, res1_lo=None, beta1=0.0, res2=None, beta2=0.0,
                out_stride=1, out_oy=0, out_ox=0):
    """w: fp32 weights, [cout][cin][kh][kw] (reference layout) or [cout][cin][taps] (pack_weights); bias [cout] or None; x NCHW, cin channels --
    an fp32 tensor, or with x_lo the hi / lo planes of a split 16-bit tensor (in_wrap: then prec 1 / 2 name the 16-bit format).  in_stride 2: x is the
    tensor the Hin x Win grid is a parity sub-grid of.  mask / res1 / res2 are given at the full resolution of the output tensor (out_stride 2: the
    sub-grid (out_oy, out_ox) of it is used); res1_lo: res1 is a split tensor, read as hi + lo.  slope: the value the kernel sees (slope or
    *slope_ptr).  rounding False: un-rounded operands (the model against stock torch).
    Returns a dict: ref (fp64, [N][cout][Hout][Wout]), S, L as the module docstring defines them, and for the epilogue's own roundings
    `pre` = acc + bias before the activation, `terms` = the sum of the absolute values of the terms of the epilogue expression (in front of every
    rounding of it), `gain` = the factor by which the epilogue passes an error of the accumulator on."""
    kind = KIND[prec]
    w = w.detach().float().cpu()
    w = w.reshape(w.shape[0], w.shape[1], -1)
    cout, cin, ntaps = w.shape
    assert ntaps == kh * kh and x.shape[1] == cin, (w.shape, x.shape, kh)
    px = pad if pad_x < 0 else pad_x
    if in_stride > 1:   # grid pixel (y, x) lives at (2 y + in_oy, 2 x + in_ox)
        x = x[:, :, in_oy::in_stride, in_ox::in_stride][:, :, :Hin, :Win]
        x_lo = None if x_lo is None else x_lo[:, :, in_oy::in_stride, in_ox::in_stride][:, :, :Hin, :Win]
    sc = float(in_scale) if (in_scale and prec in (2, 4) and x_lo is None) else 1.0
    split = prec in (3, 4) or x_lo is not None
    if not rounding:
        prods, nterm = [(w.double(), x.double())], (3 if split else 1)
    elif x_lo is not None:       # split 16-bit tensor: the stored planes; weights [hi | hi | lo]
        wh, wl = split16(w, kind)
        prods, nterm = [(wh.double(), x.double()), (wh.double(), x_lo.double()), (wl.double(), x.double())], 3
    elif prec in (1, 2):
        prods, nterm = [(r16(w, kind).double(), r16(x.float() * sc, kind).double())], 1
    else:
        wh, wl = split16(w, kind)
        xh, xl = split16(x.float() * sc, kind)
        prods, nterm = [(wh.double(), xh.double()), (wh.double(), xl.double()), (wl.double(), xh.double())], 3
    acc = S = 0.0
    for wo, xo in prods:
        P = _patches(xo, kh, stride, pad, px, ups, Hout, Wout)
        acc = acc + torch.einsum('ock,nckhw->nohw', wo, P)
        S = S + torch.einsum('ock,nckhw->nohw', wo.abs(), P.abs())
    acc, S = acc / sc, S / sc
    L = ntaps * cin * nterm
    # ---- epilogue, in the header's order
    v, mag, gain = acc, acc.abs(), 1.0
    if bias is not None:
        b = bias.detach().double().cpu().view(1, -1, 1, 1)
        v, mag = v + b, mag + b.abs()
    pre = v
    if act == 1:
        f = torch.where(v > 0, torch.ones_like(v), torch.full_like(v, slope))
        v, mag, gain = v * f, mag * f.abs(), gain * max(1.0, abs(slope))
    elif act == 2:
        v = 1.0 / (1.0 + torch.exp(-v))
        mag, gain = v.abs(), gain * 0.25
    m = _sub(mask, Hout, Wout, out_stride, out_oy, out_ox)
    if m is not None:   # +0 and -0 are "not > 0"
        f = torch.where(m > 0, torch.ones_like(v), torch.full_like(v, slope))
        v, mag, gain = v * f, mag * f.abs(), gain * max(1.0, abs(slope))
    v, mag, gain = alpha * v, abs(alpha) * mag, gain * abs(alpha)
    r1 = _sub(res1, Hout, Wout, out_stride, out_oy, out_ox)
    if r1 is not None:
        if res1_lo is not None:
            r1 = r1 + _sub(res1_lo, Hout, Wout, out_stride, out_oy, out_ox)
        v, mag = v + beta1 * r1, mag + (beta1 * r1).abs()
    r2 = _sub(res2, Hout, Wout, out_stride, out_oy, out_ox)
    if r2 is not None:
        v, mag = v + beta2 * r2, mag + (beta2 * r2).abs()
    return dict(ref=v, S=S, L=L, pre=pre, terms=mag, gain=gain, r1=r1)


def conv(*args, **kw):
    """(ref, S, L) of conv_detail"""
    d = conv_detail(*args, **kw)
    return d['ref'], d['S'], d['L']


def out16(v, gamma, kind, split=False):
    """the 16-bit output of a value v: round16(gamma * v); split: (hi, lo = round16(gamma * v - hi))"""
    gv = (gamma * v.double()).float()
    if not split:
        return r16(gv, kind)
    return split16(gv, kind)


def scatter(dst, sub, out_stride=1, out_oy=0, out_ox=0):
    """write an output sub-grid into the full-resolution tensor it addresses (in place)"""
    Ho, Wo = sub.shape[2], sub.shape[3]
    if out_stride > 1:
        dst[:, :, out_oy::out_stride, out_ox::out_stride][:, :, :Ho, :Wo] = sub.to(dst.dtype)
    else:
        dst[:, :, :Ho, :Wo] = sub.to(dst.dtype)
    return dst
