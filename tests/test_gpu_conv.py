"""GPU parity tests of dasr_conv (csrc/conv.hip) and of dasr_pack_weights as its operand producer, in every dispatch mode of the launcher, against the
fp64 model of oracle/conv_ref.py (itself held to stock torch by tests/test_conv_ref.py).

Set-up of every case (as tests/test_gpu_elementwise.py): the input is planes [c0, c0 + K) of a wider slab whose other planes hold NaN (a halo or
chunk read outside the view makes the output non-finite), padding channels inside the view are zero; mask and residuals are slab views whose padding
channels hold NaN (the kernel must not let them through: padded output channels are written as exact zeros); outputs are views of sentinel-filled
slabs and everything outside the written region must come back bit for bit.

What is asserted, per element (no norms):
    |got - ref| <= c(L) 2^-23 S gain + k 2^-24 terms
c(L) = 4 + 2 sqrt(L) as tests/test_gpu_wgrad.py uses it for fp32 MFMA accumulation (L = taps x padded cin, x 3 for the split precisions), S = sum
|w_t| |x_t| over the products the kernel forms, gain = what the epilogue multiplies an accumulator error by, k = the fp32 roundings of the epilogue
expression (counted in k_epilogue below), terms = the sum of the absolute values of the terms of that expression.  The 16-bit output is held to
round16(gamma ref) within the propagated bound plus half a 16-bit ulp, and where both outputs are written with gamma = 1 to round16 of the kernel's
own f32 output bit for bit.

Where each `case` label of the dasr_conv switch is hit (test id after the label):
    10    glds[k10_e67_*], glds[k10_e68_*], glds[k10_gen_*]          20    conv5[bf16-*] (232 / 233 / 248 / 249, both shapes), glds[k20_gen_*], glds[k20_e*_small]
    110   reg[p1_mt1]     120   reg[p1_mt2_c96], reg[p1_f16out_both_g1]
    1110  reg[p3_k0] epi[reg-*]   1111 reg[p3_k1]   1112 reg[p3_k2]   1113 reg[p3_k3] strided_out[*-3]   1114 reg[p3_k4]   1115 reg[p3_k5]   1116 reg[p3_k6]
    2010  glds[k2010_e67_*], [k2010_e68_*], [k2010_e64_*], [k2010_gen_*], [k2010_ups]
    2020  conv5[f16-*], glds[k2020_e67 / e68 / e64 / gen], glds[k2020_e*_8w_small]
    3110 .. 3116  reg[p4_k0 .. p4_k6] (3113 also strided_out[*-4])
    2110 .. 2116  reg[p2_k0 .. p2_k6]     2120  reg[p2_mt2_c96]     2123  reg[p2_mt2_k3]
    default (DASR_EINVAL)  test_rejections"""
import ctypes as C
import math
import re

import pytest
import torch

from oracle import blocked_ref as R
from oracle import conv_ref as CR
from test_gpu_elementwise import SENT, Slab, _gpu, biteq, bounded, gen

EINVAL = -22
U32 = R.U32
NAN = float('nan')
gpu = pytest.mark.gpu


def c_of(L):
    """fp32 MFMA accumulation over L products, in units of 2^-23 S (tests/test_gpu_wgrad.py)"""
    return 4.0 + 2.0 * math.sqrt(L)


def nan_slab(dev, kind, N, K, H, W, data, lead=1):
    """K planes inside a slab whose other planes hold NaN"""
    s = Slab(dev, kind, N, K, H, W, None, lead=lead)
    s.b.t.fill_(NAN)
    s.b.t[:, s.p0:s.p0 + K].copy_(data)
    s.before = s.b.t.cpu().clone()
    return s


class Weights:
    """fp32 master weights + bias in a ParamStore, one packed conv made from them by dasr_pack_weights, and the model's view of the same pack"""

    def __init__(self, dev, src_shape, cout, cin, ntaps, mt, fmt, seed, segs=None, tapmap=None, src_ntaps=None, tapmasks=None):
        from dasr_amd.engine import PackRegistry, ParamStore
        g = gen(seed)
        fan = src_shape[1] * src_shape[2] * src_shape[3]
        self.w = torch.randn(*src_shape, generator=g) * math.sqrt(2.0 / fan)
        self.b = torch.randn(cout, generator=g) * 0.1
        self.P = ParamStore([('w', tuple(src_shape)), ('b', (cout,))], dev)
        self.P.load_state_dict({'w': self.w, 'b': self.b})
        segs = segs or [(0, src_shape[0], src_shape[1], 0, src_shape[1], 0, 0)]
        cpad = CR.c16(cin)
        self.pack = PackRegistry(self.P)
        self.ref = self.pack.add(cout, 3 * cpad if fmt in (5, 6) else cpad, ntaps, mt, fmt, segs, tapmap=tapmap, src_ntaps=src_ntaps, tapmasks=tapmasks)
        self.pack.finalize()
        self.pack.run()
        self.eff = CR.pack_weights(self.P.flat.cpu(), cout, cpad, ntaps, segs, tapmap=tapmap, src_ntaps=src_ntaps, tapmasks=tapmasks)


def launch(op, via):
    from dasr_amd import _lib
    from dasr_amd.engine import OpList, _stream
    if via == 'op':
        ol = OpList()
        ol.add(op)
        try:
            ol.run()
            rc = 0
        except _lib.DasrHipError as e:
            rc = int(re.search(r'code (-?\d+)', str(e)).group(1))
    else:
        rc = _lib.lib().dasr_conv(C.byref(op.conv), _stream())
    torch.cuda.synchronize()
    return rc


def k_epilogue(c, r1_pre):
    """fp32 roundings of v = alpha * mask'(act(acc + bias)) + beta1 res1 + beta2 res2, one per operation:
    bias: the sum (1).  act 1: slope * v (1; the select / max / the sum with an exact zero add nothing).  mask: slope * v (1).  alpha != 1: the product (1).
    res1: beta1 * r and the sum (2); a split res1 is first summed hi + lo (1 more); the conv5 epilogues of the LDS-DMA kernel start the accumulator
    at (beta1 / alpha) * res1: the quotient, that product, and alpha times the sum (the accumulation on top is counted in c(L)): 3.  res2: 2.
    The sigmoid is counted apart (k_sigmoid)."""
    k = (1 if c['bias'] else 0) + (1 if c['act'] == 1 else 0) + (1 if c['mask'] else 0) + (1 if c['alpha'] != 1.0 else 0)
    k += {None: 0, 'f32': 3 if r1_pre else 2, 'split': 3}[c['res1']] + (2 if c['res2'] else 0)
    return k


def k_sigmoid(v):
    """the kernel evaluates sigmoid as __frcp_rn(1.f + __expf(-v)): v_mul_f32 by log2(e) (the rounded constant and the product: a relative error of
    2 |v| u on 2^t), v_exp_f32 (1 ulp = 2 u), the sum with 1 (1 u), v_rcp_f32 (1 ulp = 2 u); the first two reach y = 1 / (1 + e) through e / (1 + e) <= 1.
    In units of u |y|: 5 + 2 |v|."""
    return 5.0 + 2.0 * v.abs()


DEFAULT = dict(prec=3, tens='f32', mt=1, kh=3, stride=1, pad=1, pad_x=-1, cin=16, cout=32, N=2, Ho=5, Wo=7, ups=0, bias=True, act=0, slope=0.2, sptr=False,
               mask=False, alpha=1.0, res1=None, beta1=0.0, res2=False, beta2=0.0, outs='f32', gamma=1.0, o16split=False, in_scale=0.0, xmag=1.0, tune=None, seed=1,
               k16='bf16',     # format of the 16-bit output of an f32-tensor launch (out16_f16); the LDS-DMA kernel writes its operand format
               conv5=False)    # the case is a conv5-class launch of the LDS-DMA kernel (epilogues 232 / 233 / 248 / 249)


def run_conv(dev, margins, name, via='abi', **over):
    """one dense launch: build, run, check every element and everything around the written region"""
    from dasr_amd import _lib
    from dasr_amd.engine import conv_op
    c = dict(DEFAULT, **over)
    prec, tens, kh, stride, pad, N, cin, cout = c['prec'], c['tens'], c['kh'], c['stride'], c['pad'], c['N'], c['cin'], c['cout']
    f32 = lambda v: R.f32(v)
    slope, alpha, beta1, beta2, gamma = f32(c['slope']), f32(c['alpha']), f32(c['beta1']), f32(c['beta2']), f32(c['gamma'])
    in_f32, split_in = tens == 'f32', tens in ('sf16', 'sbf16')
    glds = not in_f32
    k16 = ('f16' if prec in (2, 4) else 'bf16') if glds else c['k16']
    px = pad if c['pad_x'] < 0 else c['pad_x']
    Ho, Wo = c['Ho'], c['Wo']
    HL, WL = (Ho - 1) * stride + kh - 2 * pad, (Wo - 1) * stride + kh - 2 * px      # the (up-sampled) input size this output size comes from
    if c['ups']:
        assert HL % 2 == 0 and WL % 2 == 0
    H, W = (HL // 2, WL // 2) if c['ups'] else (HL, WL)
    g = gen(c['seed'] + 1000)
    fmt = {'sf16': 5, 'sbf16': 6}.get(tens, prec)
    wt = Weights(dev, (cout, cin, kh, kh), cout, cin, kh * kh, c['mt'], fmt, c['seed'])
    Kin, Kout, cpad = R.planes(cin), R.planes(cout), CR.c16(cin)
    x = torch.randn(N, cin, H, W, generator=g) * c['xmag']
    xz = torch.zeros(N, cpad, H, W)
    x_lo = None
    if in_f32:
        xs = nan_slab(dev, 'f32', N, Kin, H, W, R.pack(x, 'f32'))
        xz[:, :cin] = x
    elif not split_in:
        x = R.r16(x, k16).float()               # the stored values are the operands
        xs = nan_slab(dev, k16, N, Kin, H, W, R.pack(x, k16))
        xz[:, :cin] = x
    else:
        hi, lo = R.split16(x, k16)
        xs = nan_slab(dev, k16, N, 2 * Kin, H, W, R.pack_split(hi, lo))
        xz, x_lo = xz.to(hi.dtype), torch.zeros(N, cpad, H, W, dtype=hi.dtype)
        xz[:, :cin], x_lo[:, :cin] = hi, lo
    mkind = 'f32' if in_f32 else k16
    kw = dict(kh=kh, stride=stride, pad=pad, pad_x=c['pad_x'], ups=c['ups'], act=c['act'], slope=slope, alpha=alpha, gamma=gamma, in_scale=c['in_scale'])
    ms = r1s = r2s = None
    m = r1 = r1lo = r2 = None
    if c['mask']:
        m = torch.randn(N, cout, Ho, Wo, generator=g)
        m[0, 0, 0, 0], m[0, 1 % cout, 0, 0], m[N - 1, cout - 1, Ho - 1, Wo - 1] = 0.0, -0.0, 0.0    # +0 and -0 are "not > 0"
        m = R.r16(m, k16).float() if glds else m
        ms = nan_slab(dev, mkind, N, Kout, Ho, Wo, R.pack(m, mkind, NAN))
        kw.update(mask=ms.view(), mask_f32=int(in_f32))
    if c['res1'] == 'f32':
        r1 = torch.randn(N, cout, Ho, Wo, generator=g)
        r1s = nan_slab(dev, 'f32', N, Kout, Ho, Wo, R.pack(r1, 'f32', NAN))
        kw.update(res1=r1s.view(), beta1=beta1)
    elif c['res1'] == 'split':
        r1, r1lo = R.split16(torch.randn(N, cout, Ho, Wo, generator=g), k16)
        r1s = nan_slab(dev, k16, N, 2 * Kout, Ho, Wo, R.pack_split(r1, r1lo, NAN))
        kw.update(res1=r1s.view(), beta1=beta1, res1_lo=Kout)
    if c['res2']:
        r2 = torch.randn(N, cout, Ho, Wo, generator=g)
        r2s = nan_slab(dev, 'f32', N, Kout, Ho, Wo, R.pack(r2, 'f32', NAN))
        kw.update(res2=r2s.view(), beta2=beta2)
    sp = torch.tensor([slope], device=dev)
    if c['sptr']:
        kw.update(slope_ptr=sp.data_ptr(), slope=99.0)
    of = Slab(dev, 'f32', N, Kout, Ho, Wo)
    ob = Slab(dev, k16, N, (2 if c['o16split'] else 1) * Kout, Ho, Wo, lead=2)
    if c['outs'] in ('f32', 'both'):
        kw['out_f32'] = of.view()
    if c['outs'] in ('16', 'both'):
        kw.update(out_bf16=ob.view(), out16_f16=int(k16 == 'f16'), out16_lo=Kout if c['o16split'] else 0)
    op = conv_op(wt.pack, wt.ref, xs.view(), in_f32, 3 * cpad if split_in else cpad, H, W, Ho, Wo, N, bias=wt.P.ptr('b') if c['bias'] else None,
                 in_wrap=2 * Kin if split_in else 0, **kw)
    L_ = _lib.lib()
    if c['tune']:
        _lib.check(L_.dasr_set_tuning(2, c['tune']))
    try:
        rc = launch(op, via)
    finally:
        if c['tune']:
            _lib.check(L_.dasr_set_tuning(2, 13))
    assert rc == 0, rc
    d = CR.conv_detail(wt.eff, wt.b if c['bias'] else None, xz, Ho, Wo, prec=prec, kh=kh, stride=stride, pad=pad, pad_x=c['pad_x'], ups=c['ups'], x_lo=x_lo,
                       in_scale=c['in_scale'], act=c['act'], slope=slope, mask=m, alpha=alpha, res1=r1, res1_lo=r1lo, beta1=beta1, res2=r2, beta2=beta2)
    ref = d['ref']
    # conv5-class launches (64 output channels per workgroup of the LDS-DMA kernel, fp32 res1 and both outputs, no activation or mask: classify_epi of
    # csrc/conv.hip gives 232 / 233 / 248 / 249) start the accumulator at (beta1 / alpha) res1.  The case table marks them (conv5=True) and builds no
    # other 64-channel LDS-DMA launch with an fp32 res1, so the bound never depends on a copy of the launcher's rule:
    assert c['conv5'] == (glds and c['mt'] == 2 and c['res1'] == 'f32'), 'mark the case conv5, or give it another shape'
    assert not c['conv5'] or (cout % 32 == 0 and c['act'] == 0 and not c['mask'] and c['outs'] == 'both' and not c['o16split'])
    r1_pre = c['conv5']
    Sacc = d['S'] + ((beta1 * d['r1']).abs() / abs(alpha) if r1_pre else 0.0)      # the conv5 epilogues accumulate on top of (beta1 / alpha) res1
    b32 = c_of(d['L'] + (1 if r1_pre else 0)) * 2.0 ** -23 * Sacc * d['gain'] + k_epilogue(c, r1_pre) * U32 * d['terms']
    if c['act'] == 2:   # the sigmoid's own roundings, relative to |alpha| y
        b32 = b32 + k_sigmoid(d['pre']) * U32 * abs(alpha) * torch.sigmoid(d['pre'])
    tag = 'conv %s %s' % (name, via)
    for s in (xs, ms, r1s, r2s):
        assert s is None or s.untouched()
    got = None
    if c['outs'] in ('f32', 'both'):
        assert of.outside_untouched()
        got = of.nchw()
        bounded(tag + ' f32', got[:, :cout], ref, b32, margins)
        assert float(got[:, cout:].abs().max() if cout % 16 else 0.0) == 0.0          # padding channels of the last plane: exact zeros
    else:
        assert of.untouched()
    if c['outs'] == 'f32':
        assert ob.untouched()
        return
    assert ob.outside_untouched()
    o16 = ob.get()
    gref = gamma * ref
    f32_term = abs(gamma) * b32 + (0.0 if gamma in (0.5, 1.0, 2.0) else U32 * gref.abs())      # gamma * v: one more rounding unless a power of two
    if not c['o16split']:
        v16 = R.unpack(o16)
        bounded(tag + ' 16', v16[:, :cout], gref, f32_term + R.err16(gref.abs() + f32_term, k16), margins)
        if got is not None and gamma == 1.0:
            assert biteq(v16, CR.out16(got, 1.0, k16))
    else:
        hi16, lo16 = R.unpack_split(o16)
        val = hi16.double() + lo16.double()
        # hi + lo misses the f32 value by the rounding of the remainder (itself at most half a 16-bit ulp of the value)
        bounded(tag + ' 16 split', val[:, :cout], gref, f32_term + R.err16(R.err16(gref.abs() + f32_term, k16), k16), margins)
        if got is not None and gamma == 1.0:
            h, l = CR.out16(got, 1.0, k16, split=True)
            assert biteq(hi16, h) and biteq(lo16, l)
        v16 = val
    assert float(v16[:, cout:].abs().max() if cout % 16 else 0.0) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# register-staged conv_kernel: 7 kernel codes x prec 2 / 3 / 4; sizes rotate with the precision: smaller than a tile (5 x 7), one full + one partial
# tile each way, an exact multiple of the tile (16 x 32: 3x3, 2x2, 1x1; 8 x 32: 4x4 s1, 5x5; 8 x 16: stride 2)
KCODE = {0: (3, 1, 1), 1: (4, 1, 1), 2: (4, 2, 1), 3: (2, 1, 1), 4: (5, 1, 2), 5: (1, 1, 0), 6: (3, 2, 1)}   # kh, stride, pad
TILE = {0: (16, 32), 1: (8, 32), 2: (8, 16), 3: (16, 32), 4: (8, 32), 5: (16, 32), 6: (8, 16)}
CH = [(3, 40), (16, 3), (40, 64), (160, 32), (16, 40), (40, 3), (3, 64)]                                       # (cin, cout) per kernel code


def _size(code, which):
    th, tw = TILE[code]
    return {0: (5, 7), 1: (th + 3, tw + 5), 2: (th, tw)}[which]


REG = []
for _p in (2, 3, 4):
    for _k, (_kh, _s, _pad) in KCODE.items():
        _ho, _wo = _size(_k, _p - 2)
        REG.append(('p%d_k%d' % (_p, _k), dict(prec=_p, kh=_kh, stride=_s, pad=_pad, cin=CH[_k][0], cout=CH[_k][1], Ho=_ho, Wo=_wo, N=2 + (_k & 1),
                                                 act=1, mask=_k % 2 == 0, res1='f32' if _k % 3 == 0 else None, beta1=0.5, outs='both' if _k < 4 else 'f32')))
REG += [
    ('p1_mt1', dict(prec=1, cin=40, cout=40, Ho=19, Wo=37, act=1, outs='both')),
    ('p1_mt2_c96', dict(prec=1, mt=2, cin=16, cout=96, Ho=16, Wo=32, N=3, act=1, mask=True, outs='both')),            # a half-empty second m-group
    ('p2_mt2_c96', dict(prec=2, mt=2, cin=40, cout=96, Ho=19, Wo=37, res1='f32', beta1=1.0, alpha=0.2)),
    ('p2_mt2_k3', dict(prec=2, mt=2, kh=2, pad=1, pad_x=0, cin=16, cout=64, Ho=19, Wo=37, N=3)),
    ('p3_pad0', dict(prec=3, pad=0, cin=16, cout=40, Ho=19, Wo=37)),                                                   # LPIPS conv1 ...
    ('p3_pad2', dict(prec=3, pad=2, cin=40, cout=3, Ho=19, Wo=37, mask=True)),                                         # ... and its adjoint
    ('p2_pad0', dict(prec=2, pad=0, cin=3, cout=64, Ho=5, Wo=7)),
    ('p4_pad2', dict(prec=4, pad=2, cin=16, cout=32, Ho=16, Wo=32)),
] + [('p3_k1_pad%d' % p, dict(prec=3, kh=4, pad=p, cin=16, cout=40, Ho=11, Wo=37)) for p in (0, 2, 3)] \
  + [('p4_k2_pad%d' % p, dict(prec=4, kh=4, stride=2, pad=p, cin=16, cout=40, Ho=11, Wo=21, mask=True)) for p in (0, 2, 3)] \
  + [('p3_k3_pad%d%d' % (p, q), dict(prec=3, kh=2, pad=p, pad_x=q, cin=40, cout=40, Ho=19, Wo=37)) for p in (0, 1) for q in (0, 1)] \
  + [('p2_k3_pad%d%d' % (p, q), dict(prec=2, kh=2, pad=p, pad_x=q, cin=16, cout=3, Ho=5, Wo=7)) for p in (0, 1) for q in (0, 1)] + [
    ('p3_ups', dict(prec=3, ups=1, cin=40, cout=40, Ho=18, Wo=38, act=1)),                                             # odd low-resolution size 9 x 19
    ('p2_ups', dict(prec=2, ups=1, cin=16, cout=64, Ho=10, Wo=14, act=1, outs='both')),
    # inputs of magnitude 1e-7: without the pre-scale they are f16 subnormals (absolute error 2^-25, i.e. ~30 % of the value)
    ('p2_in_scale', dict(prec=2, cin=40, cout=40, Ho=19, Wo=37, xmag=1e-7, in_scale=4096.0, bias=False, mask=True)),
    ('p4_in_scale', dict(prec=4, cin=40, cout=40, Ho=19, Wo=37, xmag=1e-7, in_scale=4096.0, bias=False)),
    # out16_f16 on f32 tensors: the 16-bit output of conv_kernel as IEEE half (a run-time branch of its epilogue), alone and beside out_f32
    ('p2_f16out_16_g3', dict(prec=2, cin=40, cout=40, Ho=19, Wo=37, act=1, outs='16', gamma=3.0, k16='f16')),
    ('p2_f16out_both_g1', dict(prec=2, cin=16, cout=64, Ho=5, Wo=7, act=1, mask=True, outs='both', k16='f16')),
    ('p3_f16out_both_g1', dict(prec=3, cin=40, cout=40, Ho=19, Wo=37, res1='f32', beta1=0.5, outs='both', k16='f16')),
    ('p3_f16out_both_g3', dict(prec=3, kh=4, stride=2, cin=16, cout=3, Ho=11, Wo=21, outs='both', gamma=3.0, k16='f16')),
    ('p3_f16out_16_g1', dict(prec=3, cin=16, cout=32, Ho=16, Wo=32, act=1, outs='16', k16='f16')),
    ('p4_f16out_16_g3', dict(prec=4, kh=2, pad=0, pad_x=1, cin=16, cout=40, Ho=5, Wo=7, outs='16', gamma=3.0, k16='f16')),
    ('p1_f16out_both_g1', dict(prec=1, mt=2, cin=16, cout=64, Ho=19, Wo=37, outs='both', k16='f16')),
    ('p4_k3_in_scale', dict(prec=4, kh=2, pad=0, pad_x=1, cin=16, cout=32, Ho=5, Wo=7, xmag=1e-7, in_scale=4096.0, bias=False)),
]


@gpu
@pytest.mark.parametrize('name,case', REG, ids=[r[0] for r in REG])
def test_reg(name, case, margins):
    run_conv(_gpu(), margins, 'reg ' + name, 'abi', **dict(case, seed=len(name)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# LDS-DMA conv_glds_kernel (16-bit tensors, 3x3 / 1 / 1).  Tiles 16 x 32 (4 waves) and 32 x 32 (8 waves); N = 2 and N = 3 at 20 x 36 make the grid a
# multiple of 8 (the XCD-aware tile order is on) and not (it switches itself off); cin 16 is a single chunk: prologue and epilogue of the double buffer meet
def _g(prec, mt, **kw):
    return dict(dict(prec=prec, tens='f16' if prec == 2 else 'bf16', mt=mt, cout=32 * mt, bias=False, outs='16'), **kw)


E67 = dict(bias=True, act=1)
E68 = dict(mask=True)
GEN = dict(bias=True, act=1, slope=1.5, mask=True, outs='both', alpha=0.5)
GLDS = []
for _key, _p, _mt in ((10, 1, 1), (2010, 2, 1), (2020, 2, 2)):
    GLDS += [
        ('k%d_e67_small_c16' % _key, _g(_p, _mt, cin=16, Ho=5, Wo=7, **E67)),
        ('k%d_e67_n2_grid8' % _key, _g(_p, _mt, cin=64, Ho=20, Wo=36, N=2, **E67)),
        ('k%d_e67_n3_grid12' % _key, _g(_p, _mt, cin=64, Ho=20, Wo=36, N=3, **E67)),
        ('k%d_e68_partial_c160' % _key, _g(_p, _mt, cin=160, Ho=19, Wo=37, **E68)),
        ('k%d_e68_exact_sptr' % _key, _g(_p, _mt, cin=16, Ho=16, Wo=32, N=4, sptr=True, slope=-0.25, **E68)),
        ('k%d_e64_partial' % _key, _g(_p, _mt, cin=64, Ho=19, Wo=37)),                                               # (bf16: no such instance, the generic one)
        ('k%d_gen_partial' % _key, _g(_p, _mt, cin=64, Ho=19, Wo=37, N=3, **GEN)),
        ('k%d_gen_c40' % _key, _g(_p, _mt, cin=40, cout=40, Ho=20, Wo=36, bias=True, act=2, outs='both')),
    ]
GLDS += [
    ('k20_gen_8w', _g(1, 2, cin=64, Ho=35, Wo=37, bias=True, act=1, outs='both')),
    # the 8-wave shape (32 x 32 tiles) on an output smaller than a tile both ways: generic epilogue, and the conv5 class in both formats
    ('k20_gen_8w_small', _g(1, 2, cin=64, Ho=5, Wo=7, bias=True, act=1, outs='both', tune=13)),
    ('k20_e233_8w_small', _g(1, 2, cin=96, Ho=5, Wo=7, bias=True, res1='f32', beta1=0.2, alpha=0.04, outs='both', tune=13, conv5=True)),
    ('k20_e248_8w_small', _g(1, 2, cin=16, Ho=5, Wo=7, N=3, res1='f32', beta1=0.2, alpha=0.04, res2=True, beta2=1.0, outs='both', gamma=3.0, tune=13, conv5=True)),
    ('k2020_e233_8w_small', _g(2, 2, cin=96, Ho=5, Wo=7, bias=True, res1='f32', beta1=0.2, alpha=0.04, outs='both', tune=13, conv5=True)),
    ('k2020_e248_8w_small', _g(2, 2, cin=16, Ho=5, Wo=7, N=3, res1='f32', beta1=0.2, alpha=0.04, res2=True, beta2=1.0, outs='both', gamma=3.0, tune=13, conv5=True)),
    ('k20_e233_4w_small', _g(1, 2, cin=16, Ho=5, Wo=7, bias=True, res1='f32', beta1=0.2, alpha=0.04, outs='both', tune=12, conv5=True)),
    ('k20_gen_4w', _g(1, 2, cin=16, Ho=19, Wo=37, bias=True, act=1, mask=True, tune=12)),
    ('k20_gen_c96', _g(1, 2, cin=64, cout=96, Ho=20, Wo=36, bias=True, outs='both')),
    ('k2010_ups', _g(2, 1, cin=64, ups=1, Ho=18, Wo=38, **E67)),                                                       # nearest x2 folded into the DMA addresses
    ('k2020_ups_gen', _g(2, 2, cin=16, ups=1, Ho=10, Wo=14, bias=True, act=1, outs='both')),
]
for _t in ('sf16', 'sbf16'):
    _p = 2 if _t == 'sf16' else 1
    GLDS += [
        ('%s_fwd_split_out' % _t, _g(_p, 2, tens=_t, cin=40, cout=64, Ho=19, Wo=37, bias=True, act=1, slope=0.0, o16split=True)),
        ('%s_dgrad_c40' % _t, _g(_p, 1, tens=_t, cin=64, cout=40, Ho=20, Wo=36, mask=True, slope=0.0, o16split=True)),
        ('%s_split_res' % _t, _g(_p, 1, tens=_t, cin=16, cout=32, Ho=5, Wo=7, bias=True, res1='split', beta1=1.0, outs='both', o16split=True)),
        ('%s_f32_out' % _t, _g(_p, 1, tens=_t, cin=64, cout=3, Ho=20, Wo=36, N=3, alpha=0.125, outs='f32')),
    ]


@gpu
@pytest.mark.parametrize('name,case', GLDS, ids=[r[0] for r in GLDS])
def test_glds(name, case, margins):
    run_conv(_gpu(), margins, 'glds ' + name, 'op', **dict(case, seed=len(name)))


# conv5 of a dense block: epilogues 232 / 233 / 248 / 249 in bf16 and f16, in both workgroup shapes
@gpu
@pytest.mark.parametrize('tune', [12, 13], ids=['4waves', '8waves'])
@pytest.mark.parametrize('epi', [232, 233, 248, 249])
@pytest.mark.parametrize('kind', ['bf16', 'f16'])
def test_conv5(kind, epi, tune, margins):
    Ho, Wo = (19, 37) if tune == 12 else (35, 37)
    if epi == 249:
        Ho, Wo = (16, 32) if tune == 12 else (32, 32)
    run_conv(_gpu(), margins, 'conv5 %s e%d %d' % (kind, epi, tune), 'abi', **_g(2 if kind == 'f16' else 1, 2, cin=16 if epi == 232 else 96, Ho=Ho, Wo=Wo,
             N=3 if epi == 248 else 2, bias=bool(epi & 1), res1='f32', beta1=0.2, alpha=0.04, res2=bool(epi & 16), beta2=1.0, outs='both', gamma=1.0 if epi < 240 else 3.0,
             tune=tune, seed=epi, conv5=True))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# epilogue matrix on one family of each kernel, through both call paths
EPI = [
    ('plain_nobias', dict(bias=False)),
    ('bias_f32', dict()),
    ('lrelu_0', dict(act=1, slope=0.0, outs='both')),
    ('lrelu_02_16only', dict(act=1, slope=0.2, outs='16')),
    ('lrelu_15', dict(act=1, slope=1.5, outs='both')),                   # outside [0, 1]: the generic epilogue
    ('lrelu_m025', dict(act=1, slope=-0.25)),
    ('lrelu_sptr', dict(act=1, slope=0.3, sptr=True, outs='both')),
    ('sigmoid', dict(act=2, outs='both', gamma=0.5)),
    ('mask_pm0', dict(mask=True, slope=0.2, bias=False)),
    ('mask_15_act', dict(mask=True, act=1, slope=1.5, outs='both', gamma=3.0)),
    ('mask_sptr_m025', dict(mask=True, sptr=True, slope=-0.25, outs='16')),
    ('alpha_betas', dict(alpha=0.3, res1='f32', beta1=-1.7, res2=True, beta2=0.6, outs='both', gamma=0.5)),
    ('f16_out_g3', dict(act=1, slope=0.2, outs='both', gamma=3.0, k16='f16')),     # (the LDS-DMA families write their operand format whatever k16 says)
    ('f16_out_g1', dict(mask=True, outs='both', k16='f16')),
    ('all_terms_g3', dict(act=1, slope=0.2, mask=True, alpha=-0.7, res1='f32', beta1=1.3, res2=True, beta2=-0.4, outs='both', gamma=3.0)),
]


@gpu
@pytest.mark.parametrize('via', ['abi', 'op'])
@pytest.mark.parametrize('fam', ['reg', 'glds_bf16', 'glds_f16'])
@pytest.mark.parametrize('name,case', EPI, ids=[e[0] for e in EPI])
def test_epi(name, case, fam, via, margins):
    base = dict(prec=3, cin=40, cout=40, Ho=19, Wo=37) if fam == 'reg' else _g(2 if fam == 'glds_f16' else 1, 1, cin=40, cout=64, Ho=19, Wo=37, bias=True, outs='f32')
    run_conv(_gpu(), margins, 'epi %s %s' % (fam, name), via, **dict(base, **case, seed=len(name) + len(fam)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# out_stride = 2: the four parity sub-convs of a stride-2 data gradient (4x4 and 3x3) and of the forward sub-pixel upconv, each into its own parity of
# ONE odd-sized full-resolution tensor, mask and res1 at full resolution
def _strided_out_packs(dev, form, prec):
    from dasr_amd.dsn_model import _P3_TAPS
    from dasr_amd.gan_nets import _PARITY_PAD, _PARITY_TAPS
    from dasr_amd.rrdbnet import _SUBPIXEL_ROWS as rows
    out = {}
    for py in (0, 1):
        for px in (0, 1):
            if form == 'fwd_subpixel':      # nearest x2 + 3x3 as 2x2 convs of the low-resolution input: tap = fp32 sum of source taps
                masks = [sum(1 << (ky * 3 + kx) for ky in rows[py][a] for kx in rows[px][b]) for a in (0, 1) for b in (0, 1)]
                wt = Weights(dev, (40, 40, 3, 3), 40, 40, 4, 1, prec, 7, tapmap=[0, 0, 0, 0], src_ntaps=9, tapmasks=masks)
                out[(py, px)] = (wt, 1 - py, 1 - px)
            else:
                kh, taps, pads = (4, _PARITY_TAPS, _PARITY_PAD) if form == 'dgrad4x4' else (3, _P3_TAPS, {0: 0, 1: 0})
                tm = [(-1 if (taps[py][a] < 0 or taps[px][b] < 0) else taps[py][a] * kh + taps[px][b]) for a in (0, 1) for b in (0, 1)]
                wt = Weights(dev, (40, 24, kh, kh), 24, 40, 4, 1, prec, 7, segs=[(0, 40, 24, 0, 40, 0, 1)], tapmap=tm, src_ntaps=kh * kh)
                out[(py, px)] = (wt, pads[py], pads[px])
    return out


@gpu
@pytest.mark.parametrize('prec', [3, 4])
@pytest.mark.parametrize('form', ['dgrad4x4', 'dgrad3x3', 'fwd_subpixel'])
def test_strided_out(form, prec, margins):
    dev = _gpu()
    from dasr_amd.engine import conv_op
    N, g = 2, gen(40 + prec)
    if form == 'fwd_subpixel':
        cin, cout, hin, win = 40, 40, 9, 19
        Hf, Wf = 2 * hin, 2 * win
    else:
        cin, cout, Hf, Wf = 40, 24, 19, 37              # odd: the parity sub-grids differ in size
        kh = 4 if form == 'dgrad4x4' else 3
        hin, win = (Hf + 2 - kh) // 2 + 1, (Wf + 2 - kh) // 2 + 1
    Kin, Kout = R.planes(cin), R.planes(cout)
    x = torch.randn(N, cin, hin, win, generator=g)
    xz = torch.zeros(N, CR.c16(cin), hin, win)
    xz[:, :cin] = x
    xs = nan_slab(dev, 'f32', N, Kin, hin, win, R.pack(x, 'f32'))
    m, r1 = torch.randn(N, cout, Hf, Wf, generator=g), torch.randn(N, cout, Hf, Wf, generator=g)
    m[0, 0, 0, 0], m[0, 1, 1, 1], m[1, 2, 0, 1], m[1, 3, 1, 0] = 0.0, -0.0, 0.0, -0.0
    ms, r1s = nan_slab(dev, 'f32', N, Kout, Hf, Wf, R.pack(m, 'f32', NAN)), nan_slab(dev, 'f32', N, Kout, Hf, Wf, R.pack(r1, 'f32', NAN))
    slope, alpha, beta1 = R.f32(0.2), R.f32(0.7), R.f32(-1.3)
    packs = _strided_out_packs(dev, form, prec)
    fwd = form == 'fwd_subpixel'
    for (py, px), (wt, pad, pad_x) in packs.items():
        hs, wsub = (Hf - py + 1) // 2, (Wf - px + 1) // 2
        of = Slab(dev, 'f32', N, Kout, Hf, Wf)
        op = conv_op(wt.pack, wt.ref, xs.view(), True, CR.c16(cin), hin, win, hs, wsub, N, bias=wt.P.ptr('b') if fwd else None, kh=2, stride=1, pad=pad, pad_x=pad_x,
                     act=1 if fwd else 0, mask=ms.view(), mask_f32=1, slope=slope, alpha=alpha, res1=r1s.view(), beta1=beta1, out_f32=of.view(),
                     out_stride=2, out_oy=py, out_ox=px, out_W=Wf)
        assert launch(op, 'abi' if py else 'op') == 0
        d = CR.conv_detail(wt.eff, wt.b if fwd else None, xz, hs, wsub, prec=prec, kh=2, pad=pad, pad_x=pad_x, act=1 if fwd else 0, slope=slope, mask=m,
                           alpha=alpha, res1=r1, beta1=beta1, out_stride=2, out_oy=py, out_ox=px)
        # k: bias (1, forward), act (1, forward), mask (1), alpha (1), res1 (2)
        b32 = c_of(d['L']) * 2.0 ** -23 * d['S'] * d['gain'] + ((2 if fwd else 0) + 4) * U32 * d['terms']
        assert of.outside_untouched() and xs.untouched() and ms.untouched() and r1s.untouched()
        got = of.nchw()
        sub = got[:, :, py::2, px::2]
        bounded('conv strided_out %s p%d (%d,%d)' % (form, prec, py, px), sub[:, :cout], d['ref'], b32, margins)
        assert float(sub[:, cout:].abs().max()) == 0.0
        want = CR.scatter(torch.full_like(got, SENT), sub, 2, py, px)      # the three other parities of the output tensor: bit-unchanged
        assert biteq(got, want)


# in_stride = 2: the transposed sub-pixel parities read the parity sub-grids of the gradient in place and accumulate through res1 as
# RRDBNet._subpixel_dgrad chains them (first launch: no res1; then res1 = the output itself, beta1 = 1)
@gpu
@pytest.mark.parametrize('prec', [2, 3, 4])
def test_strided_in_chain(prec, margins):
    dev = _gpu()
    from dasr_amd.engine import conv_op
    from dasr_amd.rrdbnet import _SUBPIXEL_ROWS as rows
    N, nf, hl, wl, g = 2, 40, 9, 19, gen(50 + prec)
    K = R.planes(nf)
    xmag, in_scale = (1e-7, 4096.0) if prec != 3 else (1.0, 0.0)
    gy = torch.randn(N, nf, 2 * hl, 2 * wl, generator=g) * xmag
    gz = torch.zeros(N, CR.c16(nf), 2 * hl, 2 * wl)
    gz[:, :nf] = gy
    gs = nan_slab(dev, 'f32', N, K, 2 * hl, 2 * wl, R.pack(gy, 'f32'))
    m = torch.randn(N, nf, hl, wl, generator=g)
    m[0, 0, 0, 0], m[1, 1, 0, 0] = 0.0, -0.0
    ms = nan_slab(dev, 'f32', N, K, hl, wl, R.pack(m, 'f32', NAN))
    out = Slab(dev, 'f32', N, K, hl, wl)
    slope, prev = R.f32(0.2), None
    for py in (0, 1):
        for px in (0, 1):
            bw = [sum(1 << (ky * 3 + kx) for ky in rows[py][1 - a] for kx in rows[px][1 - b]) for a in (0, 1) for b in (0, 1)]
            wt = Weights(dev, (nf, nf, 3, 3), nf, nf, 4, 1, prec, 9, segs=[(0, nf, nf, 0, nf, 0, 1)], tapmap=[0, 0, 0, 0], src_ntaps=9, tapmasks=bw)
            op = conv_op(wt.pack, wt.ref, gs.view(), True, CR.c16(nf), hl, wl, hl, wl, N, kh=2, stride=1, pad=py, pad_x=px, mask=ms.view(), mask_f32=1, slope=slope,
                         res1=None if prev is None else out.view(), beta1=0.0 if prev is None else 1.0, out_f32=out.view(), in_stride=2, in_oy=py, in_ox=px,
                         in_W=2 * wl, in_scale=in_scale)
            assert launch(op, 'op' if py else 'abi') == 0
            # the residual of this launch is what the previous one left (padding channels: its zeros)
            d = CR.conv_detail(wt.eff, None, gz, hl, wl, prec=prec, kh=2, pad=py, pad_x=px, in_scale=in_scale, in_stride=2, in_oy=py, in_ox=px, Hin=hl, Win=wl,
                               slope=slope, mask=m, res1=None if prev is None else prev[:, :nf], beta1=1.0)
            # k: mask (1), res1 (2: the product with beta1 = 1 is exact, counted all the same)
            b32 = c_of(d['L']) * 2.0 ** -23 * d['S'] * d['gain'] + (1 + (0 if prev is None else 2)) * U32 * d['terms']
            assert out.outside_untouched() and gs.untouched() and ms.untouched()
            prev = out.nchw()
            bounded('conv strided_in p%d (%d,%d)' % (prec, py, px), prev[:, :nf], d['ref'], b32, margins)
            assert float(prev[:, nf:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _base_ops(dev):
    """two valid launches to derive the rejected ones from: an f32-tensor conv (register-staged kernel) and a bf16-tensor one (LDS-DMA kernel)"""
    from dasr_amd.engine import conv_op
    N, H, W = 2, 5, 7
    outs = [Slab(dev, 'f32', N, 2, H, W), Slab(dev, 'bf16', N, 2, H, W), Slab(dev, 'f16', N, 2, H, W)]
    x32 = nan_slab(dev, 'f32', N, 2, H, W, torch.zeros(N, 2, H, W, 16))
    x16 = nan_slab(dev, 'bf16', N, 2, H, W, torch.zeros(N, 2, H, W, 16, dtype=torch.bfloat16))
    w3, w1 = Weights(dev, (32, 32, 3, 3), 32, 32, 9, 1, 3, 3), Weights(dev, (32, 32, 3, 3), 32, 32, 9, 1, 1, 3)

    def f32op():
        return conv_op(w3.pack, w3.ref, x32.view(), True, 32, H, W, H, W, N, out_f32=outs[0].view(), out_bf16=outs[1].view())

    def b16op():
        return conv_op(w1.pack, w1.ref, x16.view(), False, 32, H, W, H, W, N, out_f32=outs[0].view(), out_bf16=outs[1].view())
    return f32op, b16op, outs, (x32, x16, w3, w1)


def _set(**kw):
    def f(p):
        for k, v in kw.items():
            setattr(p, k, v)
    return f


REJECT = [
    ('cin_24', 'f32', _set(cin=24)),
    ('kh_6', 'f32', _set(kh=6)),
    ('mt_3', 'f32', _set(mt=3)),
    ('prec4_mt2', 'f32', _set(prec=4, mt=2)),
    ('prec4_16bit_input', 'b16', _set(prec=4)),
    ('prec2_f16_tensors_kh4', 'b16', _set(prec=2, kh=4, out16_f16=1)),
    ('pad0_16bit_input', 'b16', _set(pad=0)),
    ('ups_bf16_tensors', 'b16', _set(ups=1, Hout=10, Wout=14)),
    ('mask_dtype', 'f32', lambda p: (setattr(p, 'mask', p.out_bf16), setattr(p, 'mask_f32', 0))),
    ('in_wrap_vs_cin', 'b16', _set(in_wrap=3)),
    ('out16_lo_without_16bit_output', 'b16', lambda p: (setattr(p, 'out16_lo', 2), setattr(p, 'out_bf16', type(p.out_bf16)(None, 0, 0)))),
    ('out16_f16_vs_operands', 'b16', _set(out16_f16=1)),
    ('in_stride_lds_dma', 'b16', _set(in_stride=2, in_W=14)),
]


@gpu
@pytest.mark.parametrize('name,base,mutate', REJECT, ids=[r[0] for r in REJECT])
def test_rejections(name, base, mutate):
    dev = _gpu()
    f32op, b16op, outs, keep = _base_ops(dev)
    good = f32op() if base == 'f32' else b16op()
    bad = f32op() if base == 'f32' else b16op()
    mutate(bad.conv)
    for via in ('abi', 'op'):
        assert launch(bad, via) == EINVAL, (name, via)
        assert all(o.untouched() for o in outs), name
    assert launch(good, 'abi') == 0             # ... and the launch they were derived from runs


@gpu
def test_raw_abi_zero_extension_fields_equal_the_explicit_form():
    """a caller that knows nothing of the extension fields leaves them zero (pad_x = 0, out_stride = 0, in_stride = 0, ...): for a 3x3 conv that means
    'as pad', dense output, dense input -- bit for bit the explicit form (pad_x = -1, out_stride = 1, in_stride = 1)"""
    dev = _gpu()
    from dasr_amd.engine import conv_op
    N, cin, cout, H, W = 2, 40, 40, 19, 37
    wt = Weights(dev, (cout, cin, 3, 3), cout, cin, 9, 1, 3, 5)
    x = torch.randn(N, cin, H, W, generator=gen(6))
    xs = nan_slab(dev, 'f32', N, 3, H, W, R.pack(x, 'f32'))
    res = []
    for raw in (False, True):
        of, ob = Slab(dev, 'f32', N, 3, H, W), Slab(dev, 'bf16', N, 3, H, W)
        op = conv_op(wt.pack, wt.ref, xs.view(), True, 48, H, W, H, W, N, bias=wt.P.ptr('b'), act=1, out_f32=of.view(), out_bf16=ob.view())
        if raw:
            for f in ('pad_x', 'out_stride', 'out_oy', 'out_ox', 'out_W', 'in_stride', 'in_oy', 'in_ox', 'in_W', 'in_wrap', 'out16_lo', 'res1_lo', 'out16_f16'):
                setattr(op.conv, f, 0)
            op.conv.in_scale, op.conv.slope_ptr, op.conv.prelu_part = 0.0, None, None
        assert launch(op, 'abi') == 0
        assert of.outside_untouched() and ob.outside_untouched()
        res.append((of.get(), ob.get()))
    assert biteq(res[0][0], res[1][0]) and biteq(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[0][0]).all())
