"""DSN training iteration (second hot path) on the MI355X kernels.

De_resnet generator        codes/DSN/model.py:25-55, ResidualBlock :213-224
FSD discriminator + filter codes/DSN/model.py:60-118, 173-210, 227-293
losses                     codes/DSN/loss.py:11-41, 44-107
iteration / optimisers     codes/DSN/train.py:204-285, 152-157;  checkpoint .tar layout train.py:357-376

Update order: both gradients are taken from the same pre-update graph, then D steps, then G steps (the reference's
`d_loss.backward(retain_graph=True); optimizer_d.step(); g_loss.backward()` only ran under torch 1.1 -- SURVEY 8(c)).
Perceptual term: per_type 'VGG' = MSE between vgg16.features[:31] of fake and of the bicubic LR (loss.py:119-130), the
weights coming from `vgg_state` / `vgg_path` or, offline, from a seeded random init; per_type 'LPIPS' (the reference default) =
LPIPS(alex)(fake, bicubic LR).mean() (loss.py:68-69,84,108-114; dasr_amd/lpips.py), weights from `lpips_alexnet` / `lpips_lin` or seeded.
nn.PReLU slopes are read from the parameter buffer at run time; their derivative masks use the sign of the layer
output, which equals the sign of the pre-activation while the slope stays positive (init 0.25).
Forward: split-bf16 (prec 3, ~fp32) on fp32 activations.  Backward of the generator's residual blocks (round 3, DASR_DSN_BWD16=0 restores
the fp32-tensor path): every forward conv also writes an f16 shadow of its output, the gradient stream carries an f16 shadow pre-scaled by a
power of two; the 16 data-gradient convs then are ONE f16 pass of the LDS-DMA dense-conv kernel (instead of three split-bf16 passes of the
register-staged one) and the 16 weight gradients run on the 12-wave LDS-DMA kernel.  The rounding of a gradient to 11 bits enters the
weight gradients like noise (nothing downstream is decided by it -- the PReLU masks come from the forward activations).
"""
import logging
import os
from collections import OrderedDict

import torch

from . import _lib
from ._lib import make_op
from .engine import (BTensor, ParamStore, PackRegistry, OpList, WgradGroup, WgradGroup3, Workspace, conv_op, ceil_div, ensure_runtime_ready, _stream,
                     patch, set_reduce_scale, dp_world, F32, SPLIT)
from .gan_nets import (NLayerDiscriminatorHIP, BatchNormDiscriminatorHIP, VGGFeatureHIP, FreqSplit, VGG16_CFG, fsd_spec, dsn_nld_spec, fold_batchnorm_fsd,
                       gaussian_kernel2d)
from .models import AdamHIP
from .dasr_model import vgg_random_state_dict, _ragan_ops

logger = logging.getLogger('base')
EPS = 1e-8


def deresnet_spec(n_res_blocks=8, scale=4):
    """scale 4: De_resnet (codes/DSN/model.py:25-57); scale 1: `Generator` (--generator DSGAN, model.py:7-22): the same net without the two
    stride-2 convs, applied to the bicubic LR image"""
    spec = [('block_input.0.weight', (64, 3, 3, 3)), ('block_input.0.bias', (64,)), ('block_input.1.weight', (1,))]
    for k in range(n_res_blocks):
        p = 'res_blocks.%d.' % k
        spec += [(p + 'conv1.weight', (64, 64, 3, 3)), (p + 'conv1.bias', (64,)), (p + 'prelu.weight', (1,)),
                 (p + 'conv2.weight', (64, 64, 3, 3)), (p + 'conv2.bias', (64,))]
    if scale == 4:
        spec += [('down_sample.0.weight', (64, 64, 3, 3)), ('down_sample.0.bias', (64,)), ('down_sample.1.weight', (1,)),
                 ('down_sample.2.weight', (64, 64, 3, 3)), ('down_sample.2.bias', (64,)), ('down_sample.3.weight', (1,))]
    spec += [('block_output.weight', (3, 64, 3, 3)), ('block_output.bias', (3,))]
    return spec


def default_init_state(spec, bn_prefixes=()):
    """nn.Conv2d / nn.PReLU / nn.BatchNorm2d default initialisation in construction order (codes/DSN/train.py:77 seeds torch with 0)"""
    import math
    from torch.nn import init
    sd = OrderedDict()
    i = 0
    while i < len(spec):
        k, shape = spec[i]
        if k.startswith(tuple(bn_prefixes)) and bn_prefixes:   # BatchNorm2d: weight 1, bias 0 (no RNG draw)
            sd[k] = torch.ones(shape) if k.endswith('.weight') else torch.zeros(shape)
            i += 1
            continue
        if len(shape) == 1 and k.endswith('.weight'):  # PReLU
            sd[k] = torch.full(shape, 0.25)
            i += 1
            continue
        if 'gaussian_filter' in k:  # bias-free depthwise conv: its default init draws from the RNG before being overwritten
            init.kaiming_uniform_(torch.empty(shape), a=math.sqrt(5))
            sd[k] = gaussian_kernel2d(shape[-1]).view(1, 1, shape[-1], shape[-1]).repeat(shape[0], 1, 1, 1)
            i += 1
            continue
        w = torch.empty(shape)
        init.kaiming_uniform_(w, a=math.sqrt(5))
        sd[k] = w
        i += 1
        if i < len(spec) and spec[i][0] == k[:-len('weight')] + 'bias':   # (the BatchNorm-ed convs of the nld discriminators have none: model.py:139-142)
            fan_in = shape[1] * shape[2] * shape[3]
            b = torch.empty(spec[i][1])
            init.uniform_(b, -1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))
            sd[spec[i][0]] = b
            i += 1
    return sd


# stride-2 3x3 (pad 1) data-gradient as 2-tap parity sub-convs: parity -> (source tap for a=0, a=1), -1 = no tap
_P3_TAPS = {0: (1, -1), 1: (2, 0)}


class DeResnetHIP:
    def __init__(self, n_res_blocks=8, device='cuda', scale=4, fwd_mode=None):
        assert scale in (1, 4)
        self.nb, self.device, self.scale = n_res_blocks, torch.device(device), scale
        self.spec = deresnet_spec(n_res_blocks, scale)
        self.params = ParamStore(self.spec, self.device)
        self.pack = PackRegistry(self.params)
        P = self.params
        self.pk = {}

        def fb(name, key, cout, cin, stride=1):
            w = P.off(key + 'weight')
            self.pk[name] = self.pack.add(cout, ceil_div(cin, 16) * 16, 9, 1, 3, [(w, cout, cin, 0, cin, 0, 0)])
            cb = ceil_div(cout, 16) * 16
            if stride == 1:
                self.pk[name + '_b'] = self.pack.add(cin, cb, 9, 1, 3, [(w, cout, cin, 0, cout, 0, 1)])
            else:
                for py in (0, 1):
                    for px in (0, 1):
                        tm = [(-1 if (_P3_TAPS[py][a] < 0 or _P3_TAPS[px][b] < 0) else _P3_TAPS[py][a] * 3 + _P3_TAPS[px][b])
                              for a in (0, 1) for b in (0, 1)]
                        self.pk[(name + '_b', py, px)] = self.pack.add(cin, cb, 4, 1, 3, [(w, cout, cin, 0, cout, 0, 1)], tapmap=tm, src_ntaps=9)

        fb('in', 'block_input.0.', 64, 3)
        for k in range(n_res_blocks):
            fb('r%d_1' % k, 'res_blocks.%d.conv1.' % k, 64, 64)
            fb('r%d_2' % k, 'res_blocks.%d.conv2.' % k, 64, 64)
        if scale == 4:
            fb('d0', 'down_sample.0.', 64, 64, 2)
            fb('d2', 'down_sample.2.', 64, 64, 2)
        fb('out', 'block_output.', 3, 64)
        self.bwd16 = os.environ.get('DASR_DSN_BWD16', '1') != '0'
        # forward of the input conv and of the residual blocks on SPLIT f16 tensors (f16 hi planes + f16 remainder planes: 22-bit operands instead of
        # split-bf16's 16, one launch of the LDS-DMA kernel over 3K virtual chunks instead of three register-staged passes); the hi planes are the
        # f16 shadows the 16-bit backward reads.  7.14 -> 6.88 ms per iteration (the generic epilogue and three MFMA passes remain).
        # DASR_DSN_FWD16=0: fp32 tensors + separate shadows.
        # Round 5 (the split forward sits at 4.7e-7 on the activations against a 1e-3 budget and pays three MFMA passes for it):
        # DASR_DSN_FWD16=2 -- the residual blocks in ONE f16 pass, exactly as the RRDB trunk runs its dense blocks: the residual stream s[k] stays fp32
        # (conv2 adds its fp32 input and writes fp32 + an f16 shadow), conv1 / conv2 read the f16 shadows (11-bit operands, fp32 accumulation).
        # MEASURED (profiles/r05_dsn_onepass.txt): iteration 6.6 -> 5.6 ms (LPIPS term), activations 2.4e-5 (budget 1e-3) -- but the GRADIENTS move to
        # 0.4 - 1.6e-2 of the fp32 oracle (configs[4] exactly: 4.7e-3; the reference's 2 x 128^2 fixtures: up to 1.6e-2, over the 1e-2 budget): an
        # activation that is off by 2e-4 flips the sign of ~1e-4 of the PReLU pre-activations, every flip changes a local derivative by 75 %, and a weight
        # gradient is a sum of random-signed terms, so the flips enter like sqrt(fraction).  With the split forward the stored f16 shadows are roundings of
        # accurate values and keep every sign.  So the split forward (1) STAYS THE DEFAULT and the one-pass forward is an opt-in (tested at configs[4]).
        fm = os.environ.get('DASR_DSN_FWD16', '1') if fwd_mode is None else str(fwd_mode)
        if fm not in ('0', '1', '2'):
            raise ValueError('DASR_DSN_FWD16 must be 0 (fp32 tensors), 1 (split f16 tensors, three passes) or 2 (one f16 pass)')
        self.fwd16 = self.bwd16 and fm == '1'
        self.fwd1p = self.bwd16 and fm == '2'
        if self.fwd1p:
            for k in range(n_res_blocks):
                for j in (1, 2):
                    w = P.off('res_blocks.%d.conv%d.weight' % (k, j))
                    self.pk['r%d_%d_f' % (k, j)] = self.pack.add(64, 64, 9, 2, 2, [(w, 64, 64, 0, 64, 0, 0)])
        if self.fwd16:
            w = P.off('block_input.0.weight')
            self.pk['in_s'] = self.pack.add(64, 48, 9, 2, 5, [(w, 64, 3, 0, 3, 0, 0)])
            for k in range(n_res_blocks):
                for j in (1, 2):
                    w = P.off('res_blocks.%d.conv%d.weight' % (k, j))
                    self.pk['r%d_%d_s' % (k, j)] = self.pack.add(64, 192, 9, 2, 5, [(w, 64, 64, 0, 64, 0, 0)])
        if self.bwd16:   # data gradient of the residual-block convs: one f16 pass on 16-bit tensors
            for k in range(n_res_blocks):
                for j in (1, 2):
                    w = P.off('res_blocks.%d.conv%d.weight' % (k, j))
                    self.pk['r%d_%d_b16' % (k, j)] = self.pack.add(64, 64, 9, 2, 2, [(w, 64, 64, 0, 64, 0, 1)])
        self.pack.finalize()
        self.plans = {}

    def repack(self):
        self.pack.run()

    def state_dict(self):
        return self.params.state_dict()

    def load_state_dict(self, sd, strict=True):
        self.params.load_state_dict(sd, strict)
        self.repack()

    def plan(self, N, H, W):
        k = (N, H, W)
        if k not in self.plans:
            self.plans[k] = _GPlan(self, N, H, W)
        return self.plans[k]


class _GPlan:
    def __init__(self, net, N, H, W):
        assert net.scale == 1 or (H % 4 == 0 and W % 4 == 0)
        self.net, self.N = net, N
        dev, P, pack, pk, nb = net.device, net.params, net.pack, net.pk, net.nb
        down = net.scale == 4
        H2, W2, H4, W4 = (H // 2, W // 2, H // 4, W // 4) if down else (H, W, H, W)
        B = lambda C_, h, w: BTensor(N, C_, h, w, True, dev)
        self.x_nchw = torch.zeros((N, 3, H, W), dtype=torch.float32, device=dev)
        self.fake_nchw = torch.zeros((N, 3, H4, W4), dtype=torch.float32, device=dev)
        self.x_in = B(16, H, W)
        f16w = net.fwd16
        # (split forward: only s[0] -- PReLU' of the input conv at the end of the backward -- and s[nb] -- input of the f32 stride-2 convs -- exist in fp32)
        self.s = [B(64, H, W) if (not f16w or k in (0, nb)) else None for k in range(nb + 1)]   # (one f16 pass, net.fwd1p: every level -- the fp32 residual stream)
        self.h = [B(64, H, W) if not (f16w or net.fwd1p) else None for _ in range(nb)]
        self.fake = B(16, H4, W4)
        self.g_fake, self.gz_out = B(16, H4, W4), B(16, H4, W4)
        if down:
            self.d1, self.d2 = B(64, H2, W2), B(64, H4, W4)
            self.g_d2, self.g_d1 = B(64, H4, W4), B(64, H2, W2)
        self.g_s = [B(64, H, W) for _ in range(2)]
        self.g_h = B(64, H, W)
        b16 = net.bwd16
        if b16:
            import math
            B16 = lambda: BTensor(N, 64, H, W, False, dev, f16=True)
            BS = lambda C_: SPLIT.alloc(N, C_, H, W, dev)   # split tensor: hi planes, then remainder planes
            if f16w:   # (view() of a split tensor = its hi planes: the 16-bit shadow)
                self.x_s = BS(16)
                self.s16 = [BS(64) for _ in range(nb)]
                self.h16 = [BS(64) for _ in range(nb)]
            else:   # (one f16 pass: also a shadow of level nb -- nobody reads it, but conv2 of the last block then runs the same compile-time epilogue as the others)
                self.s16 = [B16() for _ in range(nb + (1 if net.fwd1p else 0))]       # f16 shadows of the residual stream s[0 .. nb-1] and of the block-internal activations
                self.h16 = [B16() for _ in range(nb)]
            # gscale * dL/ds[j] (j = 0 .. nb) and gscale * dL/dh[k] in f16: ONE buffer per level (round 4), so that the 2 nb weight gradients of the
            # residual blocks run as ONE grouped launch behind the data-gradient chain (16 parts x 16 pixel splits instead of 16 launches of
            # 1 part x 256 splits: a sixteenth of the partial-sum traffic, one reduce instead of sixteen); 2 nb x 67 MB at batch 8 x 256^2
            self.g_s16 = [None] + [B16() for j in range(1, nb + 1)]   # (level 0 has no 16-bit consumer: not allocated, not written -- ADVICE r05: 67 MB and one store stream at 8 x 256^2)
            self.g_h16 = [B16() for _ in range(nb)]
            # dL/dfake of the mean losses is ~(largest loss weight) / (number of output elements): a power of two puts it at ~2^-3 before the f16
            # rounding.  net.loss_weight = max(w_col, w_tex, w_per) (set by DSNModel; 1 for a bare generator): with w_col = 0 the gradient is
            # 2-3 orders smaller and would otherwise sit in f16's subnormal range (the non-finite flag only sees overflow)
            lw = float(getattr(net, 'loss_weight', 1.0)) or 1.0
            self.gscale = float(2.0 ** max(0, min(60, int(math.floor(math.log2(max(1.0, N * 3 * H4 * W4 / lw)))) - 3)))
        sh = lambda t: ({'out_bf16': t.view(), 'out16_f16': 1} if b16 else {})
        self.scratch = torch.zeros(1024, dtype=torch.float32, device=dev)
        self.ws = Workspace(dev)
        sp = lambda key: P.ptr(key)
        # ---- forward ----
        f = OpList()
        f.add(make_op(_lib.OP_NCHW2B, src=self.x_nchw.data_ptr(), N=N, C=3, H=H, W=W, dst_f32=self.x_in.view()))
        if f16w and nb:
            f.add(make_op(_lib.OP_CVT_F16, x=self.x_in.view(), N=N, C=16, H=H, W=W, scale=1.0, y=self.x_s.view(), form=SPLIT.cvt_form))
            f.add(conv_op(pack, pk['in_s'], Hin=H, Win=W, Hout=H, Wout=W, N=N, **SPLIT.conv_in(self.x_s, 16), bias=sp('block_input.0.bias'), act=1,
                          slope_ptr=sp('block_input.1.weight'), out_f32=self.s[0].view(), **SPLIT.conv_out(self.s16[0], 64)))
        else:
            f.add(conv_op(pack, pk['in'], self.x_in.view(), True, 16, H, W, H, W, N, bias=sp('block_input.0.bias'), act=1,
                          slope_ptr=sp('block_input.1.weight'), out_f32=self.s[0].view(), **(sh(self.s16[0]) if (b16 and nb) else {})))
        for k in range(nb):
            pre = 'res_blocks.%d.' % k
            if net.fwd1p:   # one f16 pass per conv on the f16 shadows; fp32 residual stream
                f.add(conv_op(pack, pk['r%d_1_f' % k], self.s16[k].view(), False, 64, H, W, H, W, N, bias=sp(pre + 'conv1.bias'), act=1,
                              slope_ptr=sp(pre + 'prelu.weight'), out_bf16=self.h16[k].view(), out16_f16=1))
                f.add(conv_op(pack, pk['r%d_2_f' % k], self.h16[k].view(), False, 64, H, W, H, W, N, bias=sp(pre + 'conv2.bias'),
                              res1=self.s[k].view(), beta1=1.0, out_f32=self.s[k + 1].view(),
                              out_bf16=self.s16[k + 1].view(), out16_f16=1))
                continue
            if f16w:
                last_blk = k + 1 == nb
                hw = dict(Hin=H, Win=W, Hout=H, Wout=W, N=N)
                f.add(conv_op(pack, pk['r%d_1_s' % k], **hw, **SPLIT.conv_in(self.s16[k], 64), bias=sp(pre + 'conv1.bias'), act=1,
                              slope_ptr=sp(pre + 'prelu.weight'), **SPLIT.conv_out(self.h16[k], 64)))
                # (the last block writes the f32 s[nb]; out16_f16 stays set on that launch: inherited)
                out = dict(F32.conv_out(self.s[nb], 64), out16_f16=1) if last_blk else SPLIT.conv_out(self.s16[k + 1], 64)
                f.add(conv_op(pack, pk['r%d_2_s' % k], **hw, **SPLIT.conv_in(self.h16[k], 64), bias=sp(pre + 'conv2.bias'),
                              beta1=1.0, **SPLIT.conv_res(self.s16[k], 64), **out))
                continue
            f.add(conv_op(pack, pk['r%d_1' % k], self.s[k].view(), True, 64, H, W, H, W, N, bias=sp(pre + 'conv1.bias'), act=1,
                          slope_ptr=sp(pre + 'prelu.weight'), out_f32=self.h[k].view(), **sh(self.h16[k] if b16 else None)))
            f.add(conv_op(pack, pk['r%d_2' % k], self.h[k].view(), True, 64, H, W, H, W, N, bias=sp(pre + 'conv2.bias'),
                          res1=self.s[k].view(), beta1=1.0, out_f32=self.s[k + 1].view(), **(sh(self.s16[k + 1]) if (b16 and k + 1 < nb) else {})))
        if down:
            f.add(conv_op(pack, pk['d0'], self.s[nb].view(), True, 64, H, W, H2, W2, N, bias=sp('down_sample.0.bias'), stride=2, act=1,
                          slope_ptr=sp('down_sample.1.weight'), out_f32=self.d1.view()))
            f.add(conv_op(pack, pk['d2'], self.d1.view(), True, 64, H2, W2, H4, W4, N, bias=sp('down_sample.2.bias'), stride=2, act=1,
                          slope_ptr=sp('down_sample.3.weight'), out_f32=self.d2.view()))
        last = self.d2 if down else self.s[nb]
        f.add(conv_op(pack, pk['out'], last.view(), True, 64, H4, W4, H4, W4, N, bias=sp('block_output.bias'), act=2,
                      out_f32=self.fake.view()))
        f.add(make_op(_lib.OP_B2NCHW, src=self.fake.view(), N=N, C=3, H=H4, W=W4, dst=self.fake_nchw.data_ptr()))
        self.fwd = f.tag(1)
        # ---- backward (input: g_fake = dL/d fake) ----
        b = OpList()
        G = P.grad.data_ptr()

        def wg(key, g, inp, cout, cin, hi, wi, ho, wo, stride=1):
            grp = WgradGroup(3, stride)
            grp.add_conv(g.view, True, g.planes, inp.view, True, inp.planes, cout, cin, hi, wi, ho, wo, N, P.off(key + 'weight'), P.off(key + 'bias'))
            grp.emit(b, self.ws, dev, G)

        def prelu_grad(key, y, gx, h, w, f16=False):
            o = make_op(_lib.OP_PRELU_GRAD, y=y.view(), gx=gx.view(), N=N, C=64, H=h, W=w, slope=sp(key), scratch256=self.scratch.data_ptr(),
                        dst=P.ptr(key, P.grad), scale=1.0)
            if f16:   # f16 shadows: the gradient carries gscale
                o.set('f16', 1)
                o.set('inv_prescale', 1.0 / self.gscale)
            b.add(o)
            self._prelu_ops.append(o)

        def dgrad_s2(name, g, out, mask, slope_key, hi, wi, ho, wo):
            for py in (0, 1):
                for px in (0, 1):
                    hs, wsub = (hi - py + 1) // 2, (wi - px + 1) // 2
                    b.add(conv_op(pack, pk[(name + '_b', py, px)], g.view(), True, 64, ho, wo, hs, wsub, N, kh=2, stride=1, pad=0, pad_x=0,
                                  mask=mask.view() if mask is not None else None, mask_f32=1,
                                  slope_ptr=sp(slope_key) if slope_key else None, out_f32=out.view(), out_stride=2, out_oy=py, out_ox=px,
                                  out_W=wi))

        self._prelu_ops = []
        self._prelu_final = None
        b.add(make_op(_lib.OP_SIGMOID_BWD, y=self.fake.view(), g=self.g_fake.view(), N=N, C=3, H=H4, W=W4, gz=self.gz_out.view()))
        wg('block_output.', self.gz_out, last, 3, 64, H4, W4, H4, W4)
        gs = self.g_s[0]
        if down:
            b.add(conv_op(pack, pk['out_b'], self.gz_out.view(), True, 16, H4, W4, H4, W4, N, mask=self.d2.view(), mask_f32=1,
                          slope_ptr=sp('down_sample.3.weight'), out_f32=self.g_d2.view()))
            prelu_grad('down_sample.3.weight', self.d2, self.g_d2, H4, W4)
            wg('down_sample.2.', self.g_d2, self.d1, 64, 64, H2, W2, H4, W4, stride=2)
            dgrad_s2('d2', self.g_d2, self.g_d1, self.d1, 'down_sample.1.weight', H2, W2, H4, W4)
            prelu_grad('down_sample.1.weight', self.d1, self.g_d1, H2, W2)
            wg('down_sample.0.', self.g_d1, self.s[nb], 64, 64, H, W, H2, W2, stride=2)
            dgrad_s2('d0', self.g_d1, gs, None, None, H, W, H2, W2)
        else:   # Generator (DSGAN): the output conv reads the residual stream directly (no activation in between)
            b.add(conv_op(pack, pk['out_b'], self.gz_out.view(), True, 16, H, W, H, W, N, out_f32=gs.view()))
        if b16 and nb:   # gscale * dL/ds[nb] in f16
            b.add(make_op(_lib.OP_CVT_F16, x=gs.view(), N=N, C=64, H=H, W=W, scale=self.gscale, y=self.g_s16[nb].view()))
        wgrp = None
        if b16 and nb:
            wgrp = WgradGroup3()
            wgrp.f16, wgrp.g_scale = True, self.gscale

        def wg16_part(key, g16, inp16):
            """weight gradient of a 64 -> 64 conv from the f16 shadows (g16 holds gscale * dL/dy) as one part of the grouped launch: the 64 input
            channels x the two 32-oc tiles"""
            tiles = [dict(dst_w_off=P.off(key + 'weight'), dst_b_off=P.off(key + 'bias'), cout=64, cin=64, oc0=oc0, c0=0, n_ctiles=2) for oc0 in (0, 32)]
            wgrp.add_block(g16.view(), 4, inp16.view(), 4, 2, H, W, H, W, N, tiles, want_bias=True)
            wgrp.flops += 2.0 * N * H * W * 9 * 64 * 64

        # PReLU-slope gradients of the residual blocks (round 6): the data-gradient conv through conv2 holds dL/dh (its result) and h (its mask) in its epilogue and leaves
        # one partial of sum_{h <= 0} dL/dh * h per workgroup (dasr_conv_params::prelu_part); ONE dasr_prelu_final launch behind the chain finishes all nb slopes --
        # instead of a second pass over h and dL/dz per block (dasr_prelu_grad_f16: 2 x 67 MB and two launches each at batch 8 x 256^2).  DASR_DSN_PRELU_FUSED=0: the old form.
        fuse_prelu = b16 and nb > 0 and os.environ.get('DASR_DSN_PRELU_FUSED', '1') != '0'
        if fuse_prelu:
            self.prelu_nblk = N * ceil_div(H, 4) * ceil_div(W, 16)   # >= the workgroups of any tile shape a conv launch may take (16 x 32 ... 4 x 32 pixels); unowned entries stay zero
            self.prelu_part = torch.zeros(nb * self.prelu_nblk, dtype=torch.float32, device=dev)
        for k in range(nb - 1, -1, -1):
            pre = 'res_blocks.%d.' % k
            if b16:
                inv = 1.0 / self.gscale
                gs16, g_h16 = self.g_s16[k + 1], self.g_h16[k]
                wg16_part(pre + 'conv2.', gs16, self.h16[k])
                o = conv_op(pack, pk['r%d_2_b16' % k], gs16.view(), False, 64, H, W, H, W, N, mask=self.h16[k].view(), mask_f32=0,
                            slope_ptr=sp(pre + 'prelu.weight'), out_bf16=g_h16.view(), out16_f16=1)   # (gscale * dL/ds in, gscale * dL/dh out: no rescaling)
                if fuse_prelu:
                    o.conv.prelu_part = self.prelu_part.data_ptr() + 4 * k * self.prelu_nblk
                b.add(o)
                if not fuse_prelu:
                    prelu_grad(pre + 'prelu.weight', self.h16[k], g_h16, H, W, f16=True)   # (dL/dh is never materialised in f32)
                wg16_part(pre + 'conv1.', g_h16, self.s16[k])
                nxt = self.g_s[1] if gs is self.g_s[0] else self.g_s[0]
                b.add(conv_op(pack, pk['r%d_1_b16' % k], g_h16.view(), False, 64, H, W, H, W, N, alpha=inv, res1=gs.view(), beta1=1.0,
                              out_f32=nxt.view(), out_bf16=self.g_s16[k].view() if k > 0 else None, out16_f16=1, gamma=self.gscale))
                gs = nxt
                continue
            wg(pre + 'conv2.', gs, self.h[k], 64, 64, H, W, H, W)
            b.add(conv_op(pack, pk['r%d_2_b' % k], gs.view(), True, 64, H, W, H, W, N, mask=self.h[k].view(), mask_f32=1,
                          slope_ptr=sp(pre + 'prelu.weight'), out_f32=self.g_h.view()))
            prelu_grad(pre + 'prelu.weight', self.h[k], self.g_h, H, W)
            wg(pre + 'conv1.', self.g_h, self.s[k], 64, 64, H, W, H, W)
            nxt = self.g_s[1] if gs is self.g_s[0] else self.g_s[0]
            b.add(conv_op(pack, pk['r%d_1_b' % k], self.g_h.view(), True, 64, H, W, H, W, N, res1=gs.view(), beta1=1.0, out_f32=nxt.view()))
            gs = nxt
        if fuse_prelu:
            keys = ['res_blocks.%d.prelu.weight' % k for k in range(nb)]
            self.prelu_slopes = torch.tensor([sp(k_) for k_ in keys], dtype=torch.int64, device=dev)
            self.prelu_dsts = torch.tensor([P.ptr(k_, P.grad) for k_ in keys], dtype=torch.int64, device=dev)
            self._prelu_final = make_op(_lib.OP_PRELU_FINAL, partial=self.prelu_part.data_ptr(), nblocks=self.prelu_nblk, stride=self.prelu_nblk, count=nb,
                                        slopes=self.prelu_slopes.data_ptr(), dsts=self.prelu_dsts.data_ptr(), scale=1.0 / self.gscale)
            b.add(self._prelu_final)
            b.keep += [self.prelu_part, self.prelu_slopes, self.prelu_dsts]
        if wgrp is not None:   # all 2 nb residual-block weight gradients: one launch of 2 nb parts, one reduce
            wgrp.emit(b, self.ws, dev, G)
        # s[0] = PReLU(conv_in(x)): apply PReLU' to dL/ds0, then the input conv's weight gradient
        b.add(make_op(_lib.OP_AXPBY, x=gs.view(), a=1.0, N=N, C=64, H=H, W=W, out_f32=self.g_h.view(), gamma=1.0, mask=self.s[0].view(), slope=0.25,
                      slope_ptr=sp('block_input.1.weight')))
        prelu_grad('block_input.1.weight', self.s[0], self.g_h, H, W)
        wg('block_input.0.', self.g_h, self.x_in, 64, 3, H, W, H, W)
        self.bwd = b.tag(4)
        self.ws.finalize()

    def set_grad_scale(self, scale):
        set_reduce_scale([self.bwd], scale)
        for o in self._prelu_ops:
            patch(o, scale=scale)
        if getattr(self, '_prelu_final', None) is not None:   # (the fused form: data-parallel factor x 1 / pre-scale of the 16-bit backward)
            patch(self._prelu_final, scale=scale / self.gscale)


def symmetry_code(k_rot, flip_rows, flip_cols):
    """torch.flip(torch.flip(torch.rot90(x, k_rot, [2, 3]), rows?), cols?) as ONE of the 8 symmetries of the square in dasr_lpips_s2d's encoding:
    T(x)[i][j] = x[u][v], (u, v) = (i, j) swapped if bit 0, then u -> H-1-u if bit 1, v -> W-1-v if bit 2.  Found by matching on an index grid."""
    idx = torch.arange(9).reshape(1, 1, 3, 3)
    t = torch.rot90(idx, k_rot, [2, 3])
    if flip_rows:
        t = torch.flip(t, (2,))
    if flip_cols:
        t = torch.flip(t, (3,))
    for code in range(8):
        got = torch.empty(3, 3, dtype=torch.long)
        for i in range(3):
            for j in range(3):
                u, v = (j, i) if code & 1 else (i, j)
                u = 2 - u if code & 2 else u
                v = 2 - v if code & 4 else v
                got[i, j] = idx[0, 0, u, v]
        if torch.equal(got, t[0, 0]):
            return code
    raise AssertionError('not a symmetry of the square')


def draw_symmetry():
    """PerceptualLoss.forward (codes/DSN/loss.py:155-168): k_rot, then the two flip coins, from python's global `random` in that order"""
    import random
    k_rot = random.choice([-1, 0, 1])
    rows = random.choice([True, False])
    cols = random.choice([True, False])
    return symmetry_code(k_rot, rows, cols)


class DSNModel:
    """iteration(hr, bicubic_lr, real_lr) / end_epoch() / save(path) / load(path)"""

    def __init__(self, opt=None, device=None, **kw):
        o = dict(n_res_blocks=8, kernel_size=5, filter='gau', norm_layer='Instance', discriminator='FSD', generator='DeResnet', learning_rate=1e-4,
                 adam_beta_1=0.5, w_col=1.0, w_tex=0.005, w_per=0.01, per_type='VGG', vgg_path=None, vgg_seed=78, num_epochs=400,
                 num_decay_epochs=150, upscale_factor=4, ragan=False, allow_random_perceptual=False, cat_or_sum='cat', disc_freq=1, gen_freq=1, lpips_rot_flip=False, wgan=False)
        o.update(opt or {})
        o.update(kw)
        self.opt = o
        ensure_runtime_ready()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.d_arch = o['discriminator'].lower()
        if self.d_arch not in ('fsd', 'nld_s1', 'nld_s2'):
            raise NotImplementedError('Discriminator architecture [{:s}] not recognized'.format(o['discriminator']))
        if o['upscale_factor'] != 4:
            raise NotImplementedError('DSN on MI355X: De_resnet x4 / DSGAN generators (--upscale_factor 4)')
        if o['norm_layer'] not in ('Instance', 'Batch'):
            raise NotImplementedError('Norm layer [{:s}] not recognized'.format(str(o['norm_layer'])))   # model.py:136-137,191
        # norm_layer 'Batch' (FSD: model.py:176-189; nld_s1 / nld_s2: model.py:136-160, bias-free convs): iteration() runs BatchNorm in training mode (statistics per discriminator call = per half
        # [fake | real], as the reference's two calls); translate() / ddm_of() run it in eval mode: a conv-only copy with the running statistics
        # folded in (refreshed when the weights changed)
        self.bn = o['norm_layer'] == 'Batch'
        self.netF = None
        if o['w_per'] > 0:
            if o['per_type'] == 'LPIPS':      # PerceptualLoss() = LPIPS(alex) on the LR-size images (loss.py:68-69,84,108-114)
                from .lpips import load_lpips
                self.netF = load_lpips({'path': {'lpips_alexnet': o.get('lpips_alexnet'), 'lpips_lin': o.get('lpips_lin')},
                                        'allow_random_perceptual': o['allow_random_perceptual']}, self.device, int(o['vgg_seed']))
            elif o['per_type'] == 'VGG':
                self.netF = VGGFeatureHIP(30, device=self.device, cfg=VGG16_CFG, mse_target=True)   # loss.py:58-63: MSE of VGG16 features
                if o['vgg_path']:
                    sd = torch.load(o['vgg_path'], map_location='cpu')
                    self.netF.load_state_dict({k: v for k, v in sd.items() if k in self.netF.params.spec})
                elif o['allow_random_perceptual']:
                    logger.warning('allow_random_perceptual: the VGG16 perceptual net uses SEEDED RANDOM weights (torchvision init rule), no vgg_path')
                    self.netF.load_state_dict(vgg_random_state_dict(self.netF.spec, int(o['vgg_seed'])))
                else:   # the reference always runs torchvision's pretrained vgg16 (loss.py:47-63); it cannot be downloaded offline
                    raise FileNotFoundError('--per_type VGG needs pretrained VGG16 weights: --vgg_path (torchvision vgg16 state_dict), or '
                                            '--allow_random_perceptual to train against a seeded random network')
            else:
                raise NotImplementedError('{} is not recognized'.format(o['per_type']))
        # --disc_freq / --gen_freq (codes/DSN/train.py:55-56, 206, 229, 251): the counter advances at the top of an iteration, a network steps when
        # the counter is a multiple of its frequency (forward, losses and BatchNorm running statistics happen every iteration)
        self.disc_freq, self.gen_freq = int(o['disc_freq']), int(o['gen_freq'])
        if self.disc_freq < 1 or self.gen_freq < 1:
            raise ValueError('disc_freq / gen_freq must be >= 1')
        self.ragan = bool(o['ragan'])   # --ragan (train.py:221-223): D(x, y) = sigmoid(D(x) - mean_n D(y)) (model.py:98-106)
        # --wgan (train.py:45,231-241; model.py:104-105; loss.py:18-19,33-36): no sigmoid, Wasserstein terms -mean(real) + mean(fake), generator term
        # mean(-fake), gradient penalty 10 (||d mean D(sample) / d sample|| - 1)^2 with its second-order pass through the discriminator (_GradPenaltyPlan)
        self.wgan = bool(o['wgan'])
        # --wgan with --ragan (train.py:221-236, model.py:98-106): without the sigmoid the relativistic terms are linear in the logits, the per-pixel batch
        # means only shift them: -mean(real_tex) + mean(fake_tex) = 2 (mean D(fake) - mean D(real)), mean(-fake_tex) = -mean D(fake) + mean D(real), the
        # gradient penalty sees D(sample) alone.  So the combination is the --wgan plan with the discriminator's Wasserstein gradients doubled and the
        # logged terms recombined (get_current_log); `rel` = the three-stage sigmoid form of --ragan alone
        self.rel = self.ragan and not self.wgan
        # frequency separation: --filter, --kernel_size and the wavelet bands of the discriminator input, --cat_or_sum: 'cat' (9 channels) or
        # 'sum' = (LH + HL + HH) / 3 (model.py:108-118)
        self.filter, self.k, self.cs = o['filter'].lower(), o['kernel_size'], str(o['cat_or_sum']).lower()
        self.freq = FreqSplit.dsn(self.filter, self.k, self.cs, self.device)
        if o['generator'].lower() not in ('deresnet', 'dsgan'):   # codes/DSN/train.py:124-129
            raise NotImplementedError('Generator model [{:s}] not recognized'.format(o['generator']))
        self.netG = DeResnetHIP(o['n_res_blocks'], device=self.device, scale=4 if o['generator'].lower() == 'deresnet' else 1)
        # --lpips_rot_flip (train.py:52, loss.py:66,149-168): a random symmetry of the square on both LPIPS inputs, drawn from python's `random` per
        # generator-loss evaluation in the reference's order; only PerceptualLoss (= per_type LPIPS) has it, the VGG16 term ignores the flag
        self.lpips_rot_flip = bool(o['lpips_rot_flip']) and o['per_type'] == 'LPIPS' and o['w_per'] > 0
        self.netG.loss_weight = max(float(o['w_col']), float(o['w_tex']), float(o['w_per']))   # sizes the f16 pre-scale of the 16-bit backward (_GPlan.gscale)
        nc = self.freq.in_nc
        gk = self.k if self.filter == 'gau' else None
        self.netD_eval = None
        if self.d_arch == 'fsd':
            spec_layers = fsd_spec(nc, gk, norm='Batch' if self.bn else 'Instance')
        else:   # codes/DSN/model.py:84-89: NLayerDiscriminator(n_layers=2) with stride 1 / 2
            spec_layers = dsn_nld_spec(nc, 1 if self.d_arch == 'nld_s1' else 2, gk, norm='Batch' if self.bn else 'Instance')
        # default nn init, G first then D (codes/DSN/train.py:124-135 under torch.manual_seed(0))
        self.netG.load_state_dict(default_init_state(self.netG.spec))
        if self.bn:
            self.netD = BatchNormDiscriminatorHIP(nc, device=self.device, spec_layers=spec_layers)
            sd = default_init_state(self.netD.spec, bn_prefixes=[L['bn'] for L in self.netD.layers if L['norm'] == 'batch'])
            sd.update({k: v.clone() for k, v in self.netD.buffers.items()})
            self.netD.load_state_dict(sd)
            self.netD_eval = NLayerDiscriminatorHIP(nc, device=self.device, spec_layers=(
                fsd_spec(nc, gk, norm='BatchEval') if self.d_arch == 'fsd' else dsn_nld_spec(nc, 1 if self.d_arch == 'nld_s1' else 2, gk, norm='BatchEval')))
            self._d_eval_stale = True
        else:
            self.netD = NLayerDiscriminatorHIP(nc, device=self.device, spec_layers=spec_layers)
            self.netD.load_state_dict(default_init_state(self.netD.spec))
        self.opt_g = AdamHIP(self.netG.params, o['learning_rate'], (o['adam_beta_1'], 0.999), 0.0)
        self.opt_d = AdamHIP(self.netD.params, o['learning_rate'], (o['adam_beta_1'], 0.999), 0.0)
        self.epoch, self.iteration_count = 0, 0
        self.acc = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.log = OrderedDict()
        self.dp = None
        self._plans = {}

    def networks(self):
        return [self.netG, self.netD]

    def lr(self):
        """LambdaLR rule of train.py:154-157 (schedulers stepped once per epoch)"""
        o = self.opt
        start = o['num_epochs'] - o['num_decay_epochs']
        e = self.epoch
        f = 1.0 if e < start else 1.0 - max(0.0, float(e - start) / o['num_decay_epochs'])
        return o['learning_rate'] * f

    def end_epoch(self):
        self.epoch += 1

    def _plan(self, N, H, W):
        # the relativistic ops bake the data-parallel world size into their batch-mean divisor: a plan is valid for ONE world size
        k = (N, H, W, dp_world(self) if (self.rel or self.wgan) else 0)
        if k not in self._plans:
            self._plans[k] = _DSNPlan(self, N, H, W)
        return self._plans[k]

    def load_discriminator_state(self, sd):
        """state_dict of the reference Discriminator (codes/DSN/model.py:60-118), FSD-Batch ones with their BatchNorm buffers"""
        self.netD.load_state_dict(sd)
        self._d_eval_stale = True

    def inference_discriminator(self):
        """the network translate() / ddm_of() run: netD itself, or for BatchNorm its eval()-mode equivalent (running statistics folded into the convs)"""
        if not self.bn:
            return self.netD
        if self._d_eval_stale:
            self.netD_eval.load_state_dict(fold_batchnorm_fsd(self.netD.state_dict()))
            self._d_eval_stale = False
        return self.netD_eval

    def iteration(self, hr, bicubic_lr, real_lr):
        N, _, H, W = hr.shape
        P = self._plan(N, H, W)
        P.g.x_nchw.copy_(hr if self.netG.scale == 4 else bicubic_lr)
        P.bic_nchw.copy_(bicubic_lr)
        P.real_nchw.copy_(real_lr)
        dp_on = self.dp is not None and self.dp.active
        scale = self.dp.grad_scale if dp_on else 1.0
        if scale != P.scale:
            P.set_grad_scale(scale)
        if self.lpips_rot_flip and (self.iteration_count + 1) % self.gen_freq == 0:   # drawn where the reference evaluates its generator loss (train.py:251-259)
            P.set_symmetry(draw_symmetry())
        rg_dp = self.rel and dp_on   # --ragan under data parallelism: per-pixel batch sums all-reduced between the three loss stages
        if rg_dp:
            if P.ragan_world != self.dp.world:
                raise RuntimeError('the DSN plan was recorded for %d ranks, the process group has %d (attach model.dp before the first iteration)' % (P.ragan_world, self.dp.world))
            c0, c1, _ = P.ragan_cuts_fwd
            P.fwd.run(0, c0)                       # ... stage 0: per-pixel sums of the logits of both halves
            self.dp.all_reduce_here(P.r_sums)
            P.fwd.run(c0, c1)                      # stage 1: loss + per-pixel sums of the sigmoid terms
            self.dp.all_reduce_here(P.r_part)
            P.fwd.run(c1)                          # stage 2: gradients incl. the mean terms; colour / perceptual losses
        else:
            P.fwd.run()     # G, front ends, D on [fake; real], all losses and loss gradients
        if self.bn:     # BatchNorm running statistics, one update per discriminator call of the reference (train.py:221-226)
            P.d_running.run()
            self._d_eval_stale = True
        self.iteration_count += 1   # (train.py:206: before the frequency checks)
        upd_d, upd_g = self.iteration_count % self.disc_freq == 0, self.iteration_count % self.gen_freq == 0
        if upd_d:
            P.d_bwd.run()   # D weight gradients (pre-update graph)
            if self.wgan:   # + the gradient penalty: one mixing weight per iteration from torch's global RNG, drawn only when D steps (train.py:231-233)
                # (data parallel: ONE weight for the global batch -- rank 0's draw -- and ONE gradient norm over it: the ranks' sums of squares are
                # all-reduced between the norm and the tangent / reverse pass)
                r = torch.rand(1)
                if dp_on and self.dp.world > 1:
                    rd = r.to(self.device)
                    self.dp.broadcast_params(rd)
                    r = rd.cpu()
                P.gp.set_mix(float(r.item()))
                if P.gp.world > 1:
                    if not dp_on or self.dp.world != P.gp.world:
                        raise RuntimeError('the DSN plan was recorded for %d ranks (attach model.dp before the first iteration)' % P.gp.world)
                    P.gp.ops.run(0, P.gp.cut)
                    self.dp.all_reduce_here(P.gp.out3[3:4])
                    P.gp.ops.run(P.gp.cut)
                else:
                    P.gp.ops.run()
                _lib.check(_lib.lib().dasr_add_flat(self.netD.params.grad.data_ptr(), P.gp.grad.data_ptr(), P.gp.grad.numel(), _stream()), 'add_flat')
        if upd_g and rg_dp:   # generator's relativistic texture loss: stage 1 (sums still valid) -> all-reduce -> stage 2, then the backward chain
            P.g_bwd.run(0, P.ragan_cut_gbwd)
            self.dp.all_reduce_here(P.r_part)
            P.g_bwd.run(P.ragan_cut_gbwd)
        elif upd_g:
            P.g_bwd.run()   # texture gradient through D's data path, colour adjoint, G backward
        if self.dp is not None and self.dp.active:
            if upd_d:
                self.dp.allreduce_mean(self.netD.params.grad)
            if upd_g:
                self.dp.allreduce_mean(self.netG.params.grad)
        lr = self.lr()
        if upd_d:
            self.opt_d.step(lr)
            self.netD.repack()
        if upd_g:
            self.opt_g.step(lr)
            self.netG.repack()
        self.fake = P.g.fake_nchw
        self._pending = True

    # ---- inference: fake LR, discriminator map and domain-distance map (codes/DSN/create_dataset_modified.py:14-24,147-164) ----
    def translate(self, img):
        """img [n,3,H,W] in [0,1] -> (fake_lr [n,3,H/4,W/4], D_out [n,1,h',w'], ddm [n,1,h',w']).  D_out = sigmoid(D(fake)) with the
        frequency-separation front end (h' = h/2 for the wavelet filter); ddm = every D_out value spread over its receptive field
        (four [5,1,2] layers as the reference's table has it: 17x17) and divided by the coverage count = a count-normalised 17x17 box
        average (receptive_cal.py:34-60)."""
        n, _, H, W = img.shape
        self.inference_discriminator()   # BatchNorm: refresh the folded eval-mode copy if the weights moved
        k = ('inf', n, H, W)
        if k not in self._plans:
            self._plans[k] = _InferPlan(self, n, H, W)
        P = self._plans[k]
        P.g.x_nchw.copy_(img)
        P.ops.run()
        return P.g.fake_nchw, P.dout.nchw(1), P.ddm.nchw(1)

    def ddm_of(self, lr):
        """lr [n,3,h,w] in [0,1] (an LR image of either domain) -> (D_out, ddm) as in translate(), without the generator
        (create_dataset_modified.py:170-176, --including_source_ddm)"""
        n, _, h, w = lr.shape
        if self.filter == 'wavelet':
            h, w = h // 2 * 2, w // 2 * 2
            lr = lr[..., :h, :w]
        self.inference_discriminator()
        k = ('ddm', n, h, w)
        if k not in self._plans:
            self._plans[k] = _InferPlan(self, n, h, w, with_g=False)
        P = self._plans[k]
        P.lr_nchw.copy_(lr)
        P.ops.run()
        return P.dout.nchw(1), P.ddm.nchw(1)

    # ---- validation pass of the training driver (codes/DSN/train.py:293-355) ----
    def generate(self, img):
        """forward-only generator pass: img [n,3,H,W] in [0,1] -> fake [n,3,H/4,W/4] (DSGAN generator: same size); the result lives in the plan
        (valid until the next call).  Plans of the last two image shapes are kept: validation folders mix sizes."""
        n, _, H, W = img.shape
        key = ('gen', n, H, W)
        lru = self.__dict__.setdefault('_gen_lru', OrderedDict())
        if key in lru:
            lru.move_to_end(key)
        else:
            gp = self.netG.plan(n, H, W)
            ops = OpList()
            ops.extend(gp.fwd)
            lru[key] = (ops, gp)
            while len(lru) > 2:
                old, (_, gp_old) = lru.popitem(last=False)
                if not any(getattr(P, 'g', None) is gp_old for P in self._plans.values()):   # (a training / inference plan of that shape keeps it)
                    self.netG.plans.pop((old[1], old[2], old[3]), None)
        ops, gp = lru[key]
        gp.x_nchw.copy_(img)
        ops.run()
        return gp.fake_nchw

    def _colour_filter(self, x):
        """GeneratorLoss.color_filter (loss.py:50-58,103-107): FilterLow(padding=False) for gau / avg_pool, Haar LL * 0.5 for wavelet"""
        import torch.nn.functional as F
        if self.filter == 'wavelet':   # DWTForward(J=1, 'haar', mode='reflect'): an odd side is extended by one mirrored sample; LL * 0.5 = 2x2 mean
            x = F.pad(x, (0, x.shape[3] % 2, 0, x.shape[2] % 2), mode='reflect')
            return F.avg_pool2d(x, 2)
        return F.conv2d(x, self.freq.w.view(1, 1, self.k, self.k).expand(3, 1, self.k, self.k), groups=3)

    def perceptual_distance(self, x, y):
        """g_loss_module.perceptual_loss(x, y) without gradient: LPIPS(alex)(x, y, normalize=True).mean() or MSE of the VGG16 features (loss.py:108-130)
        on the HIP networks; nan when the model was built without a perceptual net (w_per = 0)."""
        if self.netF is None:
            return torch.full((), float('nan'), device=self.device)
        n, _, h, w = x.shape
        if self.opt['per_type'] == 'LPIPS':
            if h % 4 or w % 4:   # the stride-4 first conv runs as a space-to-depth conv on this path: whole 4x4 cells only
                if not self.__dict__.get('_warned_lpips_crop'):
                    logger.warning('validation LPIPS: %dx%d image centre-cropped to multiples of 4', h, w)
                    self._warned_lpips_crop = True
                h4, w4 = h // 4 * 4, w // 4 * 4
                y0, x0 = (h - h4) // 2, (w - w4) // 2
                x, y = x[..., y0:y0 + h4, x0:x0 + w4], y[..., y0:y0 + h4, x0:x0 + w4]
            return self.netF.distance(x.contiguous(), y.contiguous())
        key = ('valper', n, h, w)
        lru = self.__dict__.setdefault('_valper_lru', OrderedDict())
        if key in lru:
            lru.move_to_end(key)
        else:
            v = self.netF.plan(2 * n, 2 * n, h, w)
            nchw = torch.zeros((2 * n, 3, h, w), dtype=torch.float32, device=self.device)
            img = BTensor(2 * n, 16, h, w, True, self.device)
            ops = OpList()
            ops.add(make_op(_lib.OP_NCHW2B, src=nchw.data_ptr(), N=2 * n, C=3, H=h, W=w, dst_f32=img.view()))
            ops.add(v.input_copy_op(img.view(), 0, 2 * n, h, w))
            ops.extend(v.fwd)
            ops.keep += [v, nchw, img]
            lru[key] = (ops, nchw, v)
            while len(lru) > 2:
                old, _ = lru.popitem(last=False)
                self.netF.plans.pop((2 * old[1], 2 * old[1], old[2], old[3]), None)
        ops, nchw, v = lru[key]
        nchw[:n].copy_(x)
        nchw[n:].copy_(y)
        ops.run()
        f = v.feat.nchw()
        return torch.mean((f[:n] - f[n:]) ** 2)

    def validation_metrics(self, fake, target):
        """the six per-image validation terms of train.py:313-321 for fake = clamp(G(input), 0, 1) against the paired LR image: mse, psnr,
        rgb_loss (L1 of the per-channel means), mean_loss (L1 of the image means), perceptual_loss, color_loss -- device scalars"""
        import torch.nn.functional as F
        mse = ((fake - target) ** 2).mean()
        return OrderedDict([
            ('mse', mse), ('psnr', -10 * torch.log10(mse)),
            ('rgb_error', F.l1_loss(fake.mean(3).mean(2), target.mean(3).mean(2))),
            ('mean_error', F.l1_loss(fake.reshape(fake.shape[0], -1).mean(1), target.reshape(target.shape[0], -1).mean(1))),
            ('perceptual_error', self.perceptual_distance(fake, target)),
            ('color_error', F.l1_loss(self._colour_filter(fake), self._colour_filter(target)))])

    def filter_low(self, x):
        """model.FilterLow(kernel_size, gaussian = filter == 'gau', include_pad=False) of the validation image strips (train.py:141): same-size low-pass
        (zero padding; the box average counts only the pixels inside)"""
        import torch.nn.functional as F
        k, p = self.k, (self.k - 1) // 2
        if self.filter == 'gau':
            return F.conv2d(x, self.freq.w.view(1, 1, k, k).expand(3, 1, k, k), padding=p, groups=3)
        return F.avg_pool2d(x, k, stride=1, padding=p, count_include_pad=False)

    def filter_high(self, x):
        """model.FilterHigh(..., normalize=True): 0.5 + 0.5 (x - low(x)) (train.py:142)"""
        return 0.5 + 0.5 * (x - self.filter_low(x))

    def check_finite(self):
        self.opt_g.check_finite('DSN generator')
        self.opt_d.check_finite('DSN discriminator')

    def get_current_log(self):
        if getattr(self, '_pending', False):
            a = self.acc.tolist()
            self.check_finite()
            o = self.opt
            if self.wgan and self.ragan:   # a[0] = -mean D(real), a[1] = mean D(fake), a[2] = -mean D(fake), scores a[4] / a[5] = mean D(real) / mean D(fake)
                w = a[0] + a[1]            # -> -mean(real_tex) = mean(fake_tex) = mean D(fake) - mean D(real); mean(-fake_tex) = -mean D(fake) + mean D(real)
                a[0], a[1], a[2], a[4], a[5] = w, w, a[2] + a[4], a[4] - a[5], a[5] - a[4]
            self.log.update({'loss/d_tex_loss': a[0] + a[1] + (a[7] if self.wgan else 0.0), 'loss/g_tex_loss': a[2], 'loss/color_loss': a[3], 'loss/perceptual_loss': a[6],
                             'loss/g_overall_loss': o['w_col'] * a[3] + o['w_tex'] * a[2] + o['w_per'] * a[6], 'disc_score/real': a[4],
                             'disc_score/fake': a[5]})
            if self.wgan:
                self.log['disc_score/gradient_penalty'] = a[7]   # train.py:247-248
            self._pending = False
        return self.log

    # ---- checkpoint (.tar dict of codes/DSN/train.py:357-376) ----
    def save(self, path):
        o = self.opt
        torch.save({'epoch': self.epoch, 'iteration': self.iteration_count, 'fs_type': o['filter'], 'fs_kernel_size': o['kernel_size'],
                    'D_type': o['discriminator'], 'model_g_state_dict': self.netG.state_dict(), 'models_d_state_dict': self.netD.state_dict(),
                    'optimizer_g_state_dict': self.opt_g.state_dict(self.lr()), 'optimizer_d_state_dict': self.opt_d.state_dict(self.lr()),
                    'scheduler_g_state_dict': self._sched_state(), 'scheduler_d_state_dict': self._sched_state()}, path)

    def _sched_state(self):
        """torch.optim.lr_scheduler.LambdaLR.state_dict() layout (the lambda itself is not picklable and is stored as None)"""
        return {'base_lrs': [self.opt['learning_rate']], 'last_epoch': self.epoch, 'verbose': False, '_step_count': self.epoch + 1,
                '_get_lr_called_within_step': False, '_last_lr': [self.lr()], 'lr_lambdas': [None]}

    def load(self, path):
        ck = torch.load(path, map_location='cpu', weights_only=False)
        self.netG.load_state_dict(ck['model_g_state_dict'])
        self.load_discriminator_state(ck['models_d_state_dict'])
        self.opt_g.load_state_dict(ck['optimizer_g_state_dict'])
        self.opt_d.load_state_dict(ck['optimizer_d_state_dict'])
        self.epoch, self.iteration_count = ck['epoch'], ck['iteration']


class _GradPenaltyPlan:
    """--wgan (codes/DSN/train.py:231-241): grad_pen = 10 (|| d mean D(sample) / d sample ||_2 - 1)^2 on sample = r real + (1 - r) fake (ONE r per iteration),
    and its gradient w.r.t. the discriminator's weights -- the reference gets it from torch.autograd.grad(..., create_graph=True) + backward.
    Here: with g = d mean D / d sample (first-order backward to the input) and c = d pen / d ||g|| / ||g||, d pen / d theta = c * d <g_const, g(theta)> / d theta, and
    <g_const, g(theta)> = the DIRECTIONAL derivative of mean D(sample; theta) along g_const -- a forward-mode tangent pass through the discriminator (convs on the
    tangent, lrelu' masks, the symmetric InstanceNorm Jacobian: dasr_inorm_lrelu_jvp) followed by ONE reverse pass over the (primal, tangent) pair: every conv weight
    receives adj_z (x) a + adj_zdot (x) adot (one weight-gradient launch over both pairs), InstanceNorm contributes its second-order term (dasr_inorm_second).
    All on the device in one recorded list; the mixing weight is patched into the first op per iteration."""

    def __init__(self, plan, m, N, h, w, hd, wd, acc_slot):
        from .gan_nets import _DPlan, SLOPE as D_SLOPE
        net, dev, d = m.netD, m.device, plan.d
        # BatchNorm discriminators (round 6): D(sample) is ONE training-mode call on the N mixed images (train.py:234) -- one statistics group, and a third
        # running-statistics update per discriminator step, behind those of D(real) and D(fake)
        self.dg = dg = _DPlan(net, N, hd, wd, groups=1)       # the discriminator on the N mixed images (its own activations / statistics)
        nl = len(net.layers)
        nc = net.layers[0]['cin']
        P, pack = net.params, net.pack
        B = lambda t: BTensor(N, t.C, t.H, t.W, True, dev)
        self.g_img, self.t0 = BTensor(N, 16, h, w, True, dev), BTensor(N, 16, hd, wd, True, dev)
        self.part, self.out3 = torch.zeros(256, dtype=torch.float32, device=dev), torch.zeros(4, dtype=torch.float32, device=dev)
        self.one = torch.ones(1, dtype=torch.float32, device=dev)
        self.grad = torch.zeros_like(P.grad)         # the penalty's weight gradients (entries no conv of the pass owns stay zero: last bias, frozen filter)
        self.ws = Workspace(dev)
        ops = OpList()
        # ---- sample (already behind the linear front end: F(r real + (1 - r) fake) = r F(real) + (1 - r) F(fake), the + 0.5 of the normalisation included)
        self.mix_op = len(ops.ops)   # a = r (real half), b = 1 - r (fake half): set_mix()
        ops.add(make_op(_lib.OP_AXPBY, x=d.x.view(n0=N), a=0.5, z=d.x.view(), b=0.5, N=N, C=nc, H=hd, W=wd, out_f32=dg.x.view(), gamma=1.0))
        ops.extend(dg.fwd)
        if m.bn:
            ops.extend(dg.running_ops(0))
        lg = dg.logits
        cnt = float(N * lg.H * lg.W)
        # d mean D / d D = 1 / cnt
        ops.add(make_op(_lib.OP_FILL_SCALED, x=dg.g_logits.view(), N=N, C=1, H=lg.H, W=lg.W, scalar=self.one.data_ptr(), factor=1.0 / cnt))
        ops.extend(dg.bwd_data_ops(N))                # -> dg.gx = d mean D / d (front-end output)
        ops.add(make_op(_lib.OP_FILL, p=self.g_img.t.data_ptr(), n=self.g_img.t.numel(), value=0.0))
        ops.add_all(m.freq.adjoint(self.g_img.view(), N, h, w, g_high=dg.gx.view()))   # adjoint of the front end -> g = d mean D / d sample (image space)
        # out3 = {||g||, 10 (||g|| - 1)^2, 20 (||g|| - 1) / ||g||}; acc[slot] += the penalty.  Data parallel: two stages around the all-reduce of the ranks'
        # sums of squares (dasr_grad_penalty; DSNModel.iteration runs ops[:cut], all-reduces out3[3], runs ops[cut:])
        self.world = dp_world(m)
        for stage in ((0,) if self.world == 1 else (1, 2)):
            ops.add(make_op(_lib.OP_GRAD_PENALTY, g=self.g_img.view(), N=N, C=3, H=h, W=w, weight=10.0, part256=self.part.data_ptr(), out3=self.out3.data_ptr(),
                            loss_acc=m.acc.data_ptr() + 4 * acc_slot, stage=stage, world=self.world))
            if stage == 1:
                self.cut = len(ops.ops)
        # ---- tangent pass along u = g: t0 = (linear part of the front end)(g)
        ops.add_all(m.freq.tangent(self.g_img.view(), N, h, w, self.t0.view()))
        keep = []
        adot, zdot = [None] * nl, [None] * nl        # tangents of the layer outputs (after norm + lrelu) / of the conv outputs in front of a norm
        src = self.t0
        for i, L in enumerate(net.layers[:-1]):
            (hi, wi), (ho, wo) = dg.dims[i], dg.dims[i + 1]
            if L['norm']:
                zdot[i] = B(dg.zs[i])
                adot[i] = B(dg.acts[i])
                ops.add(conv_op(pack, L['fwd'], src.view(), True, L['cin_pad'], hi, wi, ho, wo, N, kh=L['kh'], stride=L['stride'], pad=L['pad'], out_f32=zdot[i].view()))
                ops.add(dg.norm_op(i, 'jvp', N, t=zdot[i].view(), out=adot[i].view()))
            else:   # conv + lrelu: adot = lrelu'(a) * conv(tangent) (the mask multiplies the conv output in the epilogue; no bias on a tangent)
                adot[i] = B(dg.acts[i])
                ops.add(conv_op(pack, L['fwd'], src.view(), True, L['cin_pad'], hi, wi, ho, wo, N, kh=L['kh'], stride=L['stride'], pad=L['pad'],
                                mask=dg.acts[i].view(), mask_f32=1, slope=D_SLOPE, out_f32=adot[i].view()))
            src = adot[i]
        # ---- reverse pass over (primal, tangent): s = mean(conv_last(adot)), upstream c / cnt
        Ll = net.layers[-1]
        gz = B(dg.g_logits)                           # adjoint of the last conv's TANGENT output
        ops.add(make_op(_lib.OP_FILL_SCALED, x=gz.view(), N=N, C=1, H=lg.H, W=lg.W, scalar=self.out3.data_ptr() + 8, factor=1.0 / cnt))
        GS = 256.0   # power-of-two pre-scale of the f16-staged weight-gradient operands (the adjoints here are c / cnt ~ 1e-2 .. 1e1)

        def wgrad(i, pairs, bias):
            L = net.layers[i]
            (hi, wi), (ho, wo) = dg.dims[i], dg.dims[i + 1]
            grp = WgradGroup(L['kh'], L['stride'])
            (g0, x0), more = pairs[0], pairs[1:]
            grp.add_conv(g0.view, True, g0.planes, x0.view, True, x0.planes, L['cout'], L['cin'], hi, wi, ho, wo, N, P.off(L['key'] + 'weight'),
                         P.off(L['key'] + 'bias') if (bias and L['bias']) else None, pad=L['pad'], f16=net.prec == 4, g_scale=GS if net.prec == 4 else 0.0,
                         more_pairs=[(gg.view, xx.view) for gg, xx in more])
            grp.emit(ops, self.ws, dev, self.grad.data_ptr())

        i = nl - 1
        wgrad(i, [(gz, adot[i - 1])], bias=False)     # the last conv's bias does not enter the directional derivative
        g_adot, g_a = B(dg.acts[i - 1]), None         # adjoints of adot[i-1] (tangent path) and of a[i-1] (primal path; none yet)
        dg._dgrad_ops(ops, i, N, gz, g_adot, None)
        for i in range(nl - 2, -1, -1):
            L = net.layers[i]
            inp_a = dg.x if i == 0 else dg.acts[i - 1]
            inp_adot = self.t0 if i == 0 else adot[i - 1]
            if L['norm']:
                # the first-order backward of the norm on both adjoints: J (lrelu'(a) ga).  BatchNorm: the primal one also gives d pen / d gamma, d beta of
                # a = lrelu(gamma xhat + beta)
                g_zdot, g_z = B(dg.zs[i]), B(dg.zs[i])
                gdst = (None, None)
                if L['norm'] == 'batch':
                    gdst = (self.grad.data_ptr() + 4 * P.off(L['bn'] + 'weight'), self.grad.data_ptr() + 4 * P.off(L['bn'] + 'bias'))
                for ga_, out_, prim in ((g_adot, g_zdot, False),) + (((g_a, g_z, True),) if g_a is not None else ()):
                    ops.add(dg.norm_op(i, 'bwd', N, ga=ga_.view(), gx=out_.view(), dgamma=gdst[0] if prim else None, dbeta=gdst[1] if prim else None))
                # + the dependence of J on z: tangent zdot, upstream lrelu'(a) * g_adot; BatchNorm: and the tangent output's own factor gamma
                # (dasr_inorm_second / dasr_bnorm_second; += on top of the primal terms when there are any)
                ops.add(dg.norm_op(i, 'second', N, t=zdot[i].view(), ga=g_adot.view(), out=g_z.view(), accumulate=1 if g_a is not None else 0,
                                   dgamma=gdst[0]))
            else:   # conv + lrelu: the adjoints pass through lrelu'(a) (applied as the mask of the data-gradient convs of the layer ABOVE, see below)
                g_zdot, g_z = g_adot, g_a
            wgrad(i, [(g_z, inp_a), (g_zdot, inp_adot)] if g_z is not None else [(g_zdot, inp_adot)], bias=g_z is not None)
            if i > 0:
                below = net.layers[i - 1]
                n_adot, n_a = B(dg.acts[i - 1]), (B(dg.acts[i - 1]) if g_z is not None else None)
                m_ = None if below['norm'] else dg.acts[i - 1]     # plain conv + lrelu below: its lrelu' is the mask of these data-gradient convs
                dg._dgrad_ops(ops, i, N, g_zdot, n_adot, m_)
                if g_z is not None:
                    dg._dgrad_ops(ops, i, N, g_z, n_a, m_)
                keep += [g_adot, g_a, g_zdot, g_z]
                g_adot, g_a = n_adot, n_a
        self.keep = keep + [g_adot, g_a, gz] + adot + zdot
        self.ws.finalize()
        self.ops = ops.tag(10)

    def set_mix(self, r):
        self.ops.set(self.mix_op, 'a', float(r))
        self.ops.set(self.mix_op, 'b', 1.0 - float(r))


class _DSNPlan:
    def __init__(self, m, N, H, W):
        dev = m.device
        self.m, self.N, self.scale = m, N, 1.0
        h, w = H // 4, W // 4
        # De_resnet maps the HR crop to LR size; the DSGAN Generator maps the bicubic LR image to an LR image (codes/DSN/train.py:213-217)
        self.g = m.netG.plan(N, H, W) if m.netG.scale == 4 else m.netG.plan(N, h, w)
        g = self.g
        fs = m.freq
        hd, wd = fs.out_size(h, w)
        self.d = m.netD.plan(2 * N, hd, wd)   # [fake; real]
        d = self.d
        self.bic_nchw = torch.zeros((N, 3, h, w), dtype=torch.float32, device=dev)
        self.real_nchw = torch.zeros((N, 3, h, w), dtype=torch.float32, device=dev)
        self.bic_b, self.real_b = BTensor(N, 16, h, w, True, dev), BTensor(N, 16, h, w, True, dev)
        hc, wc = fs.colour_size(h, w)
        self.col_f, self.col_b, self.g_col = (BTensor(N, 16, hc, wc, True, dev) for _ in range(3))
        acc = m.acc.data_ptr()
        o_ = m.opt
        f = OpList()
        f.extend(g.fwd)
        f.add(make_op(_lib.OP_FILL, p=acc, n=8, value=0.0))
        for src, dst in ((self.bic_nchw, self.bic_b), (self.real_nchw, self.real_b)):
            f.add(make_op(_lib.OP_NCHW2B, src=src.data_ptr(), N=N, C=3, H=h, W=w, dst_f32=dst.view()))
        # discriminator front end on fake -> d.x[:N], real -> d.x[N:]
        for src, n0 in ((g.fake, 0), (self.real_b, N)):
            f.add_all(fs.split(src.view(), N, h, w, high=d.x.view(n0=n0)))
        f.extend(d.fwd)
        # BatchNorm discriminator: the reference calls D(real) then D(fake) (with --ragan: net(real), net(fake), net(fake), net(real)); every call
        # in training mode moves the running statistics once, with that call's batch statistics (group 0 = fake half, 1 = real half)
        self.d_running = OpList()
        if m.bn:
            for grp_ in ((1, 0, 0, 1) if m.ragan else (1, 0)):
                self.d_running.extend(d.running_ops(grp_))
        lg = d.logits
        cnt = float(N * lg.H * lg.W)
        # --ragan: the same two terms on relativistic logits real - mean_n(fake), fake - mean_n(real): the three dasr_ragan stages back to back
        # (whole loss -> acc[0]; scores = mean sigmoid of the relativistic logits); gradients of both halves incl. the mean terms
        self.r_sums = self.r_part = None
        if m.rel:
            hw = lg.H * lg.W
            self.r_sums, self.r_part = (torch.zeros(2 * hw, dtype=torch.float32, device=dev) for _ in range(2))
            rl = [OpList(), OpList(), OpList()]
            # data parallel: the batch means are means over the GLOBAL batch (n_glob = N * world); iteration() all-reduces the per-pixel sums
            # between the stages, as the SRN trainer does (dasr_model.py::_run_ragan), so the lists are cut at the stage boundaries
            self.ragan_world = dp_world(m)
            _ragan_ops(rl, lg.view(n0=N), lg.view(), N, lg.H, lg.W, N * self.ragan_world, 1.0, 0.0, 1.0 / cnt, 1.0 / cnt, self.r_sums, self.r_part, acc, acc + 4 * 4,
                       acc + 4 * 5, 1.0 / cnt, d.g_logits.view(n0=N), d.g_logits.view(), form=1, eps=EPS)
            self.ragan_cuts_fwd = []
            for l_ in rl:
                f.extend(l_)
                self.ragan_cuts_fwd.append(len(f.ops))
        # discriminator loss: -log(real) - log(1 - fake)   (acc[0], acc[1]); scores acc[4] (real), acc[5] (fake)
        for n0, target, a_loss, a_score in (((N, 1.0, 0, 4), (0, 0.0, 1, 5)) if m.wgan else ()):   # --wgan: -mean(real) + mean(fake) on the raw map (loss.py:33-36)
            # (--ragan: both relativistic terms carry every logit once)
            f.add(make_op(_lib.OP_BCE, x=lg.view(n0=n0), N=N, C=1, H=lg.H, W=lg.W, gan_type=2, target=target, coef=1.0 / cnt,
                          gcoef=(2.0 if m.ragan else 1.0) / cnt, loss_acc=acc + 4 * a_loss, score_acc=acc + 4 * a_score, score_coef=1.0 / cnt,
                          grad=d.g_logits.view(n0=n0)))
        for n0, mode, a_loss, a_score in (() if (m.rel or m.wgan) else ((N, 0, 0, 4), (0, 1, 1, 5))):
            f.add(make_op(_lib.OP_LOGLOSS, x=lg.view(n0=n0), N=N, H=lg.H, W=lg.W, mode=mode, eps=EPS, coef=1.0 / cnt, gcoef=1.0 / cnt, score_coef=1.0 / cnt,
                          loss_acc=acc + 4 * a_loss, score_acc=acc + 4 * a_score, grad=d.g_logits.view(n0=n0)))
        # colour loss: L1 between the low-pass of fake and of the bicubic LR (acc[3])
        for src, dst in ((g.fake, self.col_f), (self.bic_b, self.col_b)):
            f.add_all(fs.colour(src.view(), N, h, w, dst.view()))
        ccnt = float(N * 3 * hc * wc)
        f.add(make_op(_lib.OP_L1DIFF, a=self.col_f.view(), b=self.col_b.view(), is_f32=1, N=N, C=3, H=hc, W=wc, coef=1.0 / ccnt,
                      gcoef=float(o_['w_col']) / ccnt, loss_acc=acc + 4 * 3, ga=self.g_col.view()))
        self.v = None
        lpips = m.netF is not None and o_['per_type'] == 'LPIPS'
        if lpips:                # perceptual: LPIPS(fake, bicubic).mean() -> acc[6]; head gradients (weight w_per) in the forward list
            self.v = m.netF.plan(2 * N, N, h, w)
            self.sym_ops = [(f, len(f.ops), 0), (f, len(f.ops) + 1, 0)]   # (list, index, base mode) of the LPIPS input / adjoint ops: set_symmetry()
            f.add(self.v.input_op(g.fake.view(), 0, N))
            f.add(self.v.input_op(self.bic_b.view(), N, N))
            f.extend(self.v.fwd)
            for o in self.v.head_ops(acc + 4 * 6, float(o_['w_per'])):
                f.add(o)
        elif m.netF is not None:   # perceptual: MSE(vgg16(fake), vgg16(bicubic)) -> acc[6], gradient into v.g_feat[:N]
            self.v = m.netF.plan(2 * N, N, h, w)
            v = self.v
            for src, n0 in ((g.fake, 0), (self.bic_b, N)):
                f.add(v.input_copy_op(src.view(), n0, N, h, w))
            f.extend(v.fwd)
            ft = v.feat
            fcnt = float(N * ft.C * ft.H * ft.W)
            f.add(make_op(_lib.OP_L1DIFF, a=ft.view(), b=ft.view(n0=N), is_f32=1 | 2, N=N, C=ft.C, H=ft.H, W=ft.W, coef=1.0 / fcnt,
                          gcoef=float(o_['w_per']) / fcnt, loss_acc=acc + 4 * 6, ga=v.g_feat.view()))
        self.fwd = f
        # D weight gradients from the pre-update graph
        self.d_bwd = d.bwd_full
        self.gp = _GradPenaltyPlan(self, m, N, h, w, hd, wd, acc_slot=7) if m.wgan else None   # value -> acc[7], weight gradients -> gp.grad
        # generator: texture loss gradient through D's data path (+ colour adjoint) -> g_fake -> G backward
        gb = OpList()
        if m.rel:   # -log(sigmoid(fake - mean_n(real)) + eps): stage 0's sums are still valid, the real term is absent (t < 0), real carries no gradient
            rl = [OpList(), OpList(), OpList()]
            _ragan_ops(rl, lg.view(n0=N), lg.view(), N, lg.H, lg.W, N * self.ragan_world, -1.0, 1.0, 1.0 / cnt, float(o_['w_tex']) / cnt, self.r_sums, self.r_part,
                       acc + 4 * 2, None, None, 0.0, None, d.g_logits.view(), form=1, eps=EPS, stages=(1, 2))
            gb.extend(rl[1])
            self.ragan_cut_gbwd = len(gb.ops)
            gb.extend(rl[2])
        elif m.wgan:   # generator_loss(wasserstein): mean(-fake_tex) (loss.py:18-19): value -> acc[2], gradient w_tex * (-1 / cnt) -> g_logits[:N]
            gb.add(make_op(_lib.OP_BCE, x=lg.view(), N=N, C=1, H=lg.H, W=lg.W, gan_type=2, target=1.0, coef=1.0 / cnt, gcoef=float(o_['w_tex']) / cnt,
                           loss_acc=acc + 4 * 2, grad=d.g_logits.view()))
        else:   # -log(fake_tex) on the fake half: value -> acc[2], gradient -> g_logits[:N]
            gb.add(make_op(_lib.OP_LOGLOSS, x=lg.view(), N=N, H=lg.H, W=lg.W, eps=EPS, coef=1.0 / cnt, gcoef=float(o_['w_tex']) / cnt, loss_acc=acc + 4 * 2,
                           grad=d.g_logits.view()))
        gb.extend(d.bwd_data_ops(N))
        gb.add(make_op(_lib.OP_FILL, p=g.g_fake.t.data_ptr(), n=g.g_fake.t.numel(), value=0.0))
        gb.add_all(fs.adjoint(g.g_fake.view(), N, h, w, g_high=d.gx.view(), g_colour=self.g_col.view()))   # adjoint of the high-pass front end and of the colour filter
        if lpips:
            gb.extend(self.v.bwd)
            self.sym_ops.append((gb, len(gb.ops), 1))
            gb.add(self.v.adjoint_op(g.g_fake.view()))
        elif self.v is not None:
            gb.extend(self.v.bwd)
            gb.add(make_op(_lib.OP_AXPBY, x=g.g_fake.view(), a=1.0, z=self.v.gx.view(), b=1.0, N=N, C=16, H=h, W=w, out_f32=g.g_fake.view(), gamma=1.0))
        gb.extend(g.bwd)
        self.g_bwd = gb

    def set_symmetry(self, xf):
        """LPIPS sees T(fake), T(bicubic): xf = symmetry code of dasr_lpips_s2d (bits: transpose, flip rows, flip columns); 0 = identity"""
        if xf and (xf & 1) and self.v.H != self.v.W:
            raise ValueError('--lpips_rot_flip with a rotation needs square crops (torch.rot90 would change the shape)')
        for lst, idx, base in getattr(self, 'sym_ops', ()):
            lst.set(idx, 'mode', base | (xf << 4))

    def set_grad_scale(self, scale):
        self.scale = scale
        self.g.set_grad_scale(scale)
        set_reduce_scale((self.d_bwd, self.g_bwd) + ((self.gp.ops,) if self.gp is not None else ()), scale)   # (with dgamma / dbeta of a BatchNorm discriminator)


DDM_RF = 17  # receptive field of the reference's conv table [[5,1,2]] * 4 for FSD (create_dataset_modified.py:120-121)
# conv tables [kernel, stride, padding] the reference walks for the domain-distance map (create_dataset_modified.py:112-121)
DDM_CONVNETS = {'fsd': [[5, 1, 2]] * 4, 'nld_s1': [[4, 1, 1]] * 4, 'nld_s2': [[4, 2, 1], [4, 2, 1], [4, 1, 1], [4, 1, 1]]}


def receptive_walk(imsize, convnet):
    """(number of features, jump, receptive field, centre of the first feature) after the conv table (receptive_cal.py:10-25,45-52)"""
    import math
    n, j, r, start = imsize, 1, 1, 0.5
    for k, s_, p in convnet:
        n_out = math.floor((n - k + 2 * p) / s_) + 1
        pad_l = math.floor(((n_out - 1) * s_ - n + k) / 2)
        j, r, start, n = j * s_, r + (k - 1) * j, start + ((k - 1) / 2 - pad_l) * j, n_out
    return n, j, r, start


class _InferPlan:
    """with_g: (H, W) is the HR input of the generator and the discriminator sees G's output; else (H, W) is an LR image fed to D"""

    def __init__(self, m, N, H, W, with_g=True):
        dev = m.device
        # De_resnet maps the image to 1/4 size; the DSGAN Generator keeps the size (create_dataset_modified.py:99-103 applies either to the image as is)
        h, w = (H // 4, W // 4) if (with_g and m.netG.scale == 4) else (H, W)
        assert not m.freq.wavelet or (h % 2 == 0 and w % 2 == 0), 'wavelet front end: even image size (ddm_of crops; translate expects it)'
        hd, wd = m.freq.out_size(h, w)
        self.d = m.inference_discriminator().plan(N, hd, wd)
        d = self.d
        nh, nw = d.logits.H, d.logits.W          # FSD keeps the map size; the nld discriminators shrink it
        self.dout, self.ddm = BTensor(N, 16, nh, nw, True, dev), BTensor(N, 16, hd, wd, True, dev)
        self.box = torch.full((DDM_RF * DDM_RF,), 1.0 / (DDM_RF * DDM_RF), dtype=torch.float32, device=dev)
        ops = OpList()
        if with_g:
            self.g = m.netG.plan(N, H, W)
            ops.extend(self.g.fwd)
            src = self.g.fake
        else:
            self.lr_nchw = torch.zeros((N, 3, h, w), dtype=torch.float32, device=dev)
            src = BTensor(N, 16, h, w, True, dev)
            ops.add(make_op(_lib.OP_NCHW2B, src=self.lr_nchw.data_ptr(), N=N, C=3, H=h, W=w, dst_f32=src.view()))
            self.src = src
        ops.add_all(m.freq.split(src.view(), N, h, w, high=d.x.view()))
        ops.extend(d.fwd)
        if m.wgan:   # --wgan (model.py:104-105): the discriminator map is the raw logit map
            ops.add(make_op(_lib.OP_AXPBY, x=d.logits.view(), a=1.0, N=N, C=1, H=nh, W=nw, out_f32=self.dout.view(), gamma=1.0))
        else:
            ops.add(make_op(_lib.OP_SIGMOID_FWD, x=d.logits.view(), N=N, C=1, H=nh, W=nw, y=self.dout.view()))
        if m.d_arch == 'fsd':   # count-normalised box average = spread over the receptive field / coverage count
            ops.add(make_op(_lib.OP_LOWPASS, x=self.dout.view(), w=self.box.data_ptr(), k=DDM_RF, N=N, C=1, H=hd, W=wd, mode=0 | 2, out_low=self.ddm.view()))
        else:                          # general receptive-field spread (jump / rf / start of the WIDTH walk for both axes, as the reference does)
            n_h = receptive_walk(hd, DDM_CONVNETS[m.d_arch])[0]
            n_w, jump, rf, start = receptive_walk(wd, DDM_CONVNETS[m.d_arch])
            assert (n_h, n_w) == (nh, nw), ((n_h, n_w), (nh, nw))
            ops.add(make_op(_lib.OP_DDM_SPREAD, d=self.dout.view(), N=N, n_h=nh, n_w=nw, H=hd, W=wd, jump=jump, rf=rf, start=float(start), out=self.ddm.view()))
        self.ops = ops
