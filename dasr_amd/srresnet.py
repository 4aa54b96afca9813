"""SRResNet generator (reference: codes/SRN/models/modules/architecture.py:18-48, ResNetBlock block.py:221-251, pixelshuffle_block
block.py:838-851; built by networks.py:88-91 with act_type 'relu', upsample_mode 'pixelshuffle', then init_weights(kaiming, 0.1)) as recorded
op lists over the MI355X kernels.

fea_conv, LR_conv + the global skip and the PixelShuffle HR tail are the layers of RRDBNetHIP(upsample_mode='pixelshuffle') at the same
state_dict keys (model.0, model.1.sub.nb, model.2 / 5 / 8 / 10): this class reuses their packs and op-list builders with ReLU (slope 0) instead of
LeakyReLU.  The trunk is nb residual blocks y = x + conv1(relu(conv0(x))) on an fp32 residual stream with a bf16 shadow (bf16 operands, fp32
accumulation):
  fused_blocks=True  -- one dasr_resblock launch per block (h = relu(conv0) stays in LDS; training plans also store it for the backward)
  fused_blocks=False -- two dasr_conv launches per block (the composition the fused kernel is bit-identical to)
  fused_blocks=None  -- the form the measurements favour at the plan's shape (use_fused)
The backward runs per layer in both forms: conv1's data gradient (ReLU' of h as the mask), conv0's data gradient with the skip gradient added in
its epilogue, 12-wave weight-gradient launches on the bf16 tensors.
"""
import ctypes as C
import logging
import math
import os

import torch

from . import _lib
from ._lib import make_op
from .engine import BTensor, ParamStore, PackRegistry, OpList, Workspace, conv_op, NULL_T, GradScale, grad_prescale
from .rrdbnet import RRDBNetHIP, _Plan as _RRDBPlan

logger = logging.getLogger('base')


def srresnet_param_spec(in_nc, out_nc, nf, nb):
    """state_dict keys / shapes of the reference SRResNet in construction order (B.sequential flattens the nested sequentials):
    model.0 fea_conv, model.1.sub.{i}.res.{0,2} the blocks, model.1.sub.{nb} LR_conv, model.2 / model.5 the PixelShuffle convs (nf -> 4 nf),
    model.8 HR_conv0, model.10 HR_conv1"""
    spec = [('model.0.weight', (nf, in_nc, 3, 3)), ('model.0.bias', (nf,))]
    for i in range(nb):
        for j in (0, 2):
            p = 'model.1.sub.%d.res.%d.' % (i, j)
            spec += [(p + 'weight', (nf, nf, 3, 3)), (p + 'bias', (nf,))]
    spec += [('model.1.sub.%d.weight' % nb, (nf, nf, 3, 3)), ('model.1.sub.%d.bias' % nb, (nf,))]
    for idx, co in ((2, 4 * nf), (5, 4 * nf), (8, nf), (10, out_nc)):
        spec += [('model.%d.weight' % idx, (co, nf, 3, 3)), ('model.%d.bias' % idx, (co,))]
    return spec


def check_options(upscale=4, norm_type=None, mode='CNA'):
    """the option surface this generator implements (every shipped config); NotImplementedError names what the reference would build otherwise"""
    if upscale != 4:
        raise NotImplementedError('sr_resnet: scale %s is not implemented (the reference builds %s PixelShuffle stage(s) for it; only scale 4 runs '
                                  'here)' % (upscale, 1 if upscale == 3 else int(math.log(upscale, 2))))
    if norm_type:
        raise NotImplementedError('sr_resnet: norm_type %r is not implemented (the reference puts a %s norm layer after every trunk conv and '
                                  'LR_conv; only norm_type null runs here)' % (norm_type, norm_type))
    if (mode or 'CNA') != 'CNA':
        raise NotImplementedError('sr_resnet: mode %r is not implemented (the reference would order its ResNetBlocks as %s, with the activation '
                                  'in front of the conv; only CNA runs here)' % (mode, mode))
    if os.environ.get('DASR_HR_PREC', '2') != '2':
        raise NotImplementedError('sr_resnet: DASR_HR_PREC=%s is not implemented (the PixelShuffle HR tail runs in f16 storage only; unset it)'
                                  % os.environ['DASR_HR_PREC'])


class _TrunkScale(GradScale):
    """What the trainers expect of a plan's `store` (rrdbnet.TrunkStore).  SRResNet defers no weight gradients (every one is part of its plan's
    backward list), but its f16-storage trunk (trunk_prec 2) keeps the 16-bit gradient shadows pre-scaled by a power of two, shared by the plans
    of one (N, h, w) and calibrated from the data as TrunkStore's is.  The gradient shadows start at about max |dL/d(trunk output)|: head-room 1."""


class SRResNetHIP(RRDBNetHIP):
    act_slope = 0.0   # ReLU (networks.py:88-91: act_type 'relu')

    def __init__(self, in_nc=3, out_nc=3, nf=64, nb=16, upscale=4, device='cuda', fused_blocks=None, norm_type=None, mode='CNA', trunk_prec=None):
        """trunk_prec: storage of the trunk's 16-bit shadows -- 1 = bf16 (default), 2 = f16 storage of the activation shadows and of the
        gradient shadows, the latter pre-scaled by a power of two calibrated from the data (_TrunkScale; as DASR_RDB_PREC=2 is for RRDBNet's
        dense blocks).  None: DASR_RDB_PREC, else 1."""
        check_options(upscale, norm_type, mode)
        if nf % 32 or in_nc > 16 or out_nc > 16:
            raise NotImplementedError('sr_resnet: nf must be a multiple of 32, in_nc / out_nc at most 16')
        if trunk_prec is None:
            trunk_prec = int(os.environ.get('DASR_RDB_PREC', '1'))
        if trunk_prec not in (1, 2):
            raise ValueError('trunk_prec / DASR_RDB_PREC must be 1 (bf16) or 2 (f16 storage)')
        if fused_blocks and nf != 64:
            raise ValueError('fused_blocks: dasr_resblock is built for nf 64')
        if fused_blocks and trunk_prec == 2:
            raise ValueError('fused_blocks: dasr_resblock runs on bf16 shadows; the f16-storage trunk (trunk_prec 2) runs two launches per block')
        self.in_nc, self.out_nc, self.nf, self.nb, self.upsample_mode = in_nc, out_nc, nf, nb, 'pixelshuffle'
        self.device = torch.device(device)
        self.params = ParamStore(srresnet_param_spec(in_nc, out_nc, nf, nb), self.device)
        # attributes of the shared RRDBNetHIP builders: split-bf16 stream convs, f16-storage PixelShuffle tail, no chained launches, bf16 trunk
        self.rdb_prec, self.stream_prec, self.rdb_f16, self.chain, self.chain_form = trunk_prec, 3, trunk_prec == 2, False, 'auto'
        self.hr_prec, self.hr_f16s, self.ps, self.subpixel = 2, True, True, False
        self.chain_err = torch.zeros(1, dtype=torch.int32, device=self.device)   # no chained launch: stays zero (the trainers' gate word)
        self.fused_blocks = fused_blocks
        self.pack = PackRegistry(self.params)
        self._register_packs()
        self.pack.finalize()
        self.plans = {}

    def _register_trunk_packs(self):
        nf, P = self.nf, self.params
        mt = 2 if nf % 64 == 0 else 1
        for i in range(self.nb):
            for j in (0, 2):
                key = 'model.1.sub.%d.res.%d.weight' % (i, j)
                self.pk[(i, j)] = self.pack.add(nf, nf, 9, mt, self.rdb_prec, [self._seg_fwd(key, nf, nf)])
                self.pk[(i, j, 'b')] = self.pack.add(nf, nf, 9, mt, self.rdb_prec, [(P.off(key), nf, nf, 0, nf, 0, 1)])   # data gradient: transposed, taps flipped

    def chain_choice(self, N, h, w):
        return None, 0, 'SRResNet has no chained trunk form'

    def trunk_store(self, N, h, w):
        """one per (N, h, w), like RRDBNetHIP's: the sub-batch replicas of a step find their plans again by it (plan key)"""
        st = self.__dict__.setdefault('_stores', {})
        if (N, h, w) not in st:
            st[(N, h, w)] = _TrunkScale(self.rdb_f16)
        return st[(N, h, w)]

    def use_fused(self, inference):
        """fused residual blocks in this plan?  The constructor's choice if it made one, else the measured default (profiles/srresnet_ab.txt,
        DESIGN.md §8): the fused form for inference plans (1 x 256^2: 0.85 against 1.21 ms), two launches per block for training plans (the step at
        16 x 32^2 / 16 x 128^2: 2.75 / 7.12 ms against 4.35 / 9.85 ms fused)"""
        if self.fused_blocks is not None:
            return bool(self.fused_blocks)
        return self.nf == 64 and inference and not self.rdb_f16

    def _make_plan(self, *args, **kw):
        return _Plan(self, *args, **kw)


class _Plan(_RRDBPlan):
    """Buffers + recorded forward / backward op lists of SRResNetHIP for one (N, h, w); the members the trainers use are those of rrdbnet._Plan"""

    def __init__(self, net, N, h, w, replica=0, inference=False, store=None, n0=0):
        self.net, self.N, self.h, self.w = net, N, h, w
        dev, nf, nb = net.device, net.nf, net.nb
        self.inference, self.replica, self.n0 = inference, replica, n0
        # the store of a sub-batch group (SRResNetHIP.trunk_store) only shares the trunk's gradient scale: nothing is deferred (shared_store False)
        self.defer, self.shared_store = False, False
        self.store = store if store is not None else _TrunkScale(net.rdb_f16 and not inference)
        self.grad = net.params.grad if (replica == 0 or inference) else torch.zeros_like(net.params.grad)
        self.gscale = grad_prescale(N * 3 * 16 * h * w)   # f16 HR tail: as rrdbnet._Plan
        self.fused = net.use_fused(inference)
        self.chain = None
        H2, W2, H4, W4 = 2 * h, 2 * w, 4 * h, 4 * w
        B = lambda C_, H, W, f32: BTensor(N, C_, H, W, f32, dev)
        Bh = lambda C_, H, W: BTensor(N, C_, H, W, False, dev, f16=True)
        S16 = lambda: BTensor(N, nf, h, w, False, dev, f16=net.rdb_f16)   # 16-bit trunk shadows: bf16, or f16 with trunk_prec 2
        self.x_nchw = torch.zeros((N, net.in_nc, h, w), dtype=torch.float32, device=dev)
        self.sr_nchw = torch.zeros((N, net.out_nc, H4, W4), dtype=torch.float32, device=dev)
        self.x_in = B(16, h, w, True)
        self.fea = B(nf, h, w, True)
        self.stream = [B(nf, h, w, True) for _ in range(2)]
        # 16-bit shadows of the block inputs (training: all of them, the weight gradients of conv0 read them) and h = relu(conv0) (training: per block,
        # the ReLU mask and the weight-gradient input of conv1; inference: one buffer for the per-layer form, none for the fused one)
        self.xs16 = [S16() for _ in range(2 if inference else nb + 1)]
        self.hbuf = [S16() for _ in range((0 if self.fused else 1) if inference else nb)]
        self.t0 = B(nf, h, w, True)
        self.t0h = Bh(nf, h, w)
        self.u1, self.u2 = Bh(nf, H2, W2), Bh(nf, H4, W4)
        self.ps1, self.ps2 = Bh(4 * nf, h, w), Bh(4 * nf, H2, W2)
        self.h0 = Bh(nf, H4, W4)
        self.sr = B(16, H4, W4, True)
        if inference:
            self._build_forward()
            return
        self.g_ps1, self.g_ps2 = Bh(4 * nf, h, w), Bh(4 * nf, H2, W2)
        self.g_sr = B(16, H4, W4, True)
        self.g_sr16 = Bh(16, H4, W4)
        self.g4a, self.g4b, self.g2a, self.g2b = Bh(nf, H4, W4), Bh(nf, H4, W4), Bh(nf, H2, W2), None
        self.g_t0 = B(nf, h, w, True)
        # dL/d(stream), fp32, and its 16-bit shadow (operand of the data / weight gradients; f16 storage: times the store's gscale)
        self.gstream = [B(nf, h, w, True) for _ in range(2)]
        self.g16 = [S16() for _ in range(2)]
        self.gh = S16()                                        # dL/dh (ReLU' applied), 16-bit, scaled like g16
        self.g_fea = B(nf, h, w, True)
        self.ws = Workspace(dev)
        self._build_forward()
        self._build_backward()
        self.ws.finalize()

    def _resblock_op(self, i, X, xs_in, Y, xs_out, hb):
        net, P = self.net, self.net.params
        prm = _lib.ResblockParams()
        prm.x16, prm.x32 = xs_in.view(), X.view()
        pre = 'model.1.sub.%d.res.' % i
        prm.w0, prm.b0 = net.pack.ptr(net.pk[(i, 0)]), P.ptr(pre + '0.bias')
        prm.w1, prm.b1 = net.pack.ptr(net.pk[(i, 2)]), P.ptr(pre + '2.bias')
        prm.y32, prm.y16 = Y.view(), xs_out.view()
        prm.h = hb.view() if hb is not None else NULL_T
        prm.N, prm.H, prm.W, prm.res_scale, prm.slope = self.N, self.h, self.w, 1.0, 0.0
        return make_op(_lib.OP_RESBLOCK, flops=2 * 2.0 * self.N * self.h * self.w * 9 * net.nf * net.nf, p=C.addressof(prm)), prm

    def _build_forward(self):
        net, N, h, w = self.net, self.N, self.h, self.w
        nf, nb, P, pack, pk = net.nf, net.nb, net.params, net.pack, net.pk
        ops = OpList()
        ops.add(make_op(_lib.OP_NCHW2B, src=self.x_nchw.data_ptr(), N=N, C=net.in_nc, H=h, W=w, dst_f32=self.x_in.view()))
        f16 = int(net.rdb_f16)
        ops.add(conv_op(pack, pk['fea'], self.x_in.view(), True, 16, h, w, h, w, N, bias=P.ptr('model.0.bias'),
                        out_f32=self.fea.view(), out_bf16=self.xs16[0].view(), out16_f16=f16))
        logger.info('SRResNet trunk, %s plan at %d x %d x %d: %s' % ('inference' if self.inference else 'training', N, h, w,
                                                                    'one fused launch per residual block (dasr_resblock)' if self.fused else
                                                                    'two launches per residual block'))
        X = self.fea
        ns = len(self.xs16)
        for i in range(nb):
            Y = self.stream[i & 1]
            xs_in, xs_out = self.xs16[i % ns], self.xs16[(i + 1) % ns]
            hb = self.hbuf[i] if not self.inference else (self.hbuf[0] if self.hbuf else None)
            pre = 'model.1.sub.%d.res.' % i
            if self.fused:
                o, prm = self._resblock_op(i, X, xs_in, Y, xs_out, None if self.inference else hb)
                ops.add(o)
                ops.keep.append(prm)
            else:
                ops.add(conv_op(pack, pk[(i, 0)], xs_in.view(), False, nf, h, w, h, w, N, bias=P.ptr(pre + '0.bias'), act=1, slope=0.0,
                                out_bf16=hb.view(), out16_f16=f16))
                ops.add(conv_op(pack, pk[(i, 2)], hb.view(), False, nf, h, w, h, w, N, bias=P.ptr(pre + '2.bias'), res1=X.view(), beta1=1.0,
                                out_f32=Y.view(), out_bf16=xs_out.view(), out16_f16=f16))
            if i in getattr(net, 'debug_taps', ()):   # tests: fp32 copy of this block's output (the stream buffers alternate)
                self.taps = getattr(self, 'taps', {})
                self.taps[i] = BTensor(N, nf, h, w, True, net.device)
                ops.add(make_op(_lib.OP_AXPBY, x=Y.view(), a=1.0, N=N, C=nf, H=h, W=w, out_f32=self.taps[i].view(), gamma=1.0))
            X = Y
        self._build_tail_forward(ops, X)

    def _build_backward_trunk(self, ops):
        net, N, h, w = self.net, self.N, self.h, self.w
        nf, nb, P, pack, pk = net.nf, net.nb, net.params, net.pack, net.pk
        lrk = 'model.1.sub.%d.' % nb
        self._wg(ops, lrk, self.g_t0, True, self.x_last, True, nf, nf, h, w, h, w)
        ops.tag(11)
        # gradient buckets (index into ops, lo, hi): params.grad[lo:hi] is complete once ops[:index] have run
        self._marks = [(len(ops.ops), P.off(lrk + 'weight'), P.total)]
        f16 = int(net.rdb_f16)
        st = self.store
        gsc = st.gscale   # f16 storage: the 16-bit gradient shadows hold gsc * dL/d(.) (bf16: 1); the fp32 gradient stream stays unscaled
        G, G16 = self.gstream[0], self.g16[0]
        ops.add(conv_op(pack, pk['lr_b'], self.g_t0.view(), True, nf, h, w, h, w, N, out_f32=G.view(), out_bf16=G16.view(), gamma=gsc, out16_f16=f16))
        if f16:
            st.register_scaled(ops.ops[-1], False)

        def wg(key, g, inp):
            self._wg3(ops, key, g, inp, nf, nf, h, w, h, w, f16=bool(f16), g_scale=gsc)
            if f16:
                st.register_reduce(ops.ops[-1])

        for i in range(nb - 1, -1, -1):
            Gn, G16n = self.gstream[(nb - i) & 1], self.g16[(nb - i) & 1]
            pre = 'model.1.sub.%d.res.' % i
            hb = self.hbuf[i]
            # conv1 (res.2): dW from dL/dy x h; dL/dh = conv1^T(dL/dy) * ReLU'(h)
            wg(pre + '2.', G16, hb)
            ops.add(conv_op(pack, pk[(i, 2, 'b')], G16.view(), False, nf, h, w, h, w, N, mask=hb.view(), mask_f32=0, slope=0.0, out_bf16=self.gh.view(),
                            out16_f16=f16))
            # conv0 (res.0): dW from dL/dh x x; dL/dx = conv0^T(dL/dh) + dL/dy (the skip)
            wg(pre + '0.', self.gh, self.xs16[i])
            ops.add(conv_op(pack, pk[(i, 0, 'b')], self.gh.view(), False, nf, h, w, h, w, N, res1=G.view(), beta1=1.0, out_f32=Gn.view(),
                            out_bf16=G16n.view(), gamma=gsc, alpha=1.0 / gsc, out16_f16=f16))
            if f16:
                st.register_scaled(ops.ops[-1], True)
            nxt = 'model.1.sub.%d.res.0.weight' % (i + 1) if i + 1 < nb else lrk + 'weight'
            self._marks.append((len(ops.ops), P.off(pre + '0.weight'), P.off(nxt)))
            G, G16 = Gn, G16n
        ops.tag(4)
        # ShortcutBlock: g_fea = g_trunk + g_t0
        ops.add(make_op(_lib.OP_AXPBY, x=G.view(), a=1.0, z=self.g_t0.view(), b=1.0, N=N, C=nf, H=h, W=w, out_f32=self.g_fea.view(), gamma=1.0))
        self._wg(ops, 'model.0.', self.g_fea, True, self.x_in, True, nf, net.in_nc, h, w, h, w)
        self._marks.append((len(ops.ops), 0, P.off('model.1.sub.0.res.0.weight' if nb else lrk + 'weight')))
        ops.tag(11)
        self.bwd = ops
        self._segments = None
