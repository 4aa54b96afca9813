"""Patch discriminator and VGG19-54 feature extractor as recorded op lists over the MI355X kernels.

NLayerDiscriminatorHIP : codes/SRN/models/modules/architecture.py:983-1024 (built by networks.py:184-185: ndf stays 64)
VGGFeatureHIP          : codes/SRN/models/modules/architecture.py:1060-1088 (vgg19.features[:35], input norm, frozen)

Both run in split-bf16 (prec 3, ~fp32) on fp32 activations: together they are <10 % of the step's FLOPs and they sit
between the losses and the generator gradient, where the 1e-2 gradient tolerance is decided.
"""
import torch

from . import _lib
from .engine import (BTensor, ParamStore, PackRegistry, OpList, WgradGroup, Workspace, conv_op, ceil_div, F32, F16, SPLIT, grad_prescale)
from ._lib import make_op

SLOPE = 0.2
IN_EPS = 1e-5


def nlayer_d_spec(input_nc, ndf=64, n_layers=2):
    """[(key, shape)] and layer descriptions of the reference nn.Sequential."""
    spec = [('model.0.weight', (ndf, input_nc, 4, 4)), ('model.0.bias', (ndf,))]
    layers = [dict(key='model.0.', cin=input_nc, cout=ndf, stride=2, bias=True, norm=False, kh=4, pad=1)]
    mult, idx = 1, 2
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        spec.append(('model.%d.weight' % idx, (ndf * mult, ndf * prev, 4, 4)))
        layers.append(dict(key='model.%d.' % idx, cin=ndf * prev, cout=ndf * mult, stride=2, bias=False, norm=True, kh=4, pad=1))
        idx += 3
    prev, mult = mult, min(2 ** n_layers, 8)
    spec.append(('model.%d.weight' % idx, (ndf * mult, ndf * prev, 4, 4)))
    layers.append(dict(key='model.%d.' % idx, cin=ndf * prev, cout=ndf * mult, stride=1, bias=False, norm=True, kh=4, pad=1))
    idx += 3
    spec += [('model.%d.weight' % idx, (1, ndf * mult, 4, 4)), ('model.%d.bias' % idx, (1,))]
    layers.append(dict(key='model.%d.' % idx, cin=ndf * mult, cout=1, stride=1, bias=True, norm=False, last=True, kh=4, pad=1))
    return spec, layers


def fold_batchnorm_fsd(sd, eps=1e-5):
    """State_dict of a DSN discriminator with BatchNorm2d (FSD: codes/DSN/model.py:176-189, Conv + BatchNorm2d at net.net.3 / net.net.6; nld_s1 / nld_s2:
    model.py:136-160, bias-free Conv + BatchNorm2d at net.model.3 / net.model.6) -> the equivalent conv-only state_dict of the network in eval() mode:
    BN(z) = (z - mean) / sqrt(var + eps) * gamma + beta is a per-channel affine map of the conv output, folded into the conv's weight and bias (host-side,
    float64, once per load).  Used for inference with BN discriminators (dataset generation, create_dataset_modified.py:147-164)."""
    pre = 'net.model.' if any(k.startswith('net.model.') for k in sd) else 'net.net.'
    out = {}
    for k, v in sd.items():
        if k.split('.')[-1] in ('running_mean', 'running_var', 'num_batches_tracked') or k.startswith((pre + '3.', pre + '6.')):
            continue
        out[k] = v.clone()
    for conv, bn in ((pre + '2.', pre + '3.'), (pre + '5.', pre + '6.')):
        s = sd[bn + 'weight'].double() / torch.sqrt(sd[bn + 'running_var'].double() + eps)
        out[conv + 'weight'] = (sd[conv + 'weight'].double() * s.view(-1, 1, 1, 1)).float()
        b = sd[conv + 'bias'].double() if (conv + 'bias') in sd else torch.zeros_like(s)
        out[conv + 'bias'] = ((b - sd[bn + 'running_mean'].double()) * s + sd[bn + 'bias'].double()).float()
    # (the folded network has a bias on every conv: re-insert the keys in the order of its spec)
    order = [k for i in (0, 2, 5, 8) for k in (pre + '%d.weight' % i, pre + '%d.bias' % i)]
    return {k: out[k] for k in list(out) if k not in order} | {k: out[k] for k in order}


def fsd_spec(input_nc, gaussian_k=None, norm='Instance'):
    """DSN DiscriminatorBasic (codes/DSN/model.py:173-210): 5x5 convs (all with bias) and a 1x1 head.  norm 'Instance': InstanceNorm after
    the 2nd / 3rd conv; 'Batch': BatchNorm2d in training mode there (BatchNormDiscriminatorHIP); 'BatchEval': BatchNorm in eval mode, folded
    into those convs (fold_batchnorm_fsd), i.e. no norm op at all.
    gaussian_k: the frozen depthwise gaussian of the 'gau' front end is part of the reference state_dict."""
    spec = []
    if gaussian_k:
        spec.append(('filter.filter_low.filter.gaussian_filter.weight', (3, 1, gaussian_k, gaussian_k)))
    layers = []
    nrm = {'Instance': True, 'Batch': 'batch', 'BatchEval': False}[norm]
    for idx, cin, cout, kh, norm_l, last in ((0, input_nc, 64, 5, False, False), (2, 64, 128, 5, nrm, False), (5, 128, 256, 5, nrm, False),
                                             (8, 256, 1, 1, False, True)):
        key = 'net.net.%d.' % idx
        spec += [(key + 'weight', (cout, cin, kh, kh)), (key + 'bias', (cout,))]
        bn = None
        if norm_l == 'batch':   # nn.BatchNorm2d right after the conv (model.py:181-187): affine parameters in the optimiser, buffers beside it
            bn = 'net.net.%d.' % (idx + 1)
            spec += [(bn + 'weight', (cout,)), (bn + 'bias', (cout,))]
        layers.append(dict(key=key, cin=cin, cout=cout, stride=1, bias=True, norm=norm_l, bn=bn, last=last, kh=kh, pad=(kh - 1) // 2))
    return spec, layers


def dsn_nld_spec(input_nc, stride, gaussian_k=None, ndf=64, norm='Instance'):
    """DSN `--discriminator nld_s1 / nld_s2` (codes/DSN/model.py:84-89,121-170): NLayerDiscriminator(n_layers=2, kw=4, padw=1) with stride 1 or 2
    in its first two convs.  norm 'Instance': `use_bias` is True, the normalised convs DO carry a bias (it cancels in the norm: zero gradient);
    'Batch' (model.py:139-142: `use_bias` False): bias-free convs, each followed by BatchNorm2d in training mode (BatchNormDiscriminatorHIP);
    'BatchEval': BatchNorm in eval mode folded into those convs (fold_batchnorm_fsd) -- convs with a bias, no norm op."""
    spec = []
    if gaussian_k:
        spec.append(('filter.filter_low.filter.gaussian_filter.weight', (3, 1, gaussian_k, gaussian_k)))
    layers = []
    nrm = {'Instance': True, 'Batch': 'batch', 'BatchEval': False}[norm]
    for idx, cin, cout, st, norm_l, last in ((0, input_nc, ndf, stride, False, False), (2, ndf, 2 * ndf, stride, nrm, False),
                                             (5, 2 * ndf, 4 * ndf, 1, nrm, False), (8, 4 * ndf, 1, 1, False, True)):
        key = 'net.model.%d.' % idx
        bias = norm_l != 'batch'
        spec.append((key + 'weight', (cout, cin, 4, 4)))
        if bias:
            spec.append((key + 'bias', (cout,)))
        bn = None
        if norm_l == 'batch':
            bn = 'net.model.%d.' % (idx + 1)
            spec += [(bn + 'weight', (cout,)), (bn + 'bias', (cout,))]
        layers.append(dict(key=key, cin=cin, cout=cout, stride=st, bias=bias, norm=norm_l, bn=bn, last=last, kh=4, pad=1))
    return spec, layers


BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def vgg128_spec(in_nc, nf=64):
    """Discriminator_VGG_128 (codes/SRN/models/modules/architecture.py:442-495): conv0_0 (bias) + LReLU, nine bias-free convs each with
    BatchNorm2d(affine) + LReLU (3x3 s1 / 4x4 s2 alternating, 128 -> 4 pixels), Linear(512*4*4, 100) + LReLU, Linear(100, 1).  The linear layers
    run as a 4x4 'valid' conv on the 4x4 map and a 1x1 conv (same weight memory order as the flattened [C][H][W] features)."""
    if nf != 64:
        raise NotImplementedError('Discriminator_VGG_128: linear1 is Linear(512 * 4 * 4, 100), i.e. nf = 64')
    chain = [('conv0_0', in_nc, nf, 3, 1, None), ('conv0_1', nf, nf, 4, 2, 'bn0_1'), ('conv1_0', nf, 2 * nf, 3, 1, 'bn1_0'),
             ('conv1_1', 2 * nf, 2 * nf, 4, 2, 'bn1_1'), ('conv2_0', 2 * nf, 4 * nf, 3, 1, 'bn2_0'), ('conv2_1', 4 * nf, 4 * nf, 4, 2, 'bn2_1'),
             ('conv3_0', 4 * nf, 8 * nf, 3, 1, 'bn3_0'), ('conv3_1', 8 * nf, 8 * nf, 4, 2, 'bn3_1'), ('conv4_0', 8 * nf, 8 * nf, 3, 1, 'bn4_0'),
             ('conv4_1', 8 * nf, 8 * nf, 4, 2, 'bn4_1')]
    spec, layers = [], []
    for name, cin, cout, kh, stride, bn in chain:
        spec.append((name + '.weight', (cout, cin, kh, kh)))
        if bn is None:
            spec.append((name + '.bias', (cout,)))
        else:
            spec += [(bn + '.weight', (cout,)), (bn + '.bias', (cout,))]
        layers.append(dict(key=name + '.', cin=cin, cout=cout, stride=stride, bias=bn is None, norm='batch' if bn else False, bn=(bn + '.') if bn else None,
                           last=False, kh=kh, pad=1))
    spec += [('linear1.weight', (100, 8 * nf, 4, 4)), ('linear1.bias', (100,)), ('linear2.weight', (1, 100, 1, 1)), ('linear2.bias', (1,))]
    layers.append(dict(key='linear1.', cin=8 * nf, cout=100, stride=1, bias=True, norm=False, bn=None, last=False, kh=4, pad=0))
    layers.append(dict(key='linear2.', cin=100, cout=1, stride=1, bias=True, norm=False, bn=None, last=True, kh=1, pad=0))
    return spec, layers


# stride-2 4x4 data-gradient = four 2x2 sub-convolutions, one per parity (py, px) of the input pixel:
# packed tap a (0/1) along one axis -> source tap k and zero-padding of the sub-conv (see DESIGN.md / conv.hip)
_PARITY_TAPS = {0: (3, 1), 1: (2, 0)}  # parity -> (k for a=0, k for a=1)
_PARITY_PAD = {0: 1, 1: 0}


class NLayerDiscriminatorHIP:
    prec = int(__import__('os').environ.get('DASR_D_PREC', '4'))   # 4: split-f16 operands (22 bits, default since round 2; DiscriminatorVGG128HIP always); 3: split-bf16 (16 bits)

    def __init__(self, input_nc, ndf=64, n_layers=2, device='cuda', spec_layers=None):
        self.input_nc, self.device = input_nc, torch.device(device)
        self.spec, self.layers = spec_layers if spec_layers is not None else nlayer_d_spec(input_nc, ndf, n_layers)
        self.params = ParamStore(self.spec, self.device)
        self.pack = PackRegistry(self.params)
        P = self.params
        for L in self.layers:
            cin_pad = ceil_div(L['cin'], 16) * 16
            w = P.off(L['key'] + 'weight')
            L['cin_pad'] = cin_pad
            nt = L['kh'] * L['kh']
            L['fwd'] = self.pack.add(L['cout'], cin_pad, nt, 1, self.prec, [(w, L['cout'], L['cin'], 0, L['cin'], 0, 0)])
            cb = ceil_div(L['cout'], 16) * 16
            if L['stride'] == 1:
                L['bwd'] = self.pack.add(L['cin'], cb, nt, 1, self.prec, [(w, L['cout'], L['cin'], 0, L['cout'], 0, 1)])
            else:
                L['bwd'] = {}
                for py in (0, 1):
                    for px in (0, 1):
                        tm = [_PARITY_TAPS[py][a] * 4 + _PARITY_TAPS[px][b] for a in (0, 1) for b in (0, 1)]
                        L['bwd'][(py, px)] = self.pack.add(L['cin'], cb, 4, 1, self.prec, [(w, L['cout'], L['cin'], 0, L['cout'], 0, 1)],
                                                           tapmap=tm, src_ntaps=16)
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
            self.plans[k] = _DPlan(self, N, H, W)
        return self.plans[k]


class BatchNormDiscriminatorHIP(NLayerDiscriminatorHIP):
    """A discriminator whose layer table has BatchNorm2d (training mode) entries (`norm == 'batch'`, parameter prefix `bn`).
    Batch statistics are taken per call of the reference = per half [fake | real] of the batch (`bn_groups`), on this rank's samples; the running
    statistics live outside the optimiser's buffers and are updated by `_DPlan.running_ops(group)` in the order of the reference's forwards."""
    bn_groups = 2
    prec = 4   # the BatchNorm backward cancels group means: 16-bit conv operands leave 4e-2 on the first layers' gradients, 22-bit ones 1e-3
    # weight gradients with 22-bit operands too (round 4): dW = g.x + g.x_lo + g_lo.x, x_lo / g_lo = what the f16 rounding of the staged operand
    # drops (dasr_f16_residual), three parts of one launch of the f16 weight-gradient kernel.  With 11-bit operands the DASR step's D_source
    # gradients were 1.3e-2 off an fp64 run of the reference step; emulated on the oracle: 4.6e-3 -> 1.9e-3 (oracle/bn_probe.py)
    split_wgrad = True

    def __init__(self, input_nc, device='cuda', spec_layers=None):
        super().__init__(input_nc, device=device, spec_layers=spec_layers)
        self.buffers = {}
        for L in self.layers:
            if L['norm'] == 'batch':
                self.buffers[L['bn'] + 'running_mean'] = torch.zeros(L['cout'], dtype=torch.float32, device=self.device)
                self.buffers[L['bn'] + 'running_var'] = torch.ones(L['cout'], dtype=torch.float32, device=self.device)
                self.buffers[L['bn'] + 'num_batches_tracked'] = torch.zeros(1, dtype=torch.float32, device=self.device)

    def state_dict(self):
        """the reference module's keys, order and shapes (BN buffers after the BN bias, num_batches_tracked int64)"""
        from collections import OrderedDict
        flat, out = self.params.state_dict(), OrderedDict()
        bn_bias = {L['bn'] + 'bias': L['bn'] for L in self.layers if L['norm'] == 'batch'}
        for k, v in flat.items():
            out[k] = v
            if k in bn_bias:
                pre = bn_bias[k]
                out[pre + 'running_mean'] = self.buffers[pre + 'running_mean'].detach().clone().cpu()
                out[pre + 'running_var'] = self.buffers[pre + 'running_var'].detach().clone().cpu()
                out[pre + 'num_batches_tracked'] = self.buffers[pre + 'num_batches_tracked'].detach().cpu().round().long().reshape(())
        return out

    def load_state_dict(self, sd, strict=True):
        own = {}
        for k, v in sd.items():
            if k in self.buffers:
                self.buffers[k].copy_(v.detach().float().reshape(self.buffers[k].shape).to(self.device))
            elif k in self.params.spec:
                own[k] = v.detach().float().reshape(self.params.spec[k][1])
            elif strict:
                raise RuntimeError('Error(s) in loading state_dict: unexpected key %s' % k)
        missing = [k for k in list(self.params.spec) + list(self.buffers) if k not in sd]
        if strict and missing:
            raise RuntimeError('Error(s) in loading state_dict: missing %s' % missing)
        self.params.load_state_dict(own, strict=False)
        self.repack()


class DiscriminatorVGG128HIP(BatchNormDiscriminatorHIP):
    """`which_model_pairD: discriminator_vgg_128` (networks.py:201-202): the source-domain discriminator with BatchNorm in training mode (the
    reference's nn.DataParallel replicas do not synchronise BatchNorm either); running statistics follow the reference's three forwards per
    step (fake in the G step, real and fake in the D step)."""

    def __init__(self, in_nc, nf=64, device='cuda'):
        super().__init__(in_nc, device=device, spec_layers=vgg128_spec(in_nc, nf))

    def state_dict(self):
        """Linear weights 2-D as in the reference module"""
        from collections import OrderedDict
        return OrderedDict((k, v.reshape(v.shape[0], -1) if k.startswith('linear') and k.endswith('weight') else v) for k, v in super().state_dict().items())


def vgg128_init_state_dict(spec, seed):
    """init_weights('kaiming', scale=1) of networks.py:30-44,227: kaiming-normal(fan_in) convs and linears, zero biases, BatchNorm weight 1 / bias 0
    (values from one seeded generator; not the reference's RNG stream)"""
    import math
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in spec:
        if k.startswith('bn'):
            sd[k] = torch.ones(shape) if k.endswith('weight') else torch.zeros(shape)
        elif k.endswith('weight'):
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        else:
            sd[k] = torch.zeros(shape)
    return sd


def gaussian_kernel2d(k):
    """GaussianFilter weights (architecture.py:1177-1199)"""
    mean, var = (k - 1) / 2.0, (k / 6.0) ** 2.0
    ax = torch.arange(k, dtype=torch.float32)
    xx = ax.repeat(k).view(k, k)
    g = torch.exp(-((xx - mean) ** 2 + (xx.t() - mean) ** 2) / (2 * var))
    return g / g.sum()


def _null(t):
    return t is None or t.p is None


class FreqSplit:
    """The frequency-separation front end of the GAN trainers: Haar wavelet (dasr_dwt_fwd / _bwd) or a k x k low-pass (dasr_lowpass / _valid) with
    the high band 0.5 + 0.5 (x - low(x)).  A model builds it once from its options (srn / dsn); the plans ask it for the ops to add, so the
    kernel, the filter weights and the flag words are chosen here and nowhere else.  x, the outputs and the gradients are dasr_tensor views of N
    three-channel images, (H, W) is the size of the image itself; an absent output or gradient is None (or NULL_T)."""

    def __init__(self, wavelet, gaussian, k, device, a_h=0.5, b_h=0.5, dwt_norm=1, valid_bit=0):
        self.wavelet, self.k = bool(wavelet), int(k)
        w = gaussian_kernel2d(self.k) if gaussian else torch.full((self.k, self.k), 1.0 / (self.k * self.k))
        self.w = w.contiguous().to(device)       # the k x k filter (a wavelet model has it for its image views: DASR_Model.filter_high)
        self.a_h, self.b_h = a_h, b_h            # a_h / b_h of dasr_lowpass: scale and offset of the high band
        self.valid_bit = valid_bit               # `mode` bit 1 (value 2) of dasr_lowpass: the box average counts only the pixels inside the image
        self.dwt_norm = dwt_norm                 # `norm` of dasr_dwt_fwd / _bwd: 1 = bands normalised to [0, 1], 2 = 'sum' format (LH + HL + HH) / 3
        self.in_nc = 9 if (self.wavelet and not dwt_norm & 2) else 3   # channels the discriminator sees

    @classmethod
    def srn(cls, fs, k, norm, device):
        """train options fs ('wavelet', 'gau', 'avgpool': count_include_pad=True), fs_kernel_size, norm of the SRN trainer"""
        if fs not in ('wavelet', 'gau', 'avgpool'):
            raise NotImplementedError('FS type [{:s}] not recognized.'.format(str(fs)))
        a_h, b_h = (0.25, 0.75) if norm else (0.5, 0.5)   # FilterHigh normalises, filter_func normalises again (App. C-11)
        return cls(fs == 'wavelet', fs != 'avgpool', k or 5, device, a_h, b_h, dwt_norm=int(bool(norm)))

    @classmethod
    def dsn(cls, filter, k, cat_or_sum, device):
        """--filter ('gau', 'avg_pool': count_include_pad=False, 'wavelet'), --kernel_size, --cat_or_sum of the DSN trainer"""
        if filter not in ('gau', 'avg_pool', 'wavelet'):
            raise NotImplementedError('Frequency Separation type [{:s}] not recognized'.format(filter))
        if cat_or_sum not in ('cat', 'sum'):
            raise NotImplementedError('Wavelet format [{:s}] not recognized'.format(str(cat_or_sum)))
        return cls(filter == 'wavelet', filter != 'avg_pool', k, device, dwt_norm=1 | (2 if cat_or_sum == 'sum' else 0),
                   valid_bit=2 if filter == 'avg_pool' else 0)

    def out_size(self, h, w):
        """size of the bands of an h x w image"""
        return (h // 2, w // 2) if self.wavelet else (h, w)

    def colour_size(self, h, w):
        """size of colour() of an h x w image"""
        return (h // 2, w // 2) if self.wavelet else (h - self.k + 1, w - self.k + 1)

    def _dwt(self, kind, N, H, W, **args):
        return make_op(kind, N=N, C=3, H2=H // 2, W2=W // 2, **args)

    def _lowpass(self, kind, N, H, W, **args):
        return make_op(kind, w=self.w.data_ptr(), k=self.k, N=N, C=3, H=H, W=W, **args)

    def split(self, x, N, H, W, low=None, high=None):
        """x -> the low band and / or the high band(s); no op when neither is wanted"""
        if _null(low) and _null(high):
            return []
        if self.wavelet:
            return [self._dwt(_lib.OP_DWT_FWD, N, H, W, x=x, norm=self.dwt_norm, ll=low, hc=high)]
        return [self._lowpass(_lib.OP_LOWPASS, N, H, W, x=x, mode=self.valid_bit, a_h=self.a_h, b_h=self.b_h, out_low=low, out_high=high)]

    def tangent(self, x, N, H, W, out):
        """the linear part of the high band (no offset) of x"""
        if self.wavelet:
            return [self._dwt(_lib.OP_DWT_FWD, N, H, W, x=x, norm=self.dwt_norm | 4, hc=out)]
        return [self._lowpass(_lib.OP_LOWPASS, N, H, W, x=x, mode=self.valid_bit, a_h=self.a_h, out_high=out)]

    def colour(self, x, N, H, W, out):
        """the DSN colour filter (loss.py:50-58,103-107): low-pass without padding, or Haar LL * 0.5"""
        if self.wavelet:
            return [self._dwt(_lib.OP_DWT_FWD, N, H, W, x=x, norm=1, ll=out)]
        return [self._lowpass(_lib.OP_LOWPASS_VALID, N, H, W, x=x, out=out)]

    def adjoint(self, dst, N, H, W, g_low=None, g_high=None, g_colour=None):
        """dst += adjoint of split() on (g_low, g_high) and of colour() on g_colour.  The wavelet takes them in ONE op (g_colour in the place of
        g_low: a plan has one or the other); the low-pass records one op for the bands and one for the colour filter."""
        assert _null(g_low) or _null(g_colour)
        if self.wavelet:
            gll = g_colour if _null(g_low) else g_low
            if _null(gll) and _null(g_high):
                return []
            return [self._dwt(_lib.OP_DWT_BWD, N, H, W, gll=gll, ghc=g_high, norm=self.dwt_norm, gx=dst, accumulate=1)]
        ops = []
        if not (_null(g_low) and _null(g_high)):
            ops.append(self._lowpass(_lib.OP_LOWPASS, N, H, W, x=g_low, x2=g_high, mode=1 | self.valid_bit, a_h=self.a_h, out_low=dst, accumulate=1))
        if not _null(g_colour):
            ops.append(self._lowpass(_lib.OP_LOWPASS_VALID, N, H, W, x=g_colour, mode=1, out=dst, accumulate=1))
        return ops

    def colour_adjoint(self, g, dst, N, H, W):
        """dst += adjoint of colour() on g"""
        return self.adjoint(dst, N, H, W, g_colour=g)


class _DPlan:
    """Forward on N images; data-gradient of the first `n_g` images (generator step, no weight gradients);
    full backward with weight gradients on all N images (discriminator step)."""

    def __init__(self, net, N, H, W, groups=None):
        self.net, self.N = net, N
        dev, P, pack = net.device, net.params, net.pack
        groups = getattr(net, 'bn_groups', 1) if groups is None else groups   # (groups = 1: ONE call of the reference on all N images, e.g. the gradient penalty's D(sample))
        assert N % groups == 0
        self.group = N // groups                       # BatchNorm: images [0, group) = fake half, [group, N) = real half, own statistics each
        self.x = BTensor(N, 16, H, W, True, dev)       # D input (3 or 9 real channels)
        self.gx = BTensor(N, 16, H, W, True, dev)      # dL/d input
        self.acts, self.zs, self.stats, self.dims = [], [], [], [(H, W)]
        h, w = H, W
        for L in net.layers:
            ho = (h + 2 * L['pad'] - L['kh']) // L['stride'] + 1
            wo = (w + 2 * L['pad'] - L['kh']) // L['stride'] + 1
            self.dims.append((ho, wo))
            z = BTensor(N, max(L['cout'], 16), ho, wo, True, dev) if L['norm'] else None
            a = BTensor(N, max(L['cout'], 16), ho, wo, True, dev)
            self.zs.append(z)
            self.acts.append(a)
            self.stats.append(torch.zeros(N * ceil_div(L['cout'], 16) * 16 * 3, dtype=torch.float32, device=dev) if L['norm'] else None)
            h, w = ho, wo
        self.logits = self.acts[-1]
        self.g_logits = BTensor(N, 16, h, w, True, dev)
        # gradient buffers: ga[i] = dL/d acts[i], gz[i] = dL/d (conv output of layer i)
        self.ga = [BTensor(N, a.C, a.H, a.W, True, dev) for a in self.acts[:-1]]
        self.gz = [BTensor(N, a.C, a.H, a.W, True, dev) for a in self.acts[:-1]] + [self.g_logits]
        self.ws = Workspace(dev)
        self.fwd = self._build_fwd(N).tag(9)
        self.bwd_full = self._build_bwd(N, wgrad=True, input_grad=False).tag(10)
        self.bwd_data = {}
        self.ws.finalize()

    _NORM_OPS = {'fwd': (_lib.OP_BNORM_FWD, _lib.OP_INORM_FWD), 'bwd': (_lib.OP_BNORM_BWD, _lib.OP_INORM_BWD),
                 'jvp': (_lib.OP_BNORM_JVP, _lib.OP_INORM_JVP), 'second': (_lib.OP_BNORM_SECOND, _lib.OP_INORM_SECOND)}

    def norm_op(self, i, kind, N, dgamma=None, dbeta=None, **tensors):
        """the normalisation op of layer i on the first N images for the pass `kind` ('fwd', 'bwd', 'jvp', 'second'): the BatchNorm op (on the conv
        output zs[i], with group / gamma / beta) or the InstanceNorm op (forward: zs[i]; the others: the saved activation acts[i]).  tensors: what differs
        from site to site (ga / gx, t / out, accumulate); dgamma / dbeta: where a BatchNorm op adds its parameter gradients (InstanceNorm has none)."""
        L, P = self.net.layers[i], self.net.params
        batch = L['norm'] == 'batch'
        ho, wo = self.dims[i + 1]
        args = dict(N=N, C=L['cout'], H=ho, W=wo, slope=SLOPE, stats=self.stats[i].data_ptr(), **tensors)
        if kind == 'fwd':
            args.update(x=self.zs[i].view(), y=self.acts[i].view(), eps=BN_EPS if batch else IN_EPS)
        else:
            args['x' if batch else 'a'] = (self.zs[i] if batch else self.acts[i]).view()
        if batch:
            args.update(group=self.group, gamma=P.ptr(L['bn'] + 'weight'), beta=P.ptr(L['bn'] + 'bias'))
            if kind == 'bwd':
                args.update(dgamma=dgamma, dbeta=dbeta, pscale=1.0)
            elif kind == 'second':
                args.update(dgamma=dgamma, pscale=1.0)
        return make_op(self._NORM_OPS[kind][0 if batch else 1], **args)

    def _build_fwd(self, N):
        net, P, pack = self.net, self.net.params, self.net.pack
        ops = OpList()
        src = self.x
        for i, L in enumerate(net.layers):
            (hi, wi), (ho, wo) = self.dims[i], self.dims[i + 1]
            bias = P.ptr(L['key'] + 'bias') if L['bias'] else None
            if L['norm']:
                ops.add(conv_op(pack, L['fwd'], src.view(), True, L['cin_pad'], hi, wi, ho, wo, N, bias=bias, kh=L['kh'], stride=L['stride'],
                                pad=L['pad'], out_f32=self.zs[i].view()))
                ops.add(self.norm_op(i, 'fwd', N))
            else:
                ops.add(conv_op(pack, L['fwd'], src.view(), True, L['cin_pad'], hi, wi, ho, wo, N, bias=bias, kh=L['kh'], stride=L['stride'],
                                pad=L['pad'], act=0 if L.get('last') else 1, slope=SLOPE, out_f32=self.acts[i].view()))
            src = self.acts[i]
        return ops

    def _dgrad_ops(self, ops, i, N, g_in, out, mask):
        """dL/d(input of layer i) from g_in = dL/d(conv output of layer i); optional LeakyReLU' mask of the input"""
        net, pack = self.net, self.net.pack
        L = net.layers[i]
        (hi, wi), (ho, wo) = self.dims[i], self.dims[i + 1]
        cb = ceil_div(L['cout'], 16) * 16
        m = mask.view() if mask is not None else None
        gsc = 4096.0 if net.prec == 4 else 0.0   # split-f16: gradients (1e-8 .. 1e-1) pre-scaled by 2^12 into f16's normal range (exact, undone on the accumulator)
        if L['stride'] == 1:
            ops.add(conv_op(pack, L['bwd'], g_in.view(), True, cb, ho, wo, hi, wi, N, kh=L['kh'], stride=1, pad=L['kh'] - 1 - L['pad'], mask=m,
                            mask_f32=1, slope=SLOPE, out_f32=out.view(), in_scale=gsc))
        else:
            for (py, px), ref in L['bwd'].items():
                hs, wsub = (hi - py + 1) // 2, (wi - px + 1) // 2
                ops.add(conv_op(pack, ref, g_in.view(), True, cb, ho, wo, hs, wsub, N, kh=2, stride=1, pad=_PARITY_PAD[py],
                                pad_x=_PARITY_PAD[px], mask=m, mask_f32=1, slope=SLOPE, out_f32=out.view(), out_stride=2, out_oy=py,
                                out_ox=px, out_W=wi, in_scale=gsc))

    def _build_bwd(self, N, wgrad, input_grad):
        """input: self.g_logits.  N may be a prefix of the batch (views start at image 0)."""
        net, P = self.net, self.net.params
        ops = OpList()
        nl = len(net.layers)
        for i in range(nl - 1, -1, -1):
            L = net.layers[i]
            (hi, wi), (ho, wo) = self.dims[i], self.dims[i + 1]
            gz = self.gz[i]
            if L['norm']:  # dL/da -> dL/dz through the norm (BatchNorm: per-half statistics) + LeakyReLU; dgamma / dbeta in the discriminator step
                pg = (P.ptr(L['bn'] + 'weight', P.grad), P.ptr(L['bn'] + 'bias', P.grad)) if (wgrad and L['norm'] == 'batch') else (None, None)
                ops.add(self.norm_op(i, 'bwd', N, ga=self.ga[i].view(), gx=gz.view(), dgamma=pg[0], dbeta=pg[1]))
            inp = self.x if i == 0 else self.acts[i - 1]
            if wgrad:
                split = None
                if getattr(net, 'split_wgrad', False) and net.prec == 4:
                    g_lo, x_lo = BTensor(N, gz.C, gz.H, gz.W, True, net.device), BTensor(N, inp.C, inp.H, inp.W, True, net.device)
                    for src, dst, sc in ((gz, g_lo, 4096.0), (inp, x_lo, 1.0)):
                        ops.add(make_op(_lib.OP_CVT_F16, x=src.view(), N=N, C=src.C, H=src.H, W=src.W, scale=sc, y=dst.view(), form=3))
                    ops.keep += [g_lo, x_lo]
                    split = (g_lo.view, x_lo.view)
                grp = WgradGroup(L['kh'], L['stride'])
                # prec 4 nets: the weight-gradient operands are rounded to f16 (11 bits, gradient pre-scaled) instead of bf16 (8 bits): behind a
                # BatchNorm the output gradient sums to zero over the group, so only the deviation of the input from its mean counts
                grp.add_conv(gz.view, True, gz.planes, inp.view, True, inp.planes, L['cout'], L['cin'], hi, wi, ho, wo, N,
                             P.off(L['key'] + 'weight'), P.off(L['key'] + 'bias') if L['bias'] else None, pad=L['pad'],
                             f16=net.prec == 4, g_scale=4096.0 if net.prec == 4 else 0.0, split=split)
                grp.emit(ops, self.ws, net.device, P.grad.data_ptr())
            if i > 0:
                prev = net.layers[i - 1]
                if prev['norm']:
                    self._dgrad_ops(ops, i, N, gz, self.ga[i - 1], None)        # IN backward applies the LeakyReLU'
                else:
                    self._dgrad_ops(ops, i, N, gz, self.gz[i - 1], self.acts[i - 1])  # plain conv+LeakyReLU layer
            elif input_grad:
                self._dgrad_ops(ops, 0, N, gz, self.gx, None)
        return ops

    def running_ops(self, g):
        """BatchNorm running statistics after a training-mode forward on group g (0 = fake half, 1 = real half): one op per BN layer"""
        ops = OpList()
        for i, L in enumerate(self.net.layers):
            if L['norm'] == 'batch':
                ho, wo = self.dims[i + 1]
                B = self.net.buffers
                ops.add(make_op(_lib.OP_BNORM_RUNNING, stats=self.stats[i].data_ptr(), g=g, C=L['cout'], count=self.group * ho * wo, momentum=BN_MOMENTUM,
                                running_mean=B[L['bn'] + 'running_mean'].data_ptr(), running_var=B[L['bn'] + 'running_var'].data_ptr(),
                                num_batches_tracked=B[L['bn'] + 'num_batches_tracked'].data_ptr()))
        return ops

    def bwd_data_ops(self, n):
        """data-gradient only (generator step) for the first n images"""
        if n not in self.bwd_data:
            ws_before = self.ws.need
            self.bwd_data[n] = self._build_bwd(n, wgrad=False, input_grad=True).tag(10)
            assert self.ws.need == ws_before
        return self.bwd_data[n]


# ---------------------------------------------------------------------------------------------------------------------
VGG19_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M']
VGG_MEAN, VGG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


VGG16_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']


def vgg19_spec(feature_layer=34, cfg=None):
    """torchvision vgg19 (or `cfg`) .features[: feature_layer + 1] as [(kind, idx, cin, cout, relu)]"""
    layers, spec, idx, c = [], [], 0, 3
    for v in (cfg or VGG19_CFG):
        if idx > feature_layer:
            break
        if v == 'M':
            layers.append(('pool', idx, c, c, False))
            idx += 1
        else:
            relu = (idx + 1) <= feature_layer
            layers.append(('conv', idx, c, v, relu))
            spec += [('features.%d.weight' % idx, (v, c, 3, 3)), ('features.%d.bias' % idx, (v,))]
            c = v
            idx += 2
    return spec, layers


class VGGFeatureHIP:
    """Frozen feature extractor: forward on N images, data-gradient w.r.t. the first n_g inputs."""

    def __init__(self, feature_layer=34, device='cuda', cfg=None, prec=None, bwd_prec=None, mse_target=False):
        """prec 4 (default): split-f16 operands on f32 tensors (f16 hi + lo pairs, 22 mantissa bits, 3 MFMA passes; gradients pre-scaled by a
        power of two): input-gradient error 4.9e-6 against the fp32 oracle.  prec 3: split-bf16 (16 bits), same cost: 6.5e-3 on the input
        gradient (max-pool arg-max flips on 16-bit ties), the default until round 2.  prec 2: activations and gradients stored in f16
        (11-bit mantissa; gradients pre-scaled by a power of two), one f16 MFMA pass on the LDS-DMA dense-conv kernel: the full GAN step
        drops from 101 to 84 ms, but over the 16 un-damped layers the operand rounding adds up to 1.0e-3 on the features, and max-pool's
        arg-max routing turns 11-bit ties into an 11 % normwise error of dL/dx (1.2-1.6e-2 on the generator gradient of the full step) with
        the seeded-random VGG of the fixtures -- outside the 1e-3 / 1e-2 tolerances, so it is an opt-in (DASR_VGG_PREC=2), not the
        default.  prec 1: plain bf16 operands on f32 tensors (8x coarser than f16)."""
        import os
        self.device = torch.device(device)
        self.prec = int(prec if prec is not None else os.environ.get('DASR_VGG_PREC', '5'))
        self.f16s = self.prec == 2
        # prec 5 (round 3, default): the SAME 22-bit operands as prec 4, but activations and gradients are STORED split (f16 hi planes + f16
        # remainder planes, 4 bytes per element like f32) so that the three products hi*hi + lo*hi + hi*lo are one launch of the LDS-DMA dense-conv
        # kernel over 3K virtual chunks (dasr_conv_params::in_wrap) instead of three passes of the register-staged first-generation kernel
        self.split = self.prec == 5
        # prec 5, data gradient: the gradients are NOT what decides max-pool's arg-max routing or the ReLU masks (the forward activations are, and
        # they keep 22 bits), so their rounding enters dL/dx like noise: one f16 pass (11-bit gradients and weights, pre-scaled) instead of three
        # on split gradients -- 3 of the 7 pass-equivalents of the perceptual network become 1.  DASR_VGG_BWD_PREC=5: three passes.
        self.bwd_prec = int(bwd_prec if bwd_prec is not None else os.environ.get('DASR_VGG_BWD_PREC', '2')) if self.split else self.prec
        # images [n_g, N) of a plan carry no gradient (the real HR half of the DASR feature loss, DASR_model.py:225; the bicubic LR half of the DSN
        # perceptual loss, loss.py:119-130): their features are only the TARGET of an L1 / MSE, so the operand rounding of a single f16 MFMA pass
        # (1e-3 on the features, zero-mean) enters the loss value in second order and the gradient only through sign flips of near-ties.  One
        # pass instead of three on a third of the perceptual network's work.  DASR_VGG_NOGRAD_PREC=0: same precision as the gradient half.
        # mse_target (feature_criterion l2, the DSN's VGG16 MSE): the gradient is 2 (f_fake - f_target) / n, the target's rounding error enters it in
        # FIRST order, so the target half keeps the precision of the gradient half unless the environment variable asks for the one-pass form.
        self.nograd_prec = int(os.environ.get('DASR_VGG_NOGRAD_PREC', '0' if mse_target else '2')) if self.prec in (3, 4, 5) else 0
        # the storage forms a plan records with: activations up to the last conv, gradients below it, and what the launch of the no-gradient images
        # reads and writes (of split tensors the hi planes only: their lo planes stay zero)
        self.act_form = SPLIT if self.split else (F16 if self.f16s else F32)
        self.grad_form = {2: F16, 5: SPLIT}.get(self.bwd_prec, F32)
        self.nograd_form = F16 if self.split else self.act_form
        self.nograd_tag = 7 if self.split else 6   # time bucket of the no-gradient launches; inherited: only the split builder ever tagged them 7
        self.spec, self.layers = vgg19_spec(feature_layer, cfg)
        self.params = ParamStore(self.spec, self.device)
        self.pack = PackRegistry(self.params)
        P = self.params
        self.pk = {}
        for kind, idx, cin, cout, relu in self.layers:
            if kind != 'conv':
                continue
            w = P.off('features.%d.weight' % idx)
            cin_pad = ceil_div(cin, 16) * 16
            mt_f = 2 if (self.prec in (1, 2, 5) and cout % 64 == 0) else 1
            mt_b = 2 if (self.prec in (1, 2, 5) and cin % 64 == 0) else 1
            v3 = 3 if self.split else 1   # split tensors: 3K virtual chunks [hi | hi | lo]
            self.pk[idx] = self.pack.add(cout, v3 * cin_pad, 9, mt_f, self.prec, [(w, cout, cin, 0, cin, 0, 0)])
            if self.split and self.bwd_prec == 2:
                self.pk[(idx, 'b')] = self.pack.add(cin, cout, 9, mt_b, 2, [(w, cout, cin, 0, cout, 0, 1)])
            else:
                self.pk[(idx, 'b')] = self.pack.add(cin, v3 * cout, 9, mt_b, self.prec, [(w, cout, cin, 0, cout, 0, 1)])
            if self.nograd_prec and self.nograd_prec != self.prec:   # forward of the images that carry no gradient (see plan())
                self.pk[(idx, 'r')] = self.pack.add(cout, cin_pad, 9, 2 if cout % 64 == 0 else 1, self.nograd_prec, [(w, cout, cin, 0, cin, 0, 0)])
        self.pack.finalize()
        self.plans = {}

    def load_state_dict(self, sd, strict=True):
        self.params.load_state_dict(sd, strict)
        self.pack.run()

    def state_dict(self):
        return self.params.state_dict()

    def plan(self, N, n_g, H, W):
        k = (N, n_g, H, W)
        if k not in self.plans:
            npool = sum(1 for L in self.layers if L[0] != 'conv')
            if (H >> npool) < 1 or (W >> npool) < 1:   # (torch raises "Output size is too small" from the pool that would produce an empty map)
                raise ValueError('images of %dx%d are too small for this feature extractor: %d 2x2 max-pools need at least %d pixels per side' % (H, W, npool, 1 << npool))
            self.plans[k] = _VGGPlan(self, N, n_g, H, W)
        return self.plans[k]


class _VGGPlan:
    """One forward and one backward walk over net.layers.  How a tensor is stored and what the ops that touch it pass come from the network's
    storage forms (engine.StorageForm): activations up to the last conv in net.act_form, gradients below it in net.grad_form.  In every form the
    last conv writes f32, a pool behind it (vgg16.features[:31]) runs in f32, and the feature map and dL/dx are f32."""

    def __init__(self, net, N, n_g, H, W):
        self.net, self.N, self.n_g = net, N, n_g
        # EVERY tensor an op of this plan points at must stay referenced: the ops hold raw device pointers.  (Until round 3 the intermediate
        # gradient tensors of the backward chain were locals of the builder: freed when it returned, their memory stayed untouched only as long as
        # the caching allocator did not hand it out again -- the cause of a rare non-finite-gradient failure of the DSN fixtures.)
        self._keep = []
        dev, P, pack = net.device, net.params, net.pack
        act, grad = net.act_form, net.grad_form

        def new(form, C_, h, w):
            self._keep.append(form.alloc(N, C_, h, w, dev))
            return self._keep[-1]
        self.x_flag = act.code                    # dtype code of x for dasr_affine4
        self.x = new(act, 16, H, W)               # normalised input
        self.outs = []
        lc = max(i for i, L in enumerate(net.layers) if L[0] == 'conv')   # last conv: the hand-off to f32
        # the images [n_g, N) that carry no gradient: a launch of their own in net.nograd_form (see VGGFeatureHIP.__init__)
        one_pass = net.nograd_prec not in (0, net.prec) and 0 < n_g < N
        h, w = H, W
        fwd = OpList()
        src = self.x
        for li, (kind, idx, cin, cout, relu) in enumerate(net.layers):
            form = act if li < lc else F32
            if kind == 'conv':
                out = new(form, cout, h, w)
                kw = dict(Hin=h, Win=w, Hout=h, Wout=w, bias=P.ptr('features.%d.bias' % idx), act=1 if relu else 0, slope=0.0)
                fwd.add(conv_op(pack, net.pk[idx], N=n_g if one_pass else N, **act.conv_in(src, cin), **form.conv_out(out, cout), **kw))
                if one_pass:
                    rform = net.nograd_form if li < lc else F32
                    fwd.add(conv_op(pack, net.pk[(idx, 'r')], N=N - n_g, **net.nograd_form.conv_in(src, cin, n_g), **rform.conv_out(out, cout, n_g), **kw))
                    fwd.ops[-1].set('tag', net.nograd_tag)
            else:
                h, w = h // 2, w // 2
                out = new(form, cout, h, w)
                # Win: input width (odd widths: the last column is dropped)
                fwd.add(make_op(_lib.OP_MAXPOOL, x=src.view(), N=N, C=cout, Ho=h, Wo=w, is_f32=form.code, y=out.view(), Win=src.W))
            self.outs.append(out)
            src = out
        self.feat = src
        self.fwd = fwd.tag(6)
        # data gradient for the first n_g images.  Gradients handed between layers are w.r.t. PRE-activation values:
        # a dgrad conv's epilogue applies the ReLU' of the layer that produced its input; a pool's backward applies the
        # ReLU' of the conv feeding the pool (every VGG pool follows a ReLU).
        n = n_g
        self.g_feat = new(F32, self.feat.C, self.feat.H, self.feat.W)
        self.gx = new(F32, 16, H, W)
        # dL/dfeat of a mean loss over n_g x C x h x w elements is ~1 / count: a power-of-two pre-scale keeps its 16-bit roundings in f16's normal range
        prescale = grad_prescale(n_g * self.feat.C * self.feat.H * self.feat.W)
        if grad.f32:   # prec 4 rounds f32 gradients to f16 pairs inside each conv (in_scale); the other f32 precisions do not scale
            in_scale = prescale if net.prec == 4 else 0.0
        else:          # 16-bit gradients: one conversion at the last conv multiplies by gscale, the conv of layer 0 divides it out
            self.gscale, in_scale = prescale, 0.0
        bwd = OpList()
        g = self.g_feat
        for li in range(len(net.layers) - 1, -1, -1):
            kind, idx, cin, cout, relu = net.layers[li]
            inp = self.x if li == 0 else self.outs[li - 1]
            if kind == 'conv':
                if li == lc and not grad.f32:   # f32 gradient of the last conv's output -> pre-scaled tensor of the gradient form
                    gs = new(grad, cout, g.H, g.W)
                    bwd.add(make_op(_lib.OP_CVT_F16, x=g.view(), N=n, C=cout, H=g.H, W=g.W, scale=self.gscale, y=gs.view(), form=grad.cvt_form))
                    g = gs
                gin = self.gx if li == 0 else new(grad, cin, inp.H, inp.W)
                if li == 0 and not grad.f32:   # dL/d(normalised input): f32, un-scaled  (no mask; slope stays at conv_op's default: inherited)
                    kw = dict(alpha=1.0 / self.gscale)
                else:   # mask = sign of the forward activation; of a 16-bit one: of its hi plane (a non-zero value never rounds to a zero of the other sign)
                    prev_relu = li > 0 and net.layers[li - 1][0] == 'conv' and net.layers[li - 1][4]
                    kw = dict(mask=inp.view() if prev_relu else None, mask_f32=int(act.f32), slope=0.0, in_scale=in_scale)
                bwd.add(conv_op(pack, net.pk[(idx, 'b')], Hin=inp.H, Win=inp.W, Hout=inp.H, Wout=inp.W, N=n, **grad.conv_in(g, cout),
                                **(F32 if li == 0 else grad).conv_out(gin, cin), **kw))
            else:
                aform, gform = (F32, F32) if li > lc else (act, grad)
                gin = new(gform, cout, inp.H, inp.W)
                bwd.add(make_op(_lib.OP_MAXPOOL_BWD, x=inp.view(), gy=g.view(), N=n, C=cout, Ho=g.H, Wo=g.W, is_f32=aform.pool_bwd(gform), relu_mask=1,
                                gx=gin.view(), Win=inp.W))
            g = gin
        self.bwd = bwd.tag(8)

    def input_copy_op(self, src_view, n0, n, H, W):
        """op that writes `n` images of a blocked f32 tensor (<= 16 channels) into x[n0 : n0 + n] (DSN: no input normalisation)"""
        dst, form = self.x.view(n0=n0), self.net.act_form
        if form.f32:
            return make_op(_lib.OP_AXPBY, x=src_view, a=1.0, N=n, C=16, H=H, W=W, out_f32=dst, gamma=1.0)
        return make_op(_lib.OP_CVT_F16, x=src_view, N=n, C=16, H=H, W=W, scale=1.0, y=dst, form=form.cvt_form)

