"""GPU parity tests of the small kernels of csrc/misc.hip and the first half of csrc/gan.hip -- axpby, affine4, the two down-sums, pixel shuffle /
unshuffle, max-pool forward / backward, the pixel and feature losses, sigmoid, fill, add, Adam and its two guard words -- in every mode
include/dasr_hip.h documents, against the fp64 references of oracle/blocked_ref.py (themselves held to stock torch by tests/test_blocked_ref.py).

Set-up of every case: tensors are planes [c0, c0 + K) of a wider slab (n_stride != K * cb_stride), the whole output slab holds a sentinel before the
call and everything outside the view must hold it bit for bit afterwards; channel counts 3 / 20 / 40, odd H and W, N = 2.  Ops with a DASR_OP_* kind
run through the ctypes entry point (via = abi) and through make_op + OpList.run (via = op: the dasr_run_ops switch on the device).

What is asserted: data movement bit for bit; a 16-bit copy against the kernel's own f32 output bit for bit; arithmetic by |got - ref| <= k u magnitude
with u32 = 2^-24, u16 = 2^-11 (f16) / 2^-8 (bf16), k = the number of roundings in the kernel's expression (a fused multiply-add counted as two),
derived beside each assertion; the grid sums by L u32 coef sum |terms| with L the longest chain of roundings behind the accumulator."""
import ctypes as C
import re

import pytest
import torch

from oracle import blocked_ref as R

EINVAL = -22
SENT = -1234.5
U32 = R.U32
IBITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
gpu = pytest.mark.gpu
VIA = pytest.mark.parametrize('via', ['abi', 'op'])


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def gen(seed):
    return torch.Generator().manual_seed(seed)


def biteq(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(IBITS[a.dtype]), b.view(IBITS[b.dtype]))


def _entries():
    from dasr_amd import _lib as L
    return {
        'axpby': (L.OP_AXPBY, ['x', 'a', 'z', 'b', 'N', 'C', 'H', 'W', 'out_f32', 'out_bf16', 'gamma', 'mask', 'slope', 'slope_ptr']),
        'downsum2x': (L.OP_DOWNSUM, ['src', 'N', 'C', 'H', 'W', 'mask', 'mask_f32', 'slope', 'dst_f32', 'dst_bf16']),
        'downsum2x_f16': (L.OP_DOWNSUM_F16, ['src', 'N', 'C', 'H', 'W', 'mask', 'slope', 'out_scale', 'dst_f32', 'dst_f16']),
        'pixel_shuffle_f16': (L.OP_PIXSHUF, ['src', 'N', 'C4', 'H', 'W', 'dst']),
        'pixel_unshuffle_f16': (L.OP_PIXUNSHUF, ['gsrc', 'mask', 'slope', 'N', 'C4', 'H', 'W', 'gdst']),
        'maxpool2': (L.OP_MAXPOOL, ['x', 'is_f32', 'N', 'C', 'Ho', 'Wo', 'y', 'Win']),
        'maxpool2_bwd': (L.OP_MAXPOOL_BWD, ['x', 'gy', 'is_f32', 'N', 'C', 'Ho', 'Wo', 'gx', 'relu_mask', 'Win']),
        'affine4': (L.OP_AFFINE4, ['x', 'N', 'C', 'H', 'W', 'scale4', 'shift4', 'y', 'y_f32', 'accumulate']),
        'l1_diff': (L.OP_L1DIFF, ['a', 'b', 'is_f32', 'N', 'C', 'H', 'W', 'coef', 'gcoef', 'loss_acc', 'ga']),
        'l1_loss': (L.OP_L1LOSS, ['sr', 'hr_nchw', 'weight_map', 'N', 'C', 'H', 'W', 'coef', 'loss_acc', 'grad', 'accumulate', 'grad_scale']),
        'sigmoid_fwd': (L.OP_SIGMOID_FWD, ['x', 'N', 'C', 'H', 'W', 'y']),
        'fill_f32': (L.OP_FILL, ['p', 'n', 'value']),
        'add_flat': (L.OP_ADD_FLAT, ['y', 'x', 'n']),
        # tests/test_gpu_filters.py
        'dwt_fwd': (L.OP_DWT_FWD, ['x', 'N', 'C', 'H2', 'W2', 'norm', 'll', 'hc']),
        'dwt_bwd': (L.OP_DWT_BWD, ['gll', 'ghc', 'N', 'C', 'H2', 'W2', 'norm', 'gx', 'accumulate']),
        'lowpass': (L.OP_LOWPASS, ['x', 'x2', 'w', 'k', 'N', 'C', 'H', 'W', 'mode', 'a_h', 'b_h', 'out_low', 'out_high', 'accumulate']),
        'lowpass_valid': (L.OP_LOWPASS_VALID, ['x', 'w', 'k', 'N', 'C', 'H', 'W', 'mode', 'out', 'accumulate']),
        'ddm_spread': (L.OP_DDM_SPREAD, ['d', 'N', 'n_h', 'n_w', 'H', 'W', 'jump', 'rf', 'start', 'out']),
        'bilinear_up': (L.OP_BILINEAR, ['src', 'N', 'h', 'w', 'factor', 'dst']),
        'logloss': (L.OP_LOGLOSS, ['x', 'N', 'H', 'W', 'mode', 'eps', 'coef', 'gcoef', 'loss_acc', 'score_acc', 'score_coef', 'grad', 'accumulate']),
        'sigmoid_bwd': (L.OP_SIGMOID_BWD, ['y', 'g', 'N', 'C', 'H', 'W', 'gz']),
        # tests/test_gpu_norm_gan.py
        'inorm_lrelu_fwd': (L.OP_INORM_FWD, ['x', 'N', 'C', 'H', 'W', 'eps', 'slope', 'y', 'stats']),
        'inorm_lrelu_bwd': (L.OP_INORM_BWD, ['a', 'ga', 'N', 'C', 'H', 'W', 'slope', 'stats', 'gx']),
        'inorm_lrelu_jvp': (L.OP_INORM_JVP, ['a', 't', 'N', 'C', 'H', 'W', 'slope', 'stats', 'out']),
        'inorm_second': (L.OP_INORM_SECOND, ['a', 't', 'ga', 'N', 'C', 'H', 'W', 'slope', 'stats', 'out', 'accumulate']),
        'grad_penalty': (L.OP_GRAD_PENALTY, ['g', 'N', 'C', 'H', 'W', 'weight', 'part256', 'out3', 'loss_acc', 'stage', 'world']),
        'fill_scaled': (L.OP_FILL_SCALED, ['x', 'N', 'C', 'H', 'W', 'scalar', 'factor']),
        'bnorm_lrelu_fwd': (L.OP_BNORM_FWD, ['x', 'N', 'C', 'H', 'W', 'group', 'eps', 'slope', 'gamma', 'beta', 'y', 'stats']),
        'bnorm_lrelu_bwd': (L.OP_BNORM_BWD, ['x', 'ga', 'N', 'C', 'H', 'W', 'group', 'slope', 'gamma', 'beta', 'stats', 'gx', 'dgamma', 'dbeta', 'pscale']),
        'bnorm_lrelu_jvp': (L.OP_BNORM_JVP, ['x', 't', 'N', 'C', 'H', 'W', 'group', 'slope', 'gamma', 'beta', 'stats', 'out']),
        'bnorm_second': (L.OP_BNORM_SECOND, ['x', 't', 'ga', 'N', 'C', 'H', 'W', 'group', 'slope', 'gamma', 'beta', 'stats', 'out', 'accumulate', 'dgamma',
                                             'pscale']),
        'bnorm_running': (L.OP_BNORM_RUNNING, ['stats', 'g', 'C', 'count', 'momentum', 'running_mean', 'running_var', 'num_batches_tracked']),
        'gan_loss': (L.OP_BCE, ['x', 'N', 'C', 'H', 'W', 'gan_type', 'target', 'coef', 'gcoef', 'loss_acc', 'score_acc', 'score_coef', 'grad']),
        'ragan': (L.OP_RAGAN, ['a', 'b', 'N', 'H', 'W', 'stage', 'n_glob', 'form', 'ta', 'tb', 'coef', 'gcoef', 'eps', 'sums', 'part', 'loss_acc', 'score_a',
                               'score_b', 'score_coef', 'ga', 'gb']),
        # tests/test_gpu_lpips_prelu.py
        'lpips_s2d': (L.OP_LPIPS_S2D, ['x', 'N', 'H', 'W', 'scale4', 'shift4', 'y', 'mode']),
        'maxpool3s2': (L.OP_MAXPOOL3, ['x', 'N', 'C', 'H', 'W', 'y']),
        'maxpool3s2_bwd': (L.OP_MAXPOOL3_BWD, ['x', 'gy', 'N', 'C', 'H', 'W', 'gx', 'relu_mask', 'accumulate']),
        'lpips_head': (L.OP_LPIPS_HEAD, ['f', 'pair_off', 'N', 'C', 'H', 'W', 'lin', 'eps', 'coef', 'gcoef', 'loss_acc', 'g0', 'relu_mask']),
        'prelu_grad': (L.OP_PRELU_GRAD, ['y', 'gx', 'N', 'C', 'H', 'W', 'slope', 'scratch256', 'dst', 'scale']),
        # the same op kind with f16 = 1; as an op it also takes inv_prescale (the executor multiplies it into scale)
        'prelu_grad_f16': (L.OP_PRELU_GRAD, ['y', 'gx', 'N', 'C', 'H', 'W', 'slope', 'scratch256', 'dst', 'scale'], dict(f16=1)),
        'prelu_final': (L.OP_PRELU_FINAL, ['partial', 'nblocks', 'stride', 'count', 'slopes', 'dsts', 'scale']),
    }


def call(via, name, **kw):
    """dasr_<name>(**kw) by argument name, through the ctypes entry point or as a recorded op; arguments left out are NULL / 0.  Returns the code."""
    from dasr_amd import _lib
    from dasr_amd.engine import NULL_T, OpList, _stream
    kind, names, fixed = (_entries()[name] + ({},))[:3]     # fixed: op slots that select this entry point behind a shared op kind
    assert set(kw) <= set(names) | (set(_lib.OP_ARGS[kind]) - set(fixed) if via == 'op' else set()), set(kw) - set(names)
    if via == 'op':
        ol = OpList()
        ol.add(_lib.make_op(kind, **fixed, **kw))
        try:
            ol.run()
            rc = 0
        except _lib.DasrHipError as e:
            rc = int(re.search(r'code (-?\d+)', str(e)).group(1))
    else:
        argv, keep = [], []
        for nm, ty in zip(names, _lib._SIGS['dasr_' + name]):
            v = kw.get(nm)
            if v is None:
                v = NULL_T if ty is _lib.Tensor else (None if ty is _lib.c_vp else 0)
            elif isinstance(v, (list, tuple)):   # scale4 / shift4: HOST pointers (the launcher reads them)
                keep.append((C.c_float * 4)(*v))
                v = C.cast(keep[-1], C.c_void_p)
            argv.append(v)
        rc = getattr(_lib.lib(), 'dasr_' + name)(*argv, _stream())
    torch.cuda.synchronize()
    return rc


class Slab:
    """K planes of a blocked tensor inside a wider sentinel-filled slab: `lead` planes in front, one behind (plain: the K planes alone)"""

    def __init__(self, dev, kind, N, K, H, W, data=None, plain=False, lead=1):
        from dasr_amd.engine import BTensor
        self.p0 = 0 if plain else lead
        tot = K if plain else lead + K + 1
        self.K = K
        self.b = BTensor(N, tot * 16, H, W, kind == 'f32', dev, f16=kind == 'f16')
        self.b.t.fill_(SENT)
        if data is not None:
            assert data.shape == (N, K, H, W, 16) and data.dtype == self.b.t.dtype, (data.shape, data.dtype)
            self.b.t[:, self.p0:self.p0 + K].copy_(data)
        self.before = self.b.t.cpu().clone()

    def view(self):
        v = self.b.view(self.p0 * 16)
        assert self.p0 == 0 or v.n_stride != self.K * v.cb_stride
        return v

    def get(self):
        return self.b.t[:, self.p0:self.p0 + self.K].cpu()

    def nchw(self, C_=None):
        return R.unpack(self.get(), C_)

    def outside_untouched(self):
        now = self.b.t.cpu()
        return biteq(now[:, :self.p0], self.before[:, :self.p0]) and biteq(now[:, self.p0 + self.K:], self.before[:, self.p0 + self.K:])

    def untouched(self):
        return biteq(self.b.t.cpu(), self.before)


def bounded(name, got, ref, bound, margins):
    """|got - ref| <= bound elementwise; the worst ratio goes to the margins log"""
    got = got.double()
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    margins('elementwise %s: worst |err| / bound %.3f' % (name, worst))
    assert bool((err <= bound).all()), '%s: %d elements beyond the bound, worst %.3f of it' % (name, int((err > bound).sum()), worst)


G = 16                                    # guard words around every flat buffer


class Buf:
    """a flat fp32 device buffer between two runs of G sentinel words"""

    def __init__(self, dev, data=None, n=None):
        body = torch.full((n,), SENT) if data is None else data.detach().float().reshape(-1).clone()
        self.n = body.numel()
        self.t = torch.cat([torch.full((G,), SENT), body, torch.full((G,), SENT)]).to(dev)
        self.before = self.t.cpu().clone()
        self.ptr = self.t.data_ptr() + 4 * G

    def get(self):
        return self.t[G:G + self.n].cpu()

    def put(self, data):
        self.t[G:G + self.n] = data.detach().float().reshape(-1).to(self.t.device)

    def guards_ok(self):
        now = self.t.cpu()
        return biteq(now[:G], self.before[:G]) and biteq(now[G + self.n:], self.before[G + self.n:])

    def untouched(self):
        return biteq(self.t.cpu(), self.before)


def ev_ok(name, got, ref, margins):
    bounded(name, got, ref.v, ref.tol(), margins)


def sent_like(t):
    return torch.full_like(t, SENT)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_axpby
AXPBY = [
    # id, C, z, mask ('host' / 'ptr' / None), slope, outputs, gamma, plain
    ('x_f32', 20, False, None, 0.0, 'f32', 1.0, False),
    ('xz_both_g2', 40, True, None, 0.0, 'both', 2.0, False),
    ('xz_mask_host_both_ghalf', 20, True, 'host', 0.2, 'both', 0.5, False),
    ('xz_mask_ptr_bf16_g03', 3, True, 'ptr', 0.25, 'bf16', 0.3, False),
    ('x_mask_ptr_both_g03', 20, False, 'ptr', 0.2, 'both', 0.3, False),
    ('xz_bf16_g1', 20, True, None, 0.0, 'bf16', 1.0, False),
    ('xz_both_plain', 40, True, None, 0.0, 'both', 1.0, True),
]


@gpu
@VIA
@pytest.mark.parametrize('case', AXPBY, ids=[c[0] for c in AXPBY])
def test_axpby(case, via, margins):
    dev = _gpu()
    name, Cc, has_z, mask, slope, outs, gamma, plain = case
    N, H, W = 2, 5, 7                       # N * K * H * W * 4 threads: 280 K, never a multiple of 256
    K, g = R.planes(Cc), gen(100)
    a, b, slope, gamma = R.f32(0.7), R.f32(-1.3), R.f32(slope), R.f32(gamma)
    # whole 16-channel planes are processed: the reference runs on all 16 K channels
    x, z, m = (torch.randn(N, 16 * K, H, W, generator=g) for _ in range(3))
    m[0, 0, 0, 0], m[0, 1, 0, 0], m[1, 2, 1, 1] = 0.0, -0.0, 0.0    # at +0 and -0 the derivative is `slope`
    xs, zs, ms = (Slab(dev, 'f32', N, K, H, W, R.pack(t), plain) for t in (x, z, m))
    of, ob = Slab(dev, 'f32', N, K, H, W, None, plain), Slab(dev, 'bf16', N, K, H, W, None, plain, lead=2)
    sp = torch.tensor([slope], device=dev)
    kw = dict(x=xs.view(), a=a, N=N, C=Cc, H=H, W=W, gamma=gamma)
    if has_z:
        kw.update(z=zs.view(), b=b)
    if mask:
        kw.update(mask=ms.view(), slope=slope if mask == 'host' else 99.0, slope_ptr=sp.data_ptr() if mask == 'ptr' else None)
    if outs in ('f32', 'both'):
        kw['out_f32'] = of.view()
    if outs in ('bf16', 'both'):
        kw['out_bf16'] = ob.view()
    assert call(via, 'axpby', **kw) == 0
    ref, mag = R.axpby(x, a, z if has_z else None, b, m if mask else None, slope)
    # k: a * x (1), + b * z as product and sum (2; nothing without z), * slope (1 unless slope is a power of two)
    k = 1 + (2 if has_z else 0) + (1 if mask and slope != 0.25 else 0)
    pow2 = gamma in (0.5, 1.0, 2.0)
    if outs == 'f32':
        assert ob.untouched()
    else:
        assert ob.outside_untouched()
    if outs == 'bf16':
        assert of.untouched()
    else:
        assert of.outside_untouched()
        got = of.nchw()
        bounded('axpby %s %s f32' % (name, via), got, ref, k * U32 * mag, margins)
    if outs == 'both':
        prod = got.double() * gamma
        if pow2:   # exact product: the copy is the rounding of the kernel's own f32 result
            assert biteq(ob.nchw(), R.r16(prod, 'bf16'))
        else:      # gamma * v rounded to f32 (1), then to bf16 (u16)
            bounded('axpby %s %s bf16 vs own f32' % (name, via), ob.nchw(), prod, U32 * prod.abs() + R.err16(prod, 'bf16'), margins)
    elif outs == 'bf16':
        f32_term = (k + (0 if pow2 else 1)) * U32 * abs(gamma) * mag
        bounded('axpby %s %s bf16' % (name, via), ob.nchw(), ref * gamma, f32_term + R.err16((ref * gamma).abs() + f32_term, 'bf16'), margins)
    assert xs.untouched() and zs.untouched() and ms.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_downsum2x / dasr_downsum2x_f16
DOWNSUM = [
    # id, C, mask kind, slope, outputs, plain
    ('nomask_f32', 20, None, 0.0, 'f32', False),
    ('mf32_both', 20, 'f32', 0.2, 'both', False),
    ('mbf16_both', 40, 'bf16', 0.2, 'both', False),
    ('mbf16_bf16', 3, 'bf16', 0.25, 'bf16', False),
    ('mf32_f32_plain', 40, 'f32', 0.2, 'f32', True),
]


@gpu
@VIA
@pytest.mark.parametrize('case', DOWNSUM, ids=[c[0] for c in DOWNSUM])
def test_downsum2x(case, via, margins):
    dev = _gpu()
    name, Cc, mk, slope, outs, plain = case
    N, H, W = 2, 5, 7
    K, g, slope = R.planes(Cc), gen(101), R.f32(slope)
    s = torch.randn(N, 16 * K, 2 * H, 2 * W, generator=g)
    m = torch.randn(N, 16 * K, H, W, generator=g)
    m[0, 0, 0, 0], m[0, 1, 0, 0] = 0.0, -0.0
    if mk == 'bf16':
        m = R.r16(m, 'bf16').float()
    ss = Slab(dev, 'f32', N, K, 2 * H, 2 * W, R.pack(s), plain)
    ms = Slab(dev, mk or 'f32', N, K, H, W, R.pack(m, mk or 'f32'), plain, lead=2)
    of, ob = Slab(dev, 'f32', N, K, H, W, None, plain), Slab(dev, 'bf16', N, K, H, W, None, plain, lead=2)
    kw = dict(src=ss.view(), N=N, C=Cc, H=H, W=W, slope=slope)
    if mk:
        kw.update(mask=ms.view(), mask_f32=int(mk == 'f32'))
    if outs != 'bf16':
        kw['dst_f32'] = of.view()
    if outs != 'f32':
        kw['dst_bf16'] = ob.view()
    assert call(via, 'downsum2x', **kw) == 0
    ref, mag = R.downsum2x(s, m if mk else None, slope)
    k = 3 + (1 if mk and slope != 0.25 else 0)    # three additions of the four terms; * slope unless it is a power of two
    assert (of.untouched() if outs == 'bf16' else of.outside_untouched()) and (ob.untouched() if outs == 'f32' else ob.outside_untouched())
    if outs != 'bf16':
        bounded('downsum2x %s %s f32' % (name, via), of.nchw(), ref, k * U32 * mag, margins)
    if outs == 'both':
        assert biteq(ob.nchw(), R.r16(of.nchw(), 'bf16'))          # the copy is the rounding of the kernel's own f32 result
    elif outs == 'bf16':
        bounded('downsum2x %s %s bf16' % (name, via), ob.nchw(), ref, k * U32 * mag + R.err16(ref.abs() + k * U32 * mag, 'bf16'), margins)
    assert ss.untouched() and ms.untouched()


DOWNSUM16 = [
    # id, C, mask, slope, out_scale, outputs, plain
    ('nomask_f32', 20, False, 0.0, 1.0, 'f32', False),
    ('mask_both', 20, True, 0.2, 1.0, 'both', False),
    ('mask_both_s2m10', 40, True, 0.2, 2.0 ** -10, 'both', False),
    ('mask_f16_s2m10', 3, True, 0.25, 2.0 ** -10, 'f16', False),
    ('nomask_both_plain', 40, False, 0.0, 1.0, 'both', True),
]


@gpu
@VIA
@pytest.mark.parametrize('case', DOWNSUM16, ids=[c[0] for c in DOWNSUM16])
def test_downsum2x_f16(case, via, margins):
    dev = _gpu()
    name, Cc, has_m, slope, out_scale, outs, plain = case
    N, H, W = 2, 5, 7
    K, g, slope = R.planes(Cc), gen(102), R.f32(slope)
    s = torch.randn(N, 16 * K, 2 * H, 2 * W, generator=g)
    s[:, :, :2] *= 2.0 ** -16                                       # these rows reach into f16's subnormal range (below 2^-14) already as inputs
    s = R.r16(s, 'f16')
    assert bool(((s.float().abs() < 2.0 ** -14) & (s.float() != 0)).any())
    m = R.r16(torch.randn(N, 16 * K, H, W, generator=g), 'f16')
    m[0, 0, 0, 0], m[0, 1, 0, 0] = 0.0, -0.0
    ss = Slab(dev, 'f16', N, K, 2 * H, 2 * W, R.pack(s, 'f16'), plain)
    ms = Slab(dev, 'f16', N, K, H, W, R.pack(m, 'f16'), plain, lead=2)
    of, oh = Slab(dev, 'f32', N, K, H, W, None, plain), Slab(dev, 'f16', N, K, H, W, None, plain, lead=2)
    kw = dict(src=ss.view(), N=N, C=Cc, H=H, W=W, slope=slope, out_scale=out_scale)
    if has_m:
        kw['mask'] = ms.view()
    if outs != 'f16':
        kw['dst_f32'] = of.view()
    if outs != 'f32':
        kw['dst_f16'] = oh.view()
    assert call(via, 'downsum2x_f16', **kw) == 0
    ref, mag = R.downsum2x(s, m if has_m else None, slope, out_scale)
    k = 3 + (1 if has_m and slope != 0.25 else 0)    # three additions in f32; * slope unless a power of two; out_scale is a power of two: exact
    assert (of.untouched() if outs == 'f16' else of.outside_untouched()) and (oh.untouched() if outs == 'f32' else oh.outside_untouched())
    if outs != 'f16':
        bounded('downsum2x_f16 %s %s f32' % (name, via), of.nchw(), ref, k * U32 * mag, margins)
    if outs == 'both':
        want = R.r16(of.nchw(), 'f16')
        if out_scale != 1.0:
            assert bool(((want.float().abs() < 2.0 ** -14) & (want.float() != 0)).any())   # the f16 results, too, reach the subnormal range
        assert biteq(oh.nchw(), want)                                # the copy is the rounding of the kernel's own f32 result
    elif outs == 'f16':
        bounded('downsum2x_f16 %s %s f16' % (name, via), oh.nchw(), ref, k * U32 * mag + R.err16(ref.abs() + k * U32 * mag, 'f16'), margins)
    assert ss.untouched() and ms.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_pixel_shuffle_f16 / dasr_pixel_unshuffle_f16
def _f16_grid(shape, g):
    """multiples of 2^-6 in [-4, 4]: a quarter of each is exact in f16"""
    return (torch.randint(-256, 257, shape, generator=g).float() * 2.0 ** -6).half()


@gpu
@VIA
@pytest.mark.parametrize('plain', [False, True], ids=['view', 'plain'])
@pytest.mark.parametrize('C4', [64, 192])
def test_pixel_shuffle_unshuffle(C4, plain, via, margins):
    dev = _gpu()
    N, H, W, g = 2, 5, 7, gen(103)
    K4, K = C4 // 16, R.planes(C4 // 4)
    src = R.r16(torch.randn(N, C4, H, W, generator=g), 'f16')
    ss = Slab(dev, 'f16', N, K4, H, W, R.pack(src, 'f16'), plain)
    ds = Slab(dev, 'f16', N, K, 2 * H, 2 * W, None, plain, lead=2)
    assert call(via, 'pixel_shuffle_f16', src=ss.view(), N=N, C4=C4, H=H, W=W, dst=ds.view()) == 0
    # the destination has C4 / 4 channels: with C4 = 64 that is one whole plane, with 192 three; every slot is written
    assert biteq(ds.nchw(), R.pixel_shuffle(src)) and ds.outside_untouched() and ss.untouched()
    # the adjoint without a mask undoes it, bit for bit
    bs = Slab(dev, 'f16', N, K4, H, W, None, plain, lead=3)
    assert call(via, 'pixel_unshuffle_f16', gsrc=ds.view(), N=N, C4=C4, H=H, W=W, gdst=bs.view()) == 0
    assert biteq(bs.nchw(), src) and bs.outside_untouched()
    # with the LeakyReLU' of the activated shuffle input: slope 0.25 on multiples of 2^-6 is exact ...
    gq = _f16_grid((N, C4 // 4, 2 * H, 2 * W), g)
    m = R.r16(torch.randn(N, C4, H, W, generator=g), 'f16')
    m[0, 0, 0, 0], m[0, 1, 0, 0] = 0.0, -0.0
    gs, ms = Slab(dev, 'f16', N, K, 2 * H, 2 * W, R.pack(gq, 'f16'), plain), Slab(dev, 'f16', N, K4, H, W, R.pack(m, 'f16'), plain, lead=2)
    for slope in (0.25, 0.2):
        o = Slab(dev, 'f16', N, K4, H, W, None, plain)
        assert call(via, 'pixel_unshuffle_f16', gsrc=gs.view(), mask=ms.view(), slope=R.f32(slope), N=N, C4=C4, H=H, W=W, gdst=o.view()) == 0
        ref, mag = R.pixel_unshuffle(gq, m, R.f32(slope))
        assert o.outside_untouched() and gs.untouched() and ms.untouched()
        if slope == 0.25:
            assert biteq(o.nchw(), R.r16(ref, 'f16'))
        else:   # ... slope 0.2: the product rounded to f32 (1) and to f16 (u16), or once by a fused conversion
            bounded('pixel_unshuffle C4 %d %s slope 0.2' % (C4, via), o.nchw(), ref, U32 * mag + R.err16(mag, 'f16'), margins)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_maxpool2 / dasr_maxpool2_bwd: is_f32 0 bf16, 1 f32, 2 f16, 3 split f16, 4 split bf16, 5 (backward) split f16 activations + plain f16 gradients
POOL_KIND = {0: 'bf16', 1: 'f32', 2: 'f16', 3: 'f16', 4: 'bf16', 5: 'f16'}
POOL_SIZES = [(2, 2), (3, 3), (6, 10), (7, 11)]


def _pool_input(mode, N, Cp, Hi, Wi, g):
    """multiples of 0.5 in [-1, 1.5] (tied maxima at positive values are common); the split and f32 modes add +-2^-14, which only the lo plane holds:
    many windows are then tied in hi and decided by lo.  Returns (x or hi, lo or None, compared value fp64)"""
    kind = POOL_KIND[mode]
    v = torch.randint(-2, 4, (N, Cp, Hi, Wi), generator=g).float() * 0.5
    if mode in (1, 3, 4, 5):
        v = v + (torch.randint(0, 2, (N, Cp, Hi, Wi), generator=g).float() * 2.0 - 1.0) * 2.0 ** -14
    if mode >= 3:
        hi, lo = R.split16(v, kind)
        assert torch.equal(hi.double() + lo.double(), v.double()) and torch.equal((hi.float() + lo.float()).double(), v.double())
        assert float((lo.float() != 0).double().mean()) > 0.5        # (where the multiple of 0.5 is 0, hi holds the 2^-14 itself)
        return hi, lo, v.double()
    x = v if kind == 'f32' else R.r16(v, kind)
    assert torch.equal(x.double(), v.double())
    return x, None, v.double()


def _assert_ties(val):
    """at least one window in ten has a tied maximum at a positive value"""
    Ho, Wo = val.shape[2] // 2, val.shape[3] // 2
    cand = torch.stack([val[:, :, dy:2 * Ho:2, dx:2 * Wo:2] for dy in (0, 1) for dx in (0, 1)], -1)
    mx = cand.max(-1).values
    tied = ((cand == mx.unsqueeze(-1)).sum(-1) > 1) & (mx > 0)
    assert float(tied.double().mean()) >= 0.1, float(tied.double().mean())


def _pool_slab(dev, kind, N, H, W, hi, lo, plain, lead=1):
    data = R.pack(hi, kind) if lo is None else R.pack_split(hi, lo)
    return Slab(dev, kind, N, data.shape[1], H, W, data, plain, lead)


@gpu
@VIA
@pytest.mark.parametrize('hw', POOL_SIZES, ids=['%dx%d' % s for s in POOL_SIZES])
@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
def test_maxpool2_forward(mode, hw, via):
    dev = _gpu()
    Hi, Wi = hw
    N, Cc, Ho, Wo, g = 2, 20, Hi // 2, Wi // 2, gen(104)
    Cp, kind, plain = 32, POOL_KIND[mode], hw == (6, 10)     # whole planes are pooled: the reference runs on all 32 channels of the two planes
    x, lo, val = _pool_input(mode, N, Cp, Hi, Wi, g)
    _assert_ties(val)
    xs = _pool_slab(dev, kind, N, Hi, Wi, x, lo, plain)
    yh, yl, _ = R.maxpool2(x, lo)
    for Win in [Wi] + ([0] if Wi % 2 == 0 else []):
        ys = Slab(dev, kind, N, xs.K, Ho, Wo, None, plain, lead=2)
        assert call(via, 'maxpool2', x=xs.view(), is_f32=mode, N=N, C=Cc, Ho=Ho, Wo=Wo, y=ys.view(), Win=Win) == 0
        want = R.pack(yh, kind) if lo is None else R.pack_split(yh, yl)
        assert biteq(ys.get(), want), (mode, hw, Win)
        assert ys.outside_untouched() and xs.untouched()


@gpu
@VIA
@pytest.mark.parametrize('hw', POOL_SIZES, ids=['%dx%d' % s for s in POOL_SIZES])
@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4, 5])
def test_maxpool2_backward(mode, hw, via):
    dev = _gpu()
    Hi, Wi = hw
    N, Cc, Ho, Wo, g = 2, 20, Hi // 2, Wi // 2, gen(105)
    Cp, kind, plain = 32, POOL_KIND[mode], hw == (6, 10)
    x, lo, val = _pool_input(mode, N, Cp, Hi, Wi, g)
    _assert_ties(val)
    gy = torch.randn(N, Cp, Ho, Wo, generator=g)
    if mode in (3, 4):
        gh, gl = R.split16(gy, kind)
    else:
        gh, gl = (gy if kind == 'f32' else R.r16(gy, kind)), None
    xs = _pool_slab(dev, kind, N, Hi, Wi, x, lo, plain)
    gs = _pool_slab(dev, kind, N, Ho, Wo, gh, gl, plain, lead=2)
    for relu in (0, 1):
        wh, wl, untouched = R.maxpool2_bwd(x, gh, lo, gl, relu_mask=bool(relu))
        for Win in [Wi] + ([0] if Wi % 2 == 0 else []):
            os_ = Slab(dev, kind, N, gs.K, Hi, Wi, None, plain, lead=3)
            assert call(via, 'maxpool2_bwd', x=xs.view(), gy=gs.view(), is_f32=mode, N=N, C=Cc, Ho=Ho, Wo=Wo, gx=os_.view(), relu_mask=relu, Win=Win) == 0
            got = os_.get()
            want = R.pack(wh, kind) if wl is None else R.pack_split(wh, wl)
            inside = ~untouched
            assert biteq(got[:, :, inside], want[:, :, inside]), (mode, hw, relu, Win)
            # the row / column an odd size leaves outside every window is not written (the trainers rely on zero at allocation there)
            assert biteq(got[:, :, untouched], sent_like(got[:, :, untouched])), (mode, hw, relu, Win)
            assert os_.outside_untouched() and xs.untouched() and gs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_affine4: y_f32 0 bf16, 1 f32, 2 f16, 3 split f16 (hi plane 0, remainder plane 1; no accumulate)
AFF_KIND = {0: 'bf16', 1: 'f32', 2: 'f16', 3: 'f16'}


# (y_f32, accumulate): the split form does not accumulate (DASR_EINVAL: test_argument_checks)
AFF_MODES = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0)]


@gpu
@VIA
@pytest.mark.parametrize('Cc', [1, 3, 4])
@pytest.mark.parametrize('y_f32,acc', AFF_MODES)
def test_affine4(y_f32, acc, Cc, via, margins):
    dev = _gpu()
    N, H, W, g = 2, 5, 7, gen(106)
    kind, plain = AFF_KIND[y_f32], Cc == 4
    scale, shift = [1.7, -0.3, 2.5, 0.9], [0.4, -1.1, 0.05, 3.0]
    x = torch.randn(N, Cc, H, W, generator=g)
    xs = Slab(dev, 'f32', N, 1, H, W, R.pack(x, 'f32', pad=SENT), plain)      # channels >= C of x hold the sentinel: computed on, then dropped
    Ky = 2 if y_f32 == 3 else 1
    y0 = torch.randn(N, Cc, H, W, generator=g)
    y0 = y0 if kind == 'f32' else R.r16(y0, kind).float()
    ys = Slab(dev, kind, N, Ky, H, W, R.pack(y0, kind, pad=SENT) if acc else None, plain, lead=2)
    before = ys.get()
    assert call(via, 'affine4', x=xs.view(), N=N, C=Cc, H=H, W=W, scale4=scale, shift4=shift, y=ys.view(), y_f32=y_f32, accumulate=acc) == 0
    assert ys.outside_untouched() and xs.untouched()
    ref, mag = R.affine4(x, scale, shift, y0 if acc else None)
    got = ys.get()
    k = 2 + acc                                      # x * scale (1), + shift (1), + y (1)
    f32_term = k * U32 * mag
    if y_f32 == 3:
        hi, lo = R.unpack(got[:, :1]), R.unpack(got[:, 1:])
        bounded('affine4 split hi C%d %s' % (Cc, via), hi[:, :Cc], ref, f32_term + R.err16(ref.abs() + f32_term, 'f16'), margins)
        # lo = round16(v - hi) of the kernel's f32 value v: hi + lo misses v by the rounding of the remainder alone
        rem = lo[:, :Cc].double().abs()
        bounded('affine4 split hi+lo C%d %s' % (Cc, via), hi[:, :Cc].double() + lo[:, :Cc].double(), ref, f32_term + R.err16(rem, 'f16'), margins)
        assert biteq(hi[:, Cc:], torch.zeros_like(hi[:, Cc:])) and biteq(lo[:, Cc:], torch.zeros_like(lo[:, Cc:]))   # channels >= C: zero, both planes
    else:
        y = R.unpack(got)
        bound = f32_term if kind == 'f32' else f32_term + R.err16(ref.abs() + f32_term, kind)
        bounded('affine4 y_f32 %d C%d acc %d %s' % (y_f32, Cc, acc, via), y[:, :Cc], ref, bound, margins)
        if acc:    # accumulate: channels >= C are left as they were
            assert biteq(y[:, Cc:], R.unpack(before)[:, Cc:])
        else:      # channels >= C of the plane: zero
            assert biteq(y[:, Cc:], torch.zeros_like(y[:, Cc:]))


@gpu
@VIA
def test_affine4_split_planes_are_exact_for_power_of_two_scales(via):
    """scale a power of two, shift 0: v = x * scale is exact, so hi = round16(v) and lo = round16(v - hi) bit for bit"""
    dev = _gpu()
    N, Cc, H, W = 2, 3, 5, 7
    x = torch.randn(N, Cc, H, W, generator=gen(107))
    scale = [2.0, 0.5, 4.0, 1.0]
    xs, ys = Slab(dev, 'f32', N, 1, H, W, R.pack(x, 'f32', pad=SENT)), Slab(dev, 'f16', N, 2, H, W)
    assert call(via, 'affine4', x=xs.view(), N=N, C=Cc, H=H, W=W, scale4=scale, shift4=[0.0] * 4, y=ys.view(), y_f32=3, accumulate=0) == 0
    v = x * torch.tensor(scale[:Cc]).view(1, Cc, 1, 1)
    hi, lo = R.split16(v, 'f16')
    assert bool((lo.float() != 0).any())
    got = ys.get()
    assert biteq(R.unpack(got[:, :1], Cc), hi) and biteq(R.unpack(got[:, 1:], Cc), lo) and ys.outside_untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_l1_diff: is_f32 bit 0 f32 / bf16 tensors, bit 1 squared
def _grid_chain(nblocks):
    """roundings behind the accumulator once a workgroup has its thread sums: wave butterfly (6), four waves (3), grid_sum_commit's per-thread
    loop over ceil(nblocks / 256) partials, butterfly (6), (a + b) + (c + d) (2), * coef (1), the add into the accumulator (1)"""
    return 6 + 3 + (nblocks + 255) // 256 + 6 + 2 + 1 + 1


@gpu
@VIA
@pytest.mark.parametrize('Cc', [20, 40])
@pytest.mark.parametrize('is_f32', [0, 1, 2, 3])
def test_l1_diff(is_f32, Cc, via, margins):
    dev = _gpu()
    N, H, W, g = 2, 5, 7, gen(108)
    kind, squared, K = ('f32' if is_f32 & 1 else 'bf16'), bool(is_f32 & 2), R.planes(Cc)
    a, b = torch.randn(N, Cc, H, W, generator=g), torch.randn(N, Cc, H, W, generator=g)
    b[:, ::3, 1, 2] = a[:, ::3, 1, 2]                              # a == b: the sign gradient there is exactly 0
    if kind == 'bf16':
        a, b = R.r16(a, kind).float(), R.r16(b, kind).float()
    # the padding channels of a and b hold (different) garbage: masked out of the sum, zero gradient
    as_, bs = Slab(dev, kind, N, K, H, W, R.pack(a, kind, pad=SENT)), Slab(dev, kind, N, K, H, W, R.pack(b, kind, pad=77.0), lead=2)
    coef, gcoef, acc0 = R.f32(1.0 / a.numel()), R.f32(2.0 / a.numel()), 0.25
    loss, lmag, ga, gmag = R.l1_diff(a, b, coef, gcoef, squared)
    nblocks = (N * K * H * W * 4 + 255) // 256
    # L: a - b (1), squared: its product (1), four terms per thread (4), then the grid chain
    Lc = 1 + int(squared) + 4 + _grid_chain(nblocks)
    for with_ga in (True, False):
        acc = torch.full((4,), acc0, device=dev)
        gs = Slab(dev, kind, N, K, H, W, None, plain=not with_ga, lead=3)
        kw = dict(a=as_.view(), b=bs.view(), is_f32=is_f32, N=N, C=Cc, H=H, W=W, coef=coef, gcoef=gcoef, loss_acc=acc.data_ptr())
        if with_ga:
            kw['ga'] = gs.view()
        assert call(via, 'l1_diff', **kw) == 0
        assert as_.untouched() and bs.untouched()
        accc = acc.cpu()
        assert bool((accc[1:] == acc0).all())
        err, bound = abs(float(accc[0].double()) - (acc0 + loss)), Lc * U32 * (lmag + acc0)
        if not squared:
            bound = min(bound, 1e-6)                               # (no looser than the absolute 1e-6 of test_bce_dwt_lowpass_pool_misc on a loss of O(1))
        margins('elementwise l1_diff is_f32 %d C%d %s loss: |err| / bound %.3f (L %d)' % (is_f32, Cc, via, err / bound, Lc))
        assert err <= bound, (err, bound)
        if not with_ga:
            assert gs.untouched()
            continue
        assert gs.outside_untouched()
        got = gs.nchw()
        assert biteq(got[:, Cc:], torch.zeros_like(got[:, Cc:]))   # zero gradient in the padding channels
        if not squared:    # gcoef * (+-1 | 0): exact
            want = ga.float() if kind == 'f32' else R.r16(ga, kind)
            assert biteq(got[:, :Cc], want) and bool((got[:, :Cc][:, ::3, 1, 2].float() == 0).all())
        else:              # a - b (1), (2 gcoef) * d (1); bf16: + one 16-bit rounding
            f32_term = 2 * U32 * gmag
            bounded('l1_diff is_f32 %d C%d %s ga' % (is_f32, Cc, via), got[:, :Cc], ga, f32_term if kind == 'f32' else f32_term + R.err16(gmag + f32_term, kind),
                    margins)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_l1_loss: accumulate bit 0 grad +=, bit 1 squared error, bit 2 f16 gradient
@gpu
@VIA
@pytest.mark.parametrize('Cc', [1, 3])
@pytest.mark.parametrize('bits', [0, 1, 2, 3])
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'wm'])
def test_l1_loss(weighted, bits, Cc, via, margins):
    dev = _gpu()
    N, H, W, g = 2, 9, 15, gen(109)                                # N * H * W = 270 threads: a second, partial workgroup
    squared, accum = bool(bits & 2), bool(bits & 1)
    sr, hr = torch.rand(N, Cc, H, W, generator=g), torch.rand(N, Cc, H, W, generator=g)
    hr[:, 0, 2, 3] = sr[:, 0, 2, 3]                                # sr == hr: the sign gradient there is exactly 0
    wm = torch.rand(N, 1, H, W, generator=g) if weighted else None
    g0 = torch.randn(N, 16, H, W, generator=g)
    ss = Slab(dev, 'f32', N, 1, H, W, R.pack(sr, 'f32', pad=SENT))   # channels >= C of sr hold the sentinel: never read
    gs = Slab(dev, 'f32', N, 1, H, W, R.pack(g0) if accum else None, lead=2)
    hrd, wmd = hr.to(dev), (wm.to(dev) if weighted else None)
    coef, acc0 = R.f32(1.0 / sr.numel()), 0.5
    acc = torch.full((4,), acc0, device=dev)
    assert call(via, 'l1_loss', sr=ss.view(), hr_nchw=hrd.data_ptr(), weight_map=wmd.data_ptr() if weighted else None, N=N, C=Cc, H=H, W=W, coef=coef,
                loss_acc=acc.data_ptr(), grad=gs.view(), accumulate=bits) == 0
    assert ss.untouched() and gs.outside_untouched()
    loss, lmag, gr, gmag = R.l1_loss(sr, hr, coef, wm, squared)
    # L: sr - hr (1), wm * |d| (1) or wm * d * d (2), C terms per thread (C), then the grid chain
    Lc = 1 + (2 if squared else 1) + Cc + _grid_chain((N * H * W + 255) // 256)
    accc = acc.cpu()
    err, bound = abs(float(accc[0].double()) - (acc0 + loss)), Lc * U32 * (lmag + acc0)
    if not squared:
        bound = min(bound, 1e-6)                                   # (no looser than the absolute 1e-6 of test_elementwise_and_adam)
    margins('elementwise l1_loss bits %d C%d wm %d %s loss: |err| / bound %.3f (L %d)' % (bits, Cc, weighted, via, err / bound, Lc))
    assert err <= bound and bool((accc[1:] == acc0).all()), (err, bound)
    got = gs.nchw()
    if accum:
        assert biteq(got[:, Cc:], g0[:, Cc:])                      # += 0: channels >= C keep what they held
        ref, mag = gr + g0[:, :Cc].double(), gmag + g0[:, :Cc].double().abs()
    else:
        assert biteq(got[:, Cc:], torch.zeros_like(got[:, Cc:]))   # zero beyond C, all 16 channels of the plane
        ref, mag = gr, gmag
    # k: sign form: coef * wm (1; exact without a map); squared: sr - hr (1), (2 coef) * wm (1), * d (1); accumulate: the add (1)
    k = (3 if squared else int(weighted)) + int(accum)
    if k == 0:
        assert biteq(got[:, :Cc], gr.float()) and bool((got[:, 0, 2, 3] == 0).all())
    else:
        bounded('l1_loss bits %d C%d wm %d %s grad' % (bits, Cc, weighted, via), got[:, :Cc], ref, k * U32 * mag, margins)


@gpu
@VIA
def test_l1_loss_optional_outputs_and_f16_gradient(via, margins):
    dev = _gpu()
    N, Cc, H, W, g = 2, 1, 9, 15, gen(110)
    sr, hr = torch.rand(N, Cc, H, W, generator=g), torch.rand(N, Cc, H, W, generator=g)
    ss, hrd = Slab(dev, 'f32', N, 1, H, W, R.pack(sr, 'f32', pad=SENT)), hr.to(dev)
    coef = R.f32(1.0 / sr.numel())
    loss, lmag, gr, _ = R.l1_loss(sr, hr, coef)
    kw = dict(sr=ss.view(), hr_nchw=hrd.data_ptr(), N=N, C=Cc, H=H, W=W, coef=coef)
    # gradient without a loss accumulator
    gs = Slab(dev, 'f32', N, 1, H, W, lead=2)
    assert call(via, 'l1_loss', grad=gs.view(), **kw) == 0
    assert biteq(gs.nchw(Cc), gr.float()) and gs.outside_untouched()
    # loss without a gradient
    acc = torch.zeros(4, device=dev)
    assert call(via, 'l1_loss', loss_acc=acc.data_ptr(), **kw) == 0
    Lc = 1 + 1 + Cc + _grid_chain(2) - 1                           # (the add into a zero accumulator is exact)
    err, bound = abs(float(acc[0].double()) - loss), min(Lc * U32 * lmag, 1e-6)
    margins('elementwise l1_loss loss only %s: |err| / bound %.3f (L %d)' % (via, err / bound, Lc))
    assert err <= bound
    # bit 2: f16 gradient, pre-scaled by a power of two; C = 1: only the first 4-channel group is written, the rest keeps the sentinel
    for bits in (4, 6):
        g16 = Slab(dev, 'f16', N, 1, H, W, lead=2)
        assert call(via, 'l1_loss', grad=g16.view(), accumulate=bits, grad_scale=1024.0, **kw) == 0
        got = g16.nchw()
        _, _, gr2, gmag2 = R.l1_loss(sr, hr, coef, None, bool(bits & 2))
        if bits == 4:      # coef * 1024 * sign: exact in f32, one f16 rounding
            assert biteq(got[:, :1], R.r16(gr2 * 1024.0, 'f16'))
        else:              # sr - hr (1), (2 coef) * d (1), * 1024 (exact), one f16 rounding
            f32_term = 2 * U32 * gmag2 * 1024.0
            bounded('l1_loss f16 squared %s grad' % via, got[:, :1], gr2 * 1024.0, f32_term + R.err16(gmag2 * 1024.0 + f32_term, 'f16'), margins)
        assert biteq(got[:, 1:4], torch.zeros_like(got[:, 1:4])) and biteq(got[:, 4:], sent_like(got[:, 4:])) and g16.outside_untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_sigmoid_fwd
@gpu
@VIA
@pytest.mark.parametrize('Cc', [1, 2, 3, 4])
def test_sigmoid_fwd(Cc, via, margins):
    dev = _gpu()
    N, H, W, g = 2, 9, 15, gen(111)
    x = torch.cat([torch.linspace(-30.0, 30.0, Cc * H * W).view(1, Cc, H, W), torch.randn(1, Cc, H, W, generator=g) * 4.0])
    xs, ys = Slab(dev, 'f32', N, 1, H, W, R.pack(x, 'f32', pad=SENT), plain=Cc == 4), Slab(dev, 'f32', N, 1, H, W, None, plain=Cc == 4, lead=2)
    assert call(via, 'sigmoid_fwd', x=xs.view(), N=N, C=Cc, H=H, W=W, y=ys.view()) == 0
    ref, mag = R.sigmoid(x)
    got = ys.nchw()
    # k = 4: expf is accurate to 1 ulp = 2 u (the device math library's documented bound; the relative error of y from e = exp(-x) is e / (1 + e) times
    # that of e, at most the same), 1 + e (1), the correctly rounded division (1)
    bounded('sigmoid_fwd C%d %s' % (Cc, via), got[:, :Cc], ref, 4 * U32 * mag, margins)
    assert biteq(got[:, Cc:], torch.zeros_like(got[:, Cc:])) and ys.outside_untouched() and xs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_fill_f32 / dasr_add_flat
BIG = 4096 * 256 + 777      # the launch has at most 4096 workgroups of 256: the grid-stride loop takes a second pass


@gpu
@VIA
@pytest.mark.parametrize('n', [1, 255, BIG])
def test_fill_and_add_flat(n, via):
    dev = _gpu()
    G, g = 64, gen(112)
    buf = torch.full((G + n + G,), SENT, device=dev)
    assert call(via, 'fill_f32', p=buf.data_ptr() + 4 * G, n=n, value=R.f32(0.3)) == 0
    want = torch.full((G + n + G,), SENT)
    want[G:G + n] = R.f32(0.3)
    assert biteq(buf, want)                                        # the guard words in front of and behind the buffer keep the sentinel
    y, x = torch.randn(n, generator=g), torch.randn(n, generator=g)
    buf[G:G + n] = y.to(dev)
    xd = x.to(dev)
    assert call(via, 'add_flat', y=buf.data_ptr() + 4 * G, x=xd.data_ptr(), n=n) == 0
    want[G:G + n] = R.add_flat(y, x)[0].float()                    # one rounding of the exact sum
    assert biteq(buf, want) and biteq(xd, x)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dasr_adam
LR, B1, B2, EPS = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8)


def _adam(p, g, m, v, n, step, wd=0.0, nonfinite=None, gate=None):
    from dasr_amd import _lib
    from dasr_amd.engine import _stream
    rc = _lib.lib().dasr_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS, wd, step,
                              nonfinite.data_ptr() if nonfinite is not None else None, gate.data_ptr() if gate is not None else None, _stream())
    torch.cuda.synchronize()
    return rc


@gpu
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('n', [1000, BIG])
def test_adam_three_steps(n, wd, margins):
    dev = _gpu()
    g, wd = gen(113), R.f32(wd)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    G = 64
    bufs = [torch.full((G + n + G,), SENT, device=dev) for _ in range(3)]
    pd, md, vd = (b[G:G + n] for b in bufs)
    pd.copy_(p0.to(dev))
    md.zero_()
    vd.zero_()
    for i, gg in enumerate(grads):
        assert _adam(pd, gg.to(dev), md, vd, n, i + 1, wd) == 0
    p, m, v, Ep, Em, Ev = R.adam(p0, grads, LR, B1, B2, EPS, wd)
    # running first-order bounds of the reference (one rounding per operation of the update, constants included), see blocked_ref.adam
    bounded('adam n %d wd %g m' % (n, wd), md.cpu(), m, U32 * Em, margins)
    bounded('adam n %d wd %g v' % (n, wd), vd.cpu(), v, U32 * Ev, margins)
    bound = torch.minimum(U32 * Ep, 1e-7 + 1e-5 * p.abs())         # (no looser than rtol 1e-5 / atol 1e-7 of test_elementwise_and_adam)
    bounded('adam n %d wd %g p' % (n, wd), pd.cpu(), p, bound, margins)
    for b in bufs:
        bc = b.cpu()
        assert bool((bc[:G] == SENT).all()) and bool((bc[G + n:] == SENT).all())


def _adam_state(dev, n, seed):
    g = gen(seed)
    return [torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev), (torch.randn(n, generator=g) * 0.1).to(dev),
            (torch.rand(n, generator=g) * 0.01).to(dev)]


@gpu
def test_adam_gate_word_keeps_the_step_from_the_weights():
    dev = _gpu()
    n = BIG
    p, g, m, v = _adam_state(dev, n, 114)
    g[5] = float('inf')                                            # a gated launch does not even report: it changes nothing at all
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    gate, flag = torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    assert _adam(p, g, m, v, n, 3, 0.01, flag, gate) == 0
    assert biteq(p, p0) and biteq(m, m0) and biteq(v, v0) and int(flag) == 0
    gate.fill_(-7)                                                 # any non-zero value closes it
    assert _adam(p, g, m, v, n, 3, 0.01, flag, gate) == 0
    assert biteq(p, p0) and biteq(m, m0) and biteq(v, v0) and int(flag) == 0
    gate.zero_()
    assert _adam(p, g, m, v, n, 3, 0.01, flag, gate) == 0
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    assert _adam(pr, g, mr, vr, n, 3, 0.01, None, None) == 0       # the same call without a gate word
    assert int(flag) == 1 and not biteq(m, m0) and biteq(p, pr) and biteq(m, mr) and biteq(v, vr)
    assert int((p != p0).sum()) > n // 2


NONFINITE_AT = [('first_wave', BIG, 5), ('tail_last_partial_wave', BIG, BIG - 3), ('second_pass', BIG, 4096 * 256 + 70), ('small_last_partial_wave', 1000, 999)]


@gpu
@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')], ids=['inf', 'neg_inf', 'nan'])
@pytest.mark.parametrize('where', NONFINITE_AT, ids=[w[0] for w in NONFINITE_AT])
def test_adam_nonfinite_flag(where, bad):
    dev = _gpu()
    _, n, idx = where
    p, g, m, v = _adam_state(dev, n, 115)
    clean = [t.clone() for t in (p, m, v)]
    flag0 = torch.zeros(1, dtype=torch.int32, device=dev)
    assert _adam(clean[0], g, clean[1], clean[2], n, 2, 0.0, flag0, None) == 0 and int(flag0) == 0     # finite gradients: the nonfinite word stays 0
    for preset in (0, 2):
        pp, mm, vv, gg = p.clone(), m.clone(), v.clone(), g.clone()
        gg[idx] = bad
        flag = torch.full((1,), preset, dtype=torch.int32, device=dev)
        assert _adam(pp, gg, mm, vv, n, 2, 0.0, flag, None) == 0
        assert int(flag) == (preset | 1)                           # bit 0 is OR-ed in, the other bits stay
        keep = torch.ones(n, dtype=torch.bool)
        keep[idx] = False
        for got, want in zip((pp, mm, vv), clean):                 # every other element: exactly the step without it
            assert biteq(got.cpu()[keep], want.cpu()[keep])
        assert not bool(torch.isfinite(mm[idx]))                   # the update itself is what torch would do: the moment absorbs it


@gpu
def test_adam_large_finite_gradients_do_not_set_the_flag():
    dev = _gpu()
    n = BIG
    p, g, m, v = _adam_state(dev, n, 116)
    for i, val in ((5, 1e38), (BIG - 3, -1e38), (4096 * 256 + 70, 1e38), (1234, 1e-38)):
        g[i] = val
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    assert _adam(p, g, m, v, n, 1, 0.0, flag, None) == 0
    assert int(flag) == 0


@gpu
def test_adamhip_check_finite_raises_once_and_clears_the_nonfinite_word(monkeypatch):
    dev = _gpu()
    from dasr_amd.engine import ParamStore
    from dasr_amd.models import AdamHIP
    monkeypatch.delenv('DASR_ALLOW_NONFINITE', raising=False)
    P = ParamStore([('w', (1000,)), ('b', (24,))], dev)
    P.flat.normal_()
    opt = AdamHIP(P, 1e-3)
    P.grad.normal_()
    opt.step(1e-3)
    torch.cuda.synchronize()
    opt.check_finite()                                             # finite gradients: nothing to report
    P.grad[1001] = float('inf')
    opt.step(1e-3)
    torch.cuda.synchronize()
    assert int(opt.nonfinite) == 1
    with pytest.raises(FloatingPointError, match='non-finite now in b'):
        opt.check_finite()
    assert int(opt.nonfinite) == 0
    opt.check_finite()                                             # raised once: the word was cleared
    monkeypatch.setenv('DASR_ALLOW_NONFINITE', '1')
    opt.step(1e-3)
    torch.cuda.synchronize()
    assert int(opt.nonfinite) == 1
    opt.check_finite()                                             # cleared, not raised
    assert int(opt.nonfinite) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@VIA
def test_argument_checks(via):
    """each returns DASR_EINVAL and leaves a sentinel-filled output untouched"""
    dev = _gpu()
    N, H, W = 2, 5, 7
    # C4 not a multiple of 64
    s16, d16 = Slab(dev, 'f16', N, 2, H, W), Slab(dev, 'f16', N, 1, 2 * H, 2 * W)
    assert call(via, 'pixel_shuffle_f16', src=s16.view(), N=N, C4=32, H=H, W=W, dst=d16.view()) == EINVAL and d16.untouched()
    assert call(via, 'pixel_unshuffle_f16', gsrc=d16.view(), N=N, C4=96, H=H, W=W, gdst=s16.view()) == EINVAL and s16.untouched()
    # affine4: C = 5; split output together with accumulate
    xs, ys = Slab(dev, 'f32', N, 1, H, W), Slab(dev, 'f16', N, 2, H, W)
    one, zero = [1.0] * 4, [0.0] * 4
    assert call(via, 'affine4', x=xs.view(), N=N, C=5, H=H, W=W, scale4=one, shift4=zero, y=ys.view(), y_f32=2, accumulate=0) == EINVAL and ys.untouched()
    assert call(via, 'affine4', x=xs.view(), N=N, C=3, H=H, W=W, scale4=one, shift4=zero, y=ys.view(), y_f32=3, accumulate=1) == EINVAL and ys.untouched()
    # l1_loss: f16 gradient together with accumulate; C = 17
    hr, acc = torch.zeros(N, 17, H, W, device=dev), torch.full((4,), SENT, device=dev)
    sr, gr = Slab(dev, 'f32', N, 2, H, W), Slab(dev, 'f32', N, 2, H, W)
    kw = dict(sr=sr.view(), hr_nchw=hr.data_ptr(), N=N, H=H, W=W, coef=1.0, loss_acc=acc.data_ptr(), grad=gr.view())
    assert call(via, 'l1_loss', C=3, accumulate=5, grad_scale=1.0, **kw) == EINVAL and gr.untouched()
    assert call(via, 'l1_loss', C=17, accumulate=0, **kw) == EINVAL and gr.untouched()
    assert bool((acc.cpu() == SENT).all())
    # max-pool: an input width that is neither 2 Wo nor 2 Wo + 1
    xp, yp, gp = Slab(dev, 'f32', N, 1, 6, 12), Slab(dev, 'f32', N, 1, 3, 5), Slab(dev, 'f32', N, 1, 6, 12)
    assert call(via, 'maxpool2', x=xp.view(), is_f32=1, N=N, C=16, Ho=3, Wo=5, y=yp.view(), Win=12) == EINVAL and yp.untouched()
    assert call(via, 'maxpool2_bwd', x=xp.view(), gy=yp.view(), is_f32=1, N=N, C=16, Ho=3, Wo=5, gx=gp.view(), relu_mask=0, Win=12) == EINVAL
    assert gp.untouched()
    # n = 0
    buf = torch.full((64,), SENT, device=dev)
    assert call(via, 'fill_f32', p=buf.data_ptr(), n=0, value=1.0) == EINVAL
    assert call(via, 'add_flat', y=buf.data_ptr(), x=buf.data_ptr(), n=0) == EINVAL
    if via == 'abi':   # dasr_adam has no op kind
        m, v, g = (torch.full((64,), SENT, device=dev) for _ in range(3))
        assert _adam(buf, g, m, v, 0, 1) == EINVAL and _adam(buf, g, m, v, 64, 0) == EINVAL
        assert bool((m.cpu() == SENT).all()) and bool((v.cpu() == SENT).all())
    assert bool((buf.cpu() == SENT).all())
