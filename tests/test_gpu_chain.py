"""GPU tests of the chained trunk launches at kernel level: dasr_conv_chain (csrc/conv.hip, conv_chain_kernel: the layer form) and dasr_rdb_chain
(csrc/rdb_is.h, rdb_is_kernel: the input-stationary form), built directly from engine.conv_op / engine.ConvChain and run through the C ABI (via = abi)
and as OP_CONV_CHAIN / OP_RDB_CHAIN of an OpList (via = op) -- no model in between.  nf 64, gc 32, one to three dense blocks of random weights.

Set-up of every case: the dense slabs, the LeakyReLU' mask slabs of a data-gradient chain and the fp32 streams are planes [1, 1 + K) of images
[1, 1 + N) (or the range the case names) of parents whose other planes and images hold NaN; the masks of a data-gradient chain are laid out as
planes x1 .. x4 of a forward slab but hold random values of their own with +0 and -0 planted (deliberately not the planes a forward chain left: both
signs at every position of every layer, and the two zeros, which a forward activation almost never holds); the planes a chain writes hold NaN as well until it writes
them (a layer that reads a plane before its producer has stored it comes out non-finite); the fp32 outputs and the 16-bit planes of the last conv5 are
views of sentinel-filled parents.  Afterwards everything but the planes the chain must write comes back bit for bit, the flag words behind the tiles of
the height that ran (the buffer is sized for 4-row tiles) and the guard words around the flag buffer included, and the device error word is 0.

What is asserted:
  bit-identity   the same parameter blocks run one dasr_conv after the other on a second copy of all buffers: every 16-bit plane and every fp32 stream
                 equal bit for bit (the header's contract: "Layer L is dasr_conv(layers[L]) -- same arithmetic, bit-identical results").
  fp64           every layer per element against the fp64 model of oracle/conv_ref.py, evaluated on the slab the chain left behind (conv k of a block
                 reads planes [0, 4 + 2k) of its slab, which nothing overwrites later; the next block's x planes are this block's 16-bit conv5 output),
                 so every layer is held to its actual 16-bit inputs.  Bound of tests/test_gpu_conv.py, unchanged: c(L) 2^-23 S gain + k 2^-24 terms, plus
                 half a 16-bit ulp on 16-bit planes.  Small shapes run oracle.conv_ref.conv_detail itself (CPU); larger ones the same expressions as
                 fp64 matrix products on the device (_detail_dev), which test_fp64_model_on_the_device_is_conv_ref holds to conv_detail.
  what ran       input-stationary form: the tile height from the launch's tag in a profiling session, q from the ticket words (they advance by q per
                 launch), both equal to RRDBNetHIP.is_launch and to the table below; tile words + 5 per dense block / + nlayers, tickets + q / + 64.

Epilogues: two blocks = conv1 waits for its neighbours' conv5; three blocks with `rrdb` = the RRDB's second fp32 residual on the third conv5 (249 / 248,
without 16-bit planes 185 / 184); `last16` = the last conv5 writes 16-bit planes (233 / 232) or not (169 / 168, input-stationary form only).

Input-stationary form, test_is_geometry[<dir>-<id>] (fwd = rdb_is_kernel<false, false, NT, NW>, bwd = <false, true, NT, NW>; 16 rows = <2, 8>, 8 rows = <1, 8>,
4 rows = <1, 4>).  last tile = last tile row / last tile column, full or partial; fwd / bwd = dense blocks x epilogue of the last conv5 (the blocks before it:
233 / 232); * = also held to fp64.  The launcher's rule sees h and w only through ceil(h / rows) and ceil(w / 32), so every geometry has shapes with full and
with partial last tiles: EVERY cell of tile height x tiles per workgroup (1, 2, more than 4) x last row x last column has a shape (asserted at import, as is
that every conv5 epilogue runs at every tile height in both directions); no cell is left out.
    id          rows    q  tiles/wg  last tile    fwd       bwd         notes
    8x4x32        4    1   1       full / full  2 x 233   2 x 168   * one tile per image (every neighbour word is the tile's own)
    8x4x36        4    2   1       full / part  3 x 185   3 x 248   *
    8x6x64        4    4   1       part / full  2 x 169   1 x 232   *
    8x6x36        4    4   1       part / part  3 x 249   2 x 232   *
    8x6x8         4    2   1       part / part  1 x 233   3 x 184   * narrower than a tile
    48x4x192      4   18   2       full / full  2 x 233   2 x 168   *
    48x4x164      4   18   2       full / part  3 x 185   3 x 248   *
    48x3x192      4   18   2       part / full  2 x 169   1 x 232   *
    48x3x164      4   18   2       part / part  3 x 249   2 x 232   *
    40x8x224      4   14   5       full / full  1 x 233   3 x 184
    40x8x196      4   14   5       full / part  2 x 233   2 x 168
    40x6x224      4   14   5       part / full  3 x 185   3 x 248   *
    40x6x196      4   14   5       part / part  2 x 169   1 x 232   *
    8x136x32      8   17   1       full / full  3 x 249   2 x 232   * prime q
    8x72x36       8   18   1       full / part  1 x 233   3 x 184   *
    48x10x64      8   24   1       part / full  2 x 233   2 x 168   *
    48x10x36      8   24   1       part / part  3 x 185   3 x 248   *
    8x144x8       8   18   1       full / part  2 x 169   1 x 232   * narrower than a tile
    48x24x96      8   27   2       full / full  3 x 249   2 x 232     odd q
    48x24x68      8   27   2       full / part  1 x 233   3 x 184
    48x18x96      8   27   2       part / full  2 x 233   2 x 168
    48x18x68      8   27   2       part / part  3 x 185   3 x 248   * odd q
    24x82x36      8   22   3       part / part  2 x 169   1 x 232
    40x136x32     8   17   5       full / full  2 x 233   2 x 168
    40x136x8      8   17   5       full / part  1 x 233   3 x 184   *
    40x129x32     8   17   5       part / full  2 x 233   2 x 168
    40x129x8      8   17   5       part / part  3 x 185   3 x 248   *
    64x34x164     8   30   8       part / part  2 x 233   2 x 168     MAX_TPW tiles per workgroup
    8x48x192     16   18   1       full / full  3 x 249   2 x 232
    8x144x36     16   18   1       full / part  1 x 233   3 x 184   *
    48x18x64     16   24   1       part / full  2 x 233   2 x 168   *
    48x18x36     16   24   1       part / part  3 x 185   3 x 248   *
    128x32x8     16   32   1       full / part  2 x 169   1 x 232   * narrower than a tile, q 32
    48x48x64     16   18   2       full / full  3 x 249   2 x 232
    48x48x36     16   18   2       full / part  1 x 233   3 x 184
    48x42x64     16   18   2       part / full  2 x 233   2 x 168
    48x42x36     16   18   2       part / part  3 x 185   3 x 248
    24x130x36    16   18   3       part / part  2 x 169   1 x 232
    40x144x64    16   18   5       full / full  2 x 169   2 x 232
    40x144x36    16   18   5       full / part  2 x 233   2 x 168
    40x130x64    16   18   5       part / full  2 x 169   2 x 232
    64x130x36    16   18   8       part / part  2 x 233   2 x 168     MAX_TPW tiles per workgroup
Layer form, test_layer_geometry[<prec>-<dir>-<id>] (conv_chain_kernel<F16, BWD>: bf16 / f16 x fwd / bwd), 512 tiles of 16 x 32 each:
    32x50x100, 16x120x120, 64x20x100   partial tiles both ways (* 64x20x100)       512x16x32   single full tile per image
    512x10x20   single partial tile *                                               8x128x256   8 x 8 full tiles: interior tiles with all eight neighbours
    16of32x128x128   images [16, 32) of a parent of 32: the sub-batch form of RRDBNetHIP.chain_split (rrdbnet._sub_batch_conv)
  test_layer_dep_chunk_every_chunk: dep_chunk as the plan builds it against <= 0 ("every chunk"), same bits.
test_flags_count_on_and_wrap: three launches on one flag buffer, then all tile words preset to 0x7ffffff0 / 0xfffffff0 (two launches each: with two dense
  blocks the words cross 2^31 / 2^32 inside the second) -- identical bits, counts as above.  The give-up path (error bit 1) is not provoked.
DASR_EINVAL (both via modes; outputs, flags, tickets, error word untouched):
  test_refused_arguments[<form>-<clause>]: null_dev_layers, null_host_layers, null_dev_dep_chunk (layer), null_dev_flags, null_dev_err, nlayers_0, nlayers_neg,
  nlayers_7 (is: not a multiple of 5);
  test_refusals[<form>-<dir>-<clause>], one field of one layer of a valid chain changed: kh_4, stride_2, pad_0, in_f32, mixed_prec, f16 (is), other_geometry_H / _W,
  other_N, cin_80_on_conv2 (is), cin_not_16 (layer), mt_2_on_conv2, mt_1_on_conv5 (is), mt_3 (layer), cout_64_on_conv3, w_null, two_slabs / slab_strides (is),
  slope_ptr, mask_f32, prelu_part, ups, in_wrap, out16_lo, res1_lo, out_stride_2, out_W, in_stride_2, out16_f16_on_bf16, and the term sets: conv5_without_res1,
  alpha_0 (is), conv5_without_f32_out, conv5_without_16bit_out (layer), mask_in_forward, bias_act_in_dgrad, act_on_conv5, no_act_on_conv1, sigmoid,
  slope_outside_0_1, first_layer_is_conv5_class (is);
  test_refused_shapes[<form>-<shape>]: N not a multiple of 8, 384 / 576 / 1024 tiles (layer), T > 32 at every height, no admissible q (is).  test_acceptance_equals_the_mirror: dasr_rdb_chain accepts exactly when
  RRDBNetHIP.is_launch is not None, dasr_conv_chain exactly when chain_choice under DASR_CHAIN_FORM=layer answers ('layer', 1)."""
import ctypes as C
import math
import types

import pytest
import torch

from oracle import blocked_ref as R
from oracle import conv_ref as CR
from test_gpu_conv import EINVAL, NAN, U32, Weights, c_of, k_epilogue, launch, nan_slab
from test_gpu_elementwise import Slab, _gpu, bounded, gen
from test_gpu_runtime import session

gpu = pytest.mark.gpu
NF, GC = 64, 32
SLOPE = R.f32(0.2)
GUARD = 16                      # guard words around a flag buffer
GUARD_WORD = 0x5a5a5a5a


def _dev():
    dev = _gpu()
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip('the chained launches need a whole 256-CU MI355X (RRDBNetHIP.chain_ok)')
    return dev


def ceil_div(a, b):
    return (a + b - 1) // b


def dev_eq(a, b):
    """bit equality of two device tensors (what biteq of tests/test_gpu_elementwise.py asserts, without the copies to the host; also integer words)"""
    ib = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.int32: torch.int32}
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(ib[a.dtype]), b.contiguous().view(ib[b.dtype])))


def spec(form, bwd, N, h, w, nb=2, prec=1, last16=True, rrdb=False, NP=None, n0=1):
    return types.SimpleNamespace(form=form, bwd=bwd, N=N, h=h, w=w, nb=nb, prec=prec, last16=last16, rrdb=rrdb, NP=NP or N + 2, n0=n0,
                                 kind='f16' if prec == 2 else 'bf16')


_WEIGHTS = {}


def weights(dev, prec, nb):
    """the packed convs of nb dense blocks (cin 64 + 32 k -> 32 / 32 / 32 / 32 / 64), shared by every case of one precision (they are only read)"""
    out = []
    for i in range(5 * nb):
        if (prec, i) not in _WEIGHTS:
            k = i % 5
            cin, cout = NF + GC * k, (NF if k == 4 else GC)
            _WEIGHTS[(prec, i)] = Weights(dev, (cout, cin, 3, 3), cout, cin, 9, 2 if k == 4 else 1, prec, 700 + i)
        out.append(_WEIGHTS[(prec, i)])
    return out


def _blocked(x, kind, dev):
    """NCHW (C a multiple of 16) -> [N][K][H][W][16] on the device"""
    N, C_, H, W = x.shape
    return x.to(dev).to(R.DTYPE[kind]).view(N, C_ // 16, 16, H, W).permute(0, 1, 3, 4, 2).contiguous()


def _nchw(t):
    N, K, H, W, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(N, K * 16, H, W)


class Bufs:
    """one copy of every tensor of a case.  Two copies made from the same spec hold the same bits."""

    def __init__(self, dev, s, seed=11):
        g = gen(seed)
        N, h, w, NP, n0 = s.N, s.h, s.w, s.NP, s.n0
        self.s, self.dev = s, dev
        rng = slice(n0, n0 + N)

        def filled(kind, K, c0, data):     # K planes in a NaN parent, channels [c0, c0 + C) of the launch's images hold data
            t = torch.full((NP, K, h, w, 16), NAN, dtype=R.DTYPE[kind], device=dev)
            t[rng, c0 // 16:c0 // 16 + data.shape[1] // 16] = _blocked(data, kind, dev)
            return self._keep(nan_slab(dev, kind, NP, K, h, w, t))
        self.all = []
        x = torch.randn(N, NF, h, w, generator=g)
        self.slabs = [filled(s.kind, 12, 0, x)]
        for _ in range(1, s.nb):
            self.slabs.append(self._keep(nan_slab(dev, s.kind, NP, 12, h, w, torch.full((NP, 12, h, w, 16), NAN, dtype=R.DTYPE[s.kind], device=dev))))
        self.masks = []
        if s.bwd:
            for _ in range(s.nb):
                m = torch.randn(N, 4 * GC, h, w, generator=g)
                m[0, 0, 0, 0], m[0, 1, 0, 0], m[N - 1, 4 * GC - 1, h - 1, w - 1] = 0.0, -0.0, 0.0      # +0 and -0 are "not > 0"
                self.masks.append(filled(s.kind, 12, NF, m))
        self.x0 = filled('f32', 4, 0, torch.randn(N, NF, h, w, generator=g))
        self.ys = [self._keep(Slab(dev, 'f32', NP, 4, h, w)) for _ in range(s.nb)]
        self.o16 = self._keep(Slab(dev, s.kind, NP, 4, h, w, lead=2)) if s.last16 else None

    def _keep(self, sl):
        sl.before_dev = sl.b.t.clone()
        self.all.append(sl)
        return sl

    def sub(self, sl, k0=0, k1=None):
        """planes [k0, k1) of the view, the launch's images"""
        k1 = sl.K if k1 is None else k1
        return sl.b.t[self.s.n0:self.s.n0 + self.s.N, sl.p0 + k0:sl.p0 + k1]

    def written(self):
        """(slab, first plane, end plane) of everything the chain must write"""
        out = [(S, 0 if b else 4, 12) for b, S in enumerate(self.slabs)] + [(y, 0, 4) for y in self.ys]
        return out + ([(self.o16, 0, 4)] if self.o16 is not None else [])

    def rest_untouched(self):
        """everything but the written planes of the launch's images holds its first bits"""
        wr = {id(sl): (a, b) for sl, a, b in self.written()}
        for sl in self.all:
            want = sl.before_dev.clone()
            if id(sl) in wr:
                a, b = wr[id(sl)]
                r = slice(self.s.n0, self.s.n0 + self.s.N)
                want[r, sl.p0 + a:sl.p0 + b] = sl.b.t[r, sl.p0 + a:sl.p0 + b]
            if not dev_eq(sl.b.t, want):
                return False
        return True

    def untouched(self):
        return all(dev_eq(sl.b.t, sl.before_dev) for sl in self.all)

    def same_as(self, other):
        return [i for i, (a, b) in enumerate(zip(self.all, other.all)) if not dev_eq(a.b.t, b.b.t)]


def layer_terms(s, b, k):
    """the epilogue of conv k + 1 of dense block b as the case table of tests/test_gpu_conv.py describes one (k_epilogue's argument), + gamma"""
    if k < 4:
        return dict(bias=not s.bwd, act=0 if s.bwd else 1, mask=s.bwd, alpha=1.0, res1=None, res2=False, beta1=0.0, beta2=0.0, gamma=1.0)
    two = s.rrdb and b == 2
    if s.bwd:
        return dict(bias=False, act=0, mask=False, alpha=R.f32(0.5), res1='f32', beta1=1.0, res2=two, beta2=1.0, gamma=R.f32(0.04 if two else 0.2))
    return dict(bias=True, act=0, mask=False, alpha=R.f32(0.04 if two else 0.2), res1='f32', beta1=R.f32(0.2 if two else 1.0), res2=two, beta2=1.0, gamma=1.0)


def build_ops(B, W):
    """the 5 nb conv ops of the case on the buffers B, as RRDBNetHIP builds those of its trunk (forward / data gradient), restricted to the launch's images"""
    from dasr_amd.engine import conv_op
    from dasr_amd.rrdbnet import _sub_batch_conv
    s = B.s
    ops, f16 = [], int(s.prec == 2)
    for b in range(s.nb):
        S = B.slabs[b]
        sv = lambda c, S=S: S.b.view(S.p0 * 16 + c)
        for k in range(5):
            cin, wt, t = NF + GC * k, W[5 * b + k], layer_terms(s, b, k)
            kw = dict(bias=wt.P.ptr('b') if t['bias'] else None, act=t['act'], slope=SLOPE, alpha=t['alpha'], gamma=t['gamma'], out16_f16=f16)
            if k < 4:
                if s.bwd:       # the mask of the conv that produces g(x_j) is x_j of the forward slab, j = 4 .. 1
                    M = B.masks[b]
                    kw.update(mask=M.b.view(M.p0 * 16 + NF + GC * (3 - k)), mask_f32=0)
                kw.update(out_bf16=sv(cin))
            else:
                nxt = B.slabs[b + 1] if b + 1 < s.nb else B.o16
                kw.update(res1=(B.ys[b - 1] if b else B.x0).view(), beta1=t['beta1'], out_f32=B.ys[b].view(),
                          out_bf16=None if nxt is None else nxt.b.view(nxt.p0 * 16))
                if t['res2']:
                    kw.update(res2=B.x0.view(), beta2=t['beta2'])
            o = conv_op(wt.pack, wt.ref, sv(0), False, cin, s.h, s.w, s.h, s.w, s.NP, **kw)
            ops.append(_sub_batch_conv(o, s.n0, s.N, s.NP))
    return ops


def plan_deps(ops):
    """dep_chunk as the plans of RRDBNetHIP build it"""
    return [0 if i % 5 == 0 else o.conv.cin // 16 - GC // 16 for i, o in enumerate(ops)]


class Flags:
    """a flag buffer between guard words: tile words, then the eight ticket words"""

    def __init__(self, dev, nwords, preset=0):
        self.n = nwords
        t = torch.full((GUARD + nwords + 8 + GUARD,), GUARD_WORD, dtype=torch.int64)
        t[GUARD:GUARD + nwords] = preset
        t[GUARD + nwords:GUARD + nwords + 8] = 0
        self.full = torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32).to(dev)
        self.t = self.full[GUARD:GUARD + nwords + 8]
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.first = self.full.clone()

    def words(self):
        torch.cuda.synchronize()
        u = self.full.cpu().to(torch.int64) & 0xffffffff
        g = torch.cat([u[:GUARD], u[GUARD + self.n + 8:]])
        assert bool((g == GUARD_WORD).all()), 'guard words around the flag buffer'
        return u[GUARD:GUARD + self.n], u[GUARD + self.n:GUARD + self.n + 8]

    def untouched(self):
        torch.cuda.synchronize()
        return dev_eq(self.full, self.first) and int(self.err.item()) == 0


def flag_words(s):
    return s.N * (ceil_div(s.h, 4) * ceil_div(s.w, 32) if s.form == 'is' else ceil_div(s.h, 16) * ceil_div(s.w, 32))


def make_chain(s, ops, fl, deps=None):
    from dasr_amd.engine import ConvChain
    return ConvChain(ops, plan_deps(ops) if deps is None else deps, s.N, 0, fl.t.device, flags=fl.t, err=fl.err, form=s.form)


def run_chain(ch, via, null=None, nlayers=None):
    """one launch; null: the pointer argument to pass as NULL.  Returns the code."""
    from dasr_amd import _lib
    from dasr_amd.engine import OpList, _stream
    a = dict(dev_layers=ch.dev.data_ptr(), host_layers=C.cast(ch.host, C.c_void_p).value, dev_dep_chunk=ch.dep.data_ptr(), nlayers=ch.n if nlayers is None else nlayers,
             dev_flags=ch.flags.data_ptr(), dev_err=ch.err.data_ptr())
    if null:
        a[null] = None if via == 'abi' else 0
    if ch.form == 'is':
        a.pop('dev_dep_chunk')
    if via == 'op':
        import re
        ol = OpList()
        ol.add(_lib.make_op(_lib.OP_RDB_CHAIN if ch.form == 'is' else _lib.OP_CONV_CHAIN, **a))
        ol.keep.append(ch)
        try:
            ol.run()
            rc = 0
        except _lib.DasrHipError as e:
            rc = int(re.search(r'code (-?\d+)', str(e)).group(1))
    else:
        host = C.cast(a['host_layers'], C.POINTER(_lib.ConvParams)) if a['host_layers'] else None
        if ch.form == 'is':
            rc = _lib.lib().dasr_rdb_chain(a['dev_layers'], host, a['nlayers'], a['dev_flags'], a['dev_err'], _stream())
        else:
            rc = _lib.lib().dasr_conv_chain(a['dev_layers'], host, a['dev_dep_chunk'], a['nlayers'], a['dev_flags'], a['dev_err'], _stream())
    torch.cuda.synchronize()
    return rc


def kernel_tag(s, rows=None):
    b = lambda v: 'true' if v else 'false'
    if s.form == 'is':
        return 'rdb_is_kernel<false, %s, %s>' % (b(s.bwd), {16: '2, 8', 8: '1, 8', 4: '1, 4'}[rows])
    return 'conv_chain_kernel<%s, %s>' % (b(s.prec == 2), b(s.bwd))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the fp64 model
def _detail_dev(weff, bias, x, kind, t, mask, res1, res2):
    """CR.conv_detail for a 3 x 3 / 1 / 1 conv on 16-bit operands, as fp64 matrix products on the device of x (held to conv_detail by
    test_fp64_model_on_the_device_is_conv_ref).  x, mask, res1, res2: NCHW device tensors; weff [cout][cin][9] fp32 (CR.pack_weights)."""
    dev = x.device
    N, cin, h, w = x.shape
    wd = R.r16(weff.float(), kind).double().to(dev)
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    acc = S = 0.0
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        p = xp[:, :, ky:ky + h, kx:kx + w].reshape(N, cin, h * w)
        acc = acc + torch.matmul(wd[:, :, tap], p)
        S = S + torch.matmul(wd[:, :, tap].abs(), p.abs())
    acc, S = acc.view(N, -1, h, w), S.view(N, -1, h, w)
    v, mag, gain = acc, acc.abs(), 1.0
    if bias is not None:
        b = bias.double().to(dev).view(1, -1, 1, 1)
        v, mag = v + b, mag + b.abs()
    if t['act'] == 1:
        f = torch.where(v > 0, torch.ones_like(v), torch.full_like(v, SLOPE))
        v, mag, gain = v * f, mag * f.abs(), gain * max(1.0, abs(SLOPE))
    if mask is not None:
        f = torch.where(mask.double() > 0, torch.ones_like(v), torch.full_like(v, SLOPE))
        v, mag, gain = v * f, mag * f.abs(), gain * max(1.0, abs(SLOPE))
    v, mag, gain = t['alpha'] * v, abs(t['alpha']) * mag, gain * abs(t['alpha'])
    r1 = None
    if res1 is not None:
        r1 = res1.double()
        v, mag = v + t['beta1'] * r1, mag + (t['beta1'] * r1).abs()
    if res2 is not None:
        v, mag = v + t['beta2'] * res2.double(), mag + (t['beta2'] * res2.double()).abs()
    return dict(ref=v, S=S, L=9 * cin, terms=mag, gain=gain, r1=r1)


def _detail(weff, bias, x, kind, prec, t, mask, res1, res2, on_cpu):
    if not on_cpu:
        return _detail_dev(weff, bias, x, kind, t, mask, res1, res2)
    c = lambda v: None if v is None else v.cpu()
    return CR.conv_detail(weff, bias, c(x).float(), x.shape[2], x.shape[3], prec=prec, act=t['act'], slope=SLOPE, mask=c(mask), alpha=t['alpha'],
                          res1=c(res1), beta1=t['beta1'], res2=c(res2), beta2=t['beta2'])


def check_fp64(B, W, margins, label):
    """every layer of the chain that ran on B against the fp64 model, on its actual 16-bit inputs"""
    s = B.s
    on_cpu = s.N * s.h * s.w <= 4096
    put = (lambda v: v.cpu()) if on_cpu else (lambda v: v)
    for b in range(s.nb):
        S = B.slabs[b]
        for k in range(5):
            t, wt, cin = layer_terms(s, b, k), W[5 * b + k], NF + GC * k
            x = _nchw(B.sub(S, 0, cin // 16)).float()
            mask = _nchw(B.sub(B.masks[b], 4 + 2 * (3 - k), 6 + 2 * (3 - k))).float() if t['mask'] else None
            res1 = _nchw(B.sub(B.ys[b - 1] if b else B.x0)) if t['res1'] else None
            res2 = _nchw(B.sub(B.x0)) if t['res2'] else None
            d = _detail(wt.eff, wt.b if t['bias'] else None, x, s.kind, s.prec, t, mask, res1, res2, on_cpu)
            nxt = B.slabs[b + 1] if b + 1 < s.nb else B.o16
            # conv5 with 16-bit planes starts its accumulators at (beta1 / alpha) res1 (the conv5-class launches of dasr_conv, see the header); without them
            # (the last block of an input-stationary chain) it is the generic epilogue, alpha acc + beta1 res1
            # (This restates the launcher's classification, which tests/test_gpu_conv.py avoids by marking its cases: it moves k and L by one unit each.  The chain runs
            # what it runs whatever the test assumes; were the rule to change, the fp32 streams -- at a tenth of the bound today -- would be held a unit tighter or looser.)
            r1_pre = k == 4 and nxt is not None
            Sacc = d['S'] + ((t['beta1'] * d['r1']).abs() / abs(t['alpha']) if r1_pre else 0.0)
            b32 = c_of(d['L'] + (1 if r1_pre else 0)) * 2.0 ** -23 * Sacc * d['gain'] + k_epilogue(t, r1_pre) * U32 * d['terms']
            tag = 'chain %s b%d conv%d' % (label, b, k + 1)
            ref, gamma = d['ref'], t['gamma']
            if k == 4:
                bounded(tag + ' f32', put(_nchw(B.sub(B.ys[b]))), ref, b32, margins)
            o16 = B.sub(S, cin // 16, cin // 16 + 2) if k < 4 else (None if nxt is None else B.sub(nxt, 0, 4))
            if o16 is not None:
                gref = gamma * ref
                f32_term = abs(gamma) * b32 + (0.0 if gamma in (0.5, 1.0, 2.0) else U32 * gref.abs())      # gamma * v: one more rounding unless a power of two
                bounded(tag + ' 16', put(_nchw(o16)), gref, f32_term + R.err16(gref.abs() + f32_term, s.kind), margins)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def run_case(s, via, margins, fp64=False, label='', expect=None):
    """chain on one copy of the buffers, per-layer launches on a second: bits, surroundings, flag counts, error word; returns (chain copy, flags)"""
    dev = _dev()
    from dasr_amd.rrdbnet import RRDBNetHIP
    W = weights(dev, s.prec, s.nb)
    A, Bref = Bufs(dev, s), Bufs(dev, s)
    assert not A.same_as(Bref)
    fl = Flags(dev, flag_words(s))
    ch = make_chain(s, build_ops(A, W), fl)
    rows = q = None
    if s.form == 'is':
        mirror = RRDBNetHIP.is_launch(s.N, s.h, s.w)
        assert mirror is not None and (expect is None or mirror == expect), (mirror, expect)
        rows, q, _ = mirror
    recs, _ = session(lambda: _expect_ok(run_chain(ch, via)))
    assert [r.tag for r in recs] == [kernel_tag(s, rows)], [r.tag for r in recs]
    assert int(fl.err.item()) == 0
    check_flags(s, fl, 1, rows, q)
    for o in build_ops(Bref, W):
        assert launch(o, 'abi') == 0
    assert A.rest_untouched() and Bref.rest_untouched()
    for sl, a, b in A.written():
        assert bool(torch.isfinite(A.sub(sl, a, b).float()).all()), 'non-finite output: a plane was read before it was written, or outside the view'
    bad = A.same_as(Bref)
    if bad:
        pytest.fail('chain and per-layer launches differ: ' + where_differs(A, Bref, rows))
    if fp64:
        check_fp64(A, W, margins, '%s %s' % (kernel_tag(s, rows), label))
    return A, fl, ch


def _expect_ok(rc):
    assert rc == 0, rc


def check_flags(s, fl, launches, rows=None, q=None, preset=0):
    """tile words of the geometry that ran: preset + launches x layers, the rest of the buffer as it was; tickets: launches x workgroups per XCD"""
    tiles, tickets = fl.words()
    used = s.N * ceil_div(s.h, rows or 16) * ceil_div(s.w, 32)
    want = (preset + launches * 5 * s.nb) & 0xffffffff
    assert bool((tiles[:used] == want).all()), (tiles[:used].unique().tolist(), want)
    assert bool((tiles[used:] == preset).all()), 'flag words behind the tiles of the height that ran'
    assert tickets.tolist() == [launches * (q if s.form == 'is' else 64)] * 8, tickets.tolist()


def where_differs(A, Bref, rows):
    """first differing (buffer, layer, image, tile) of two copies, for the failure message"""
    s, th = A.s, rows or 16
    names = ['slab%d' % b for b in range(s.nb)] + ['mask%d' % b for b in range(len(A.masks))] + ['x0'] + ['y%d' % b for b in range(s.nb)] + ['o16']
    out = []
    for i, (a, b) in enumerate(zip(A.all, Bref.all)):
        d = (a.b.t.float() != b.b.t.float()) & ~(torch.isnan(a.b.t.float()) & torch.isnan(b.b.t.float()))
        if bool(d.any()):
            n, p, y, x, _ = [int(v) for v in d.nonzero()[0]]
            pl = p - a.p0
            what = ('conv%d' % ((pl - 4) // 2 + 1) if pl >= 4 else 'x / conv5 of the block before') if names[i].startswith('slab') else 'conv5'
            out.append('%s plane %d (%s) image %d row %d col %d = tile (%d, %d), %d elements' % (names[i], pl, what, n - s.n0, y, x, y // th, x // 32, int(d.sum())))
    return '; '.join(out)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# input-stationary form: (N, h, w) -> (rows, q, tiles per workgroup), computed with the rule of dasr_rdb_chain and confirmed by the mirror and by what ran.
# The rule sees h and w only through ceil(h / rows) and ceil(w / 32): every shape has siblings with full or partial last tiles and the same geometry.
IS_SHAPES = [
    # 4 rows: one tile per workgroup (full / partial last column, partial last row with both, narrower than a tile) ...
    ((8, 4, 32), (4, 1, 1)), ((8, 4, 36), (4, 2, 1)), ((8, 6, 64), (4, 4, 1)), ((8, 6, 36), (4, 4, 1)), ((8, 6, 8), (4, 2, 1)),
    # ... two, five
    ((48, 4, 192), (4, 18, 2)), ((48, 4, 164), (4, 18, 2)), ((48, 3, 192), (4, 18, 2)), ((48, 3, 164), (4, 18, 2)),
    ((40, 8, 224), (4, 14, 5)), ((40, 8, 196), (4, 14, 5)), ((40, 6, 224), (4, 14, 5)), ((40, 6, 196), (4, 14, 5)),
    # 8 rows: one (the last: narrower than a tile), two, three, five, eight
    ((8, 136, 32), (8, 17, 1)), ((8, 72, 36), (8, 18, 1)), ((48, 10, 64), (8, 24, 1)), ((48, 10, 36), (8, 24, 1)), ((8, 144, 8), (8, 18, 1)),
    ((48, 24, 96), (8, 27, 2)), ((48, 24, 68), (8, 27, 2)), ((48, 18, 96), (8, 27, 2)), ((48, 18, 68), (8, 27, 2)), ((24, 82, 36), (8, 22, 3)),
    ((40, 136, 32), (8, 17, 5)), ((40, 136, 8), (8, 17, 5)), ((40, 129, 32), (8, 17, 5)), ((40, 129, 8), (8, 17, 5)), ((64, 34, 164), (8, 30, 8)),
    # 16 rows: one (the last: narrower than a tile), two, three, five, eight
    ((8, 48, 192), (16, 18, 1)), ((8, 144, 36), (16, 18, 1)), ((48, 18, 64), (16, 24, 1)), ((48, 18, 36), (16, 24, 1)), ((128, 32, 8), (16, 32, 1)),
    ((48, 48, 64), (16, 18, 2)), ((48, 48, 36), (16, 18, 2)), ((48, 42, 64), (16, 18, 2)), ((48, 42, 36), (16, 18, 2)), ((24, 130, 36), (16, 18, 3)),
    ((40, 144, 64), (16, 18, 5)), ((40, 144, 36), (16, 18, 5)), ((40, 130, 64), (16, 18, 5)), ((64, 130, 36), (16, 18, 8)),
]


def _cell(shape, expect):
    """(rows, tiles per workgroup as 1 / 2 / 'more than 4' / the count, last tile row full, last tile column full)"""
    rows, _, tpw = expect
    return rows, ('>4' if tpw > 4 else tpw), shape[1] % rows == 0, shape[2] % 32 == 0


# every cell of tile height x tiles per workgroup 1 / 2 / more than 4 x last tile row full / partial x last tile column full / partial has a shape
assert {_cell(*e) for e in IS_SHAPES} >= {(r, t, fr, fc) for r in (16, 8, 4) for t in (1, 2, '>4') for fr in (True, False) for fc in (True, False)}
# block count / residual set / 16-bit planes of the last conv5, rotated over the shapes
IS_VARIANT = [dict(nb=2, last16=True), dict(nb=3, rrdb=True, last16=False), dict(nb=2, last16=False), dict(nb=3, rrdb=True, last16=True), dict(nb=1, last16=True)]
IS_BIG = 150000      # pixels above which a case runs two blocks (they are what exercises the waits; a third only repeats them)


def _is_spec(i, shape, bwd):
    N, h, w = shape
    var = IS_VARIANT[(i + (2 if bwd else 0)) % len(IS_VARIANT)]
    if N * h * w > IS_BIG:
        var = dict(nb=2, last16=bool((i + bwd) % 2))
    return spec('is', bwd, N, h, w, **var)


# ... so that every conv5 epilogue (one / two residuals x with / without 16-bit planes: 233 249 169 185 forward, 232 248 168 184 data gradient) runs at every
# tile height in both directions
for _bwd in (False, True):
    for _rows in (16, 8, 4):
        _seen = {(v.rrdb, v.last16) for v in (_is_spec(i, sh, _bwd) for i, (sh, ex) in enumerate(IS_SHAPES) if ex[0] == _rows)}
        assert _seen == {(False, True), (True, False), (False, False), (True, True)}, (_bwd, _rows, _seen)


@gpu
@pytest.mark.parametrize('i', range(len(IS_SHAPES)), ids=['%dx%dx%d' % s for s, _ in IS_SHAPES])
@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_is_geometry(bwd, i, margins):
    shape, expect = IS_SHAPES[i]
    s = _is_spec(i, shape, bwd)
    rows, q, tpw = expect
    assert 8 * q * tpw == shape[0] * ceil_div(shape[1], rows) * ceil_div(shape[2], 32) and 8 * q <= 256 and tpw <= 8       # the table is consistent with itself
    fp64 = shape[0] * shape[1] * shape[2] <= 60000
    run_case(s, 'op' if (i + bwd) % 2 else 'abi', margins, fp64=fp64, label='%dx%dx%d nb%d' % (shape + (s.nb,)), expect=expect)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# layer form: exactly 512 tiles of 16 x 32
LAYER_SHAPES = [('32x50x100', dict(N=32, h=50, w=100)), ('16x120x120', dict(N=16, h=120, w=120)), ('64x20x100', dict(N=64, h=20, w=100)),
                ('512x16x32', dict(N=512, h=16, w=32)), ('512x10x20', dict(N=512, h=10, w=20)), ('8x128x256', dict(N=8, h=128, w=256)),
                ('16of32x128x128', dict(N=16, h=128, w=128, NP=32, n0=16))]
LAYER_FP64 = ('64x20x100', '512x10x20')
LAYER_VARIANT = [dict(nb=2), dict(nb=3, rrdb=True), dict(nb=1)]


@gpu
@pytest.mark.parametrize('i', range(len(LAYER_SHAPES)), ids=[n for n, _ in LAYER_SHAPES])
@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('prec', [1, 2], ids=['bf16', 'f16'])
def test_layer_geometry(prec, bwd, i, margins):
    name, shape = LAYER_SHAPES[i]
    var = dict(nb=2) if shape.get('NP') else LAYER_VARIANT[(i + bwd + prec) % 3]      # (the parent of 32 images: two blocks keep the case quick)
    s = spec('layer', bwd, prec=prec, **dict(var, **shape))
    assert s.N * ceil_div(s.h, 16) * ceil_div(s.w, 32) == 512 and s.N % 8 == 0
    run_case(s, 'abi' if (i + bwd) % 2 else 'op', margins, fp64=name in LAYER_FP64, label='%s nb%d' % (name, s.nb))


@gpu
@pytest.mark.parametrize('name', ['32x50x100', '512x10x20'])
@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('prec', [1, 2], ids=['bf16', 'f16'])
def test_layer_dep_chunk_every_chunk(prec, bwd, name, margins):
    """dep_chunk <= 0 ("every chunk": the wait in front of the layer's first chunk) against the values the plan builds, and against a chain whose
    dependent chunks are declared one chunk early: the same bits"""
    dev = _dev()
    s = spec('layer', bwd, prec=prec, nb=2, **dict(LAYER_SHAPES)[name])
    W = weights(dev, prec, s.nb)
    A, fl = run_case(s, 'abi', margins)[:2]
    for deps in ([0] * 10, [-1] * 10, [max(d - 1, 0) for d in plan_deps(build_ops(A, W))]):
        Z, flz = Bufs(dev, s), Flags(dev, flag_words(s))
        assert run_chain(make_chain(s, build_ops(Z, W), flz, deps=deps), 'op') == 0
        assert int(flz.err.item()) == 0 and Z.rest_untouched() and not Z.same_as(A), deps
        check_flags(s, flz, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
FLAG_CASES = [('is-8x6x8-4rows', ('is', 8, 6, 8)), ('is-48x18x68-8rows-q27', ('is', 48, 18, 68)), ('is-24x130x36-16rows-3tiles', ('is', 24, 130, 36)),
              ('layer-64x20x100', ('layer', 64, 20, 100)), ('layer-512x10x20', ('layer', 512, 10, 20))]


@gpu
@pytest.mark.parametrize('case', [c for _, c in FLAG_CASES], ids=[n for n, _ in FLAG_CASES])
@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_flags_count_on_and_wrap(bwd, case, margins):
    """the flag words count on from launch to launch and a tile compares its neighbours' words with its own start value: three launches on one buffer,
    then buffers whose tile words all start at 0x7ffffff0 / 0xfffffff0 (tickets 0) -- the words cross 2^31 / 2^32 inside the second launch of each --
    give the bits of the first launch"""
    from dasr_amd.rrdbnet import RRDBNetHIP
    form, N, h, w = case
    s = spec(form, bwd, N, h, w, nb=2)
    A, fl, ch = run_case(s, 'abi', margins)
    rows, q = RRDBNetHIP.is_launch(N, h, w)[:2] if form == 'is' else (None, None)
    first = [sl.b.t.clone() for sl in A.all]
    for n in (2, 3):
        assert run_chain(ch, 'op' if n == 2 else 'abi') == 0
        assert int(fl.err.item()) == 0
        check_flags(s, fl, n, rows, q)
        assert all(dev_eq(sl.b.t, f) for sl, f in zip(A.all, first)), 'launch %d' % n
    W = weights(A.dev, s.prec, s.nb)
    for preset in (0x7ffffff0, 0xfffffff0):
        Z, flz = Bufs(A.dev, s), Flags(A.dev, flag_words(s), preset=preset)
        chz = make_chain(s, build_ops(Z, W), flz)
        for n in (1, 2):
            assert run_chain(chz, 'abi') == 0
            assert int(flz.err.item()) == 0
            check_flags(s, flz, n, rows, q, preset=preset)
            assert all(dev_eq(sl.b.t, f) for sl, f in zip(Z.all, first)), 'preset %#x launch %d' % (preset, n)
        assert ((preset + 5 * s.nb) ^ (preset + 10 * s.nb)) & (1 << 31) or (preset + 10 * s.nb) >> 32      # the second launch crossed


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# refusals
def _set(idx, **kw):
    def f(ops):
        for i in ([idx] if isinstance(idx, int) else idx):
            for k, v in kw.items():
                setattr(ops[i].conv, k, v)
    return f


def _move(name, idx=1, by=64):
    def f(ops):
        t = getattr(ops[idx].conv, name)
        t.p = t.p + by
    return f


def _null(name, idx):
    def f(ops):
        from dasr_amd.engine import NULL_T
        setattr(ops[idx].conv, name, NULL_T)
    return f


def _f16_chain(ops):
    for o in ops:
        o.conv.prec, o.conv.out16_f16 = 2, 1


def _own(name):
    """the pointer field takes a live device address (that of the op's weights)"""
    def f(ops):
        c = ops[1].conv
        setattr(c, name, C.cast(c.w, C.c_void_p).value)
    return f


# (clause, forms, directions, mutation of the op list)
REFUSALS = [
    ('kh_4', 'is layer', 'f', _set(2, kh=4)), ('stride_2', 'is layer', 'f', _set(2, stride=2)), ('pad_0', 'is layer', 'b', _set(3, pad=0)),
    ('in_f32', 'is layer', 'f', _set(1, in_f32=1)), ('mixed_prec', 'is layer', 'fb', _set(2, prec=2, out16_f16=1)),
    ('f16', 'is', 'fb', _f16_chain),
    ('other_geometry_H', 'is layer', 'f', _set(3, Hin=5, Hout=5)), ('other_geometry_W', 'is layer', 'b', _set(4, Win=31, Wout=31)), ('other_N', 'is layer', 'f', _set(2, N=16)),
    ('cin_80_on_conv2', 'is', 'f', _set(1, cin=80)), ('cin_not_16', 'layer', 'f', _set(1, cin=88)), ('mt_2_on_conv2', 'is layer', 'f', _set(1, mt=2)), ('mt_1_on_conv5', 'is', 'f', _set(4, mt=1)),
    ('cout_64_on_conv3', 'is layer', 'b', _set(2, cout=64)), ('mt_3', 'layer', 'f', _set(2, mt=3)), ('w_null', 'is layer', 'f', _set(3, w=None)),
    ('two_slabs', 'is', 'fb', _move('inp', 2)), ('slab_strides', 'is', 'f', lambda ops: setattr(ops[3].conv.inp, 'cb_stride', ops[3].conv.inp.cb_stride * 2)),
    ('slope_ptr', 'is layer', 'fb', _own('slope_ptr')), ('mask_f32', 'is layer', 'b', _set(1, mask_f32=1)), ('prelu_part', 'is layer', 'b', _own('prelu_part')),
    ('ups', 'is layer', 'f', _set(0, ups=1)), ('in_wrap', 'is layer', 'f', _set(1, in_wrap=4)), ('out16_lo', 'is layer', 'f', _set(4, out16_lo=4)),
    ('res1_lo', 'is layer', 'b', _set(4, res1_lo=4)), ('out_stride_2', 'is layer', 'f', _set(4, out_stride=2)), ('out_W', 'is layer', 'f', _set(0, out_W=64)),
    ('in_stride_2', 'is layer', 'f', _set(1, in_stride=2)), ('out16_f16_on_bf16', 'is layer', 'f', _set(0, out16_f16=1)),
    ('conv5_without_res1', 'is layer', 'fb', _null('res1', 4)), ('alpha_0', 'is', 'fb', _set(4, alpha=0.0)),
    ('conv5_without_f32_out', 'is layer', 'f', _null('out_f32', 4)), ('conv5_without_16bit_out', 'layer', 'fb', _null('out_bf16', 4)),
    ('mask_in_forward', 'is layer', 'f', lambda ops: setattr(ops[2].conv, 'mask', ops[2].conv.out_bf16)),
    ('bias_act_in_dgrad', 'is layer', 'b', lambda ops: (setattr(ops[1].conv, 'bias', C.cast(ops[1].conv.w, C.c_void_p).value), setattr(ops[1].conv, 'act', 1))),
    ('act_on_conv5', 'is layer', 'f', _set(4, act=1)), ('no_act_on_conv1', 'is layer', 'f', _set(0, act=0)), ('sigmoid', 'is layer', 'f', _set(1, act=2)),
    ('slope_outside_0_1', 'is layer', 'f', _set(1, slope=1.5)), ('first_layer_is_conv5_class', 'is', 'f', _set(0, alpha=0.5)),
]
REFUSAL_CASES = [('%s-%s-%s' % (form, 'fwd' if d == 'f' else 'bwd', name), form, d == 'b', mut) for name, forms, dirs, mut in REFUSALS for form in forms.split() for d in dirs]
REFUSAL_ARGS = [('%s-%s' % (form, name), form, name) for form in ('is', 'layer') for name in
                ('null_dev_layers', 'null_host_layers', 'null_dev_flags', 'null_dev_err', 'nlayers_0', 'nlayers_neg') + (('nlayers_7',) if form == 'is' else ('null_dev_dep_chunk',))]
_BASE = {}


def _refusal_base(dev, form, bwd):
    """a valid one-block chain (the smallest shape of its form) whose refused variants leave every buffer as it is: built once, shared"""
    if (form, bwd) not in _BASE:
        s = spec(form, bwd, 8, 4, 32, nb=1) if form == 'is' else spec(form, bwd, 512, 10, 20, nb=1)
        B = Bufs(dev, s)
        _BASE[(form, bwd)] = (s, B, weights(dev, 1, 1), Flags(dev, flag_words(s)))
    return _BASE[(form, bwd)]


@gpu
@pytest.mark.parametrize('name,form,bwd,mutate', REFUSAL_CASES, ids=[c[0] for c in REFUSAL_CASES])
def test_refusals(name, form, bwd, mutate):
    dev = _dev()
    s, B, W, fl = _refusal_base(dev, form, bwd)
    ops = build_ops(B, W)
    mutate(ops)
    ch = make_chain(s, ops, fl, deps=plan_deps(build_ops(B, W)))
    for via in ('abi', 'op'):
        assert run_chain(ch, via) == EINVAL, (name, via)
        assert B.untouched() and fl.untouched(), (name, via)


@gpu
@pytest.mark.parametrize('name,form,what', REFUSAL_ARGS, ids=[c[0] for c in REFUSAL_ARGS])
def test_refused_arguments(name, form, what):
    dev = _dev()
    s, B, W, fl = _refusal_base(dev, form, False)
    ch = make_chain(s, build_ops(B, W) * (2 if what == 'nlayers_7' else 1), fl)
    kw = dict(null=what[5:]) if what.startswith('null_') else dict(nlayers={'nlayers_0': 0, 'nlayers_neg': -5, 'nlayers_7': 7}[what])
    for via in ('abi', 'op'):
        assert run_chain(ch, via, **kw) == EINVAL, (name, via)
        assert B.untouched() and fl.untouched(), (name, via)


@gpu
@pytest.mark.parametrize('form', ['is', 'layer'])
@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_the_chain_the_refusals_are_derived_from_runs(bwd, form, margins):
    s, _, _, _ = _refusal_base(_dev(), form, bwd)
    run_case(s, 'abi', margins)


class Plain:
    """a one-block forward chain on zero-filled tensors of their own (no parent, no copy on the host): shapes a launcher accepts or refuses"""

    def __init__(self, dev, form, N, h, w):
        from dasr_amd.engine import BTensor, conv_op
        W = weights(dev, 1, 1)
        self.s = spec(form, False, N, h, w, nb=1, NP=N, n0=0)
        self.t = [BTensor(N, 12 * 16, h, w, False, dev), BTensor(N, NF, h, w, True, dev), BTensor(N, NF, h, w, True, dev), BTensor(N, NF, h, w, False, dev)]
        S, x0, y, o16 = self.t
        self.ops = []
        for k in range(5):
            cin, wt = NF + GC * k, W[k]
            if k < 4:
                self.ops.append(conv_op(wt.pack, wt.ref, S.view(0), False, cin, h, w, h, w, N, bias=wt.P.ptr('b'), act=1, slope=SLOPE, out_bf16=S.view(cin)))
            else:
                self.ops.append(conv_op(wt.pack, wt.ref, S.view(0), False, cin, h, w, h, w, N, bias=wt.P.ptr('b'), alpha=R.f32(0.2), res1=x0.view(), beta1=1.0,
                                        out_f32=y.view(), out_bf16=o16.view()))
        self.fl = Flags(dev, flag_words(self.s) if form == 'is' else 512)     # (the layer form's tickets sit behind 512 tile words)
        self.ch = make_chain(self.s, self.ops, self.fl)

    def zero(self):
        return all(not bool(t.t.any()) for t in self.t)


IS_BORDER = [(8, 128, 128), (16, 128, 128), (24, 128, 128), (32, 128, 128), (72, 128, 128), (88, 64, 64), (64, 64, 64), (8, 132, 128), (8, 128, 132), (8, 128, 112), (16, 32, 32),
             (16, 64, 64), (12, 32, 32), (4, 32, 32), (8, 1, 1), (40, 32, 32), (56, 32, 32), (72, 32, 32), (8, 16, 1024), (8, 16, 1056), (8, 256, 128), (16, 64, 128)]
LAYER_BORDER = [(16, 128, 128), (16, 128, 96), (16, 144, 128), (16, 112, 128), (32, 128, 128), (24, 128, 256), (8, 256, 128), (8, 128, 256), (8, 129, 256), (4, 256, 256),
                (12, 128, 128), (64, 64, 64), (256, 32, 32), (256, 32, 33), (512, 16, 32), (512, 17, 32), (504, 16, 32), (520, 16, 32), (32, 50, 100), (16, 120, 120), (16, 192, 192)]
BORDER = [('is',) + c for c in IS_BORDER] + [('layer',) + c for c in LAYER_BORDER]


@gpu
@pytest.mark.parametrize('form,N,h,w', BORDER, ids=['%s-%dx%dx%d' % c for c in BORDER])
def test_acceptance_equals_the_mirror(form, N, h, w, monkeypatch):
    """dasr_rdb_chain accepts exactly the shapes RRDBNetHIP.is_launch names a geometry for, dasr_conv_chain exactly those chain_choice gives ('layer', 1)
    under DASR_CHAIN_FORM=layer; an accepted shape runs (q workgroups per XCD as the mirror says), a refused one touches nothing"""
    dev = _dev()
    from dasr_amd.rrdbnet import RRDBNetHIP
    if form == 'is':
        mirror = RRDBNetHIP.is_launch(N, h, w)
        accept = mirror is not None
    else:
        monkeypatch.delenv('DASR_CHAIN_SPLIT', raising=False)
        net = types.SimpleNamespace(chain=True, chain_form='layer', device=dev, nf=NF)
        accept = RRDBNetHIP.chain_choice(net, N, h, w)[:2] == ('layer', 1)
    p = Plain(dev, form, N, h, w)
    for via in ('abi', 'op'):
        rc = run_chain(p.ch, via)
        assert rc == (0 if accept else EINVAL), (rc, accept, via)
        if not accept:
            assert p.fl.untouched() and p.zero()
    if accept:
        assert int(p.fl.err.item()) == 0
        rows, q = mirror[:2] if form == 'is' else (None, None)
        check_flags(p.s, p.fl, 2, rows, q)
        assert all(bool(torch.isfinite(t.t.float()).all()) for t in p.t)


REFUSED_SHAPES = [('is', 12, 32, 32), ('is', 72, 128, 128), ('is', 88, 64, 64), ('is', 8, 132, 128),
                  ('layer', 12, 128, 128), ('layer', 16, 128, 96), ('layer', 16, 144, 128), ('layer', 32, 128, 128)]


@gpu
@pytest.mark.parametrize('form,N,h,w', REFUSED_SHAPES, ids=['%s-%dx%dx%d' % c for c in REFUSED_SHAPES])
def test_refused_shapes(form, N, h, w):
    """the geometry clauses by name, whatever the mirror says: N not a multiple of 8; input-stationary form: more than 32 tiles per image at every height
    (8 x 132 x 128), no admissible q (72 x 128 x 128, 88 x 64 x 64); layer form: not 512 tiles (384, 576, 1024)"""
    p = Plain(_dev(), form, N, h, w)
    for via in ('abi', 'op'):
        assert run_chain(p.ch, via) == EINVAL
        assert p.fl.untouched() and p.zero()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_fp64_model_on_the_device_is_conv_ref(bwd):
    """_detail_dev (fp64 matrix products on the device) gives what oracle.conv_ref.conv_detail gives: every returned quantity to 1e-12 of its scale"""
    dev = _gpu()
    g = gen(5)
    N, h, w, kind = 2, 7, 37, 'bf16'
    for k in (0, 4):
        cin, cout = NF + GC * k, (NF if k == 4 else GC)
        t = layer_terms(spec('is', bwd, N, h, w, nb=3, rrdb=True), 2, k)
        weff = torch.randn(cout, cin, 9, generator=g) * 0.05
        bias = torch.randn(cout, generator=g) if t['bias'] else None
        x = R.r16(torch.randn(N, cin, h, w, generator=g), kind).float()
        mask = R.r16(torch.randn(N, cout, h, w, generator=g), kind).float() if t['mask'] else None
        res1 = torch.randn(N, cout, h, w, generator=g) if t['res1'] else None
        res2 = torch.randn(N, cout, h, w, generator=g) if t['res2'] else None
        d = lambda v: None if v is None else v.to(dev)
        a = _detail(weff, bias, d(x), kind, 1, t, d(mask), d(res1), d(res2), on_cpu=False)
        b = _detail(weff, bias, d(x), kind, 1, t, d(mask), d(res1), d(res2), on_cpu=True)
        assert a['L'] == b['L'] and math.isclose(a['gain'], b['gain'], rel_tol=1e-15)
        for key in ('ref', 'S', 'terms'):
            assert float((a[key].cpu() - b[key]).abs().max()) <= 1e-12 * float(b['terms'].abs().max() + b['S'].abs().max()), key
