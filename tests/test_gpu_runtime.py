"""GPU tests of the host runtime around the kernels (csrc/misc.hip, dasr_amd/engine.py): the scratch rows of the deterministic grid sums
(dasr_red_scratch / dasr_red_release / grid_sum_commit of csrc/common.h), the threaded enqueuer (dasr_run_ops_mt, engine.run_parallel), the scheduling
ops (OP_EVENT_RECORD / OP_STREAM_WAIT / OP_SET_STREAM, OpList.run(lo, hi)) and the profiling session (dasr_prof_begin / _end / _filter).  The CPU side
(OpList.safe_cuts, argument checks) is tests/test_runtime_host.py.  Machinery (call, Slab, Buf) from tests/test_gpu_elementwise.py.

What is asserted.
  A  Grid sums on INTEGER data: a - b in {0, +-1, +-2, +-3}, coef 1, an integer in the accumulator, every total below 2^24 (asserted on the CPU for each
     case): every partial sum of every order is an integer below 2^24, so fp32 adds are exact and the accumulator must hold acc0 + sum BIT FOR BIT --
     a partial dropped, read twice or read before it was written, a ticket that did not start from zero, a lost add of two streams all move it by an
     integer.  Launch sizes: 1, 2, 256, 257, 513 workgroups (the last arriver's loop of 1, 2, 3 rounds and its 256 / 257 edge) and 4113 (the row grows past
     its first 4096 floats).  K = 2 and K = 3 (dasr_gan_loss, dasr_ragan stage 1) at about 300 workgroups against the fp64 references and the bounds of
     oracle/norm_gan_cases.py, whose grid-chain term counts the two loop rounds.
  B  Order-dependent programs of OP_FILL / OP_ADD_FLAT (y += y, y += z, z += y, re-fills) on private buffers, about 200 ops per list, emulated on the
     host in fp32 -- the same IEEE adds, so the buffers must match bit for bit; failures by an op that returns DASR_EINVAL before launching.
  C  Event and stream ops by a consumer that is only right if the wait / the redirect took effect: the producer stream is held back for tens of
     milliseconds by dasr_probe_spin (bench library), the enqueue takes microseconds.
  D  The records of a profiling session, field by field."""
import collections
import ctypes as C
import functools
import random
import struct
import time

import pytest
import torch

from oracle import blocked_ref as R
from oracle import norm_gan_cases as K
from test_gpu_elementwise import SENT, U32, VIA, Buf, Slab, _gpu, _grid_chain, biteq, bounded, call, gen, gpu
from test_gpu_norm_gan import check_acc, slab

EINVAL, ECAPTURE = -22, -16
LIMIT = 2 ** 24                           # integers up to here are fp32 numbers: sums that stay below are exact in any order


def _L():
    from dasr_amd import _lib
    return _lib.lib()


def _f32(v):
    return struct.unpack('<f', struct.pack('<f', v))[0]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# A. grid sums.  dasr_l1_diff launches ceil(N * ceil(C / 16) * H * W * 4 / 256) workgroups, K = 1
L1_SHAPES = {1: (1, 13, 5, 7), 2: (2, 13, 5, 7), 256: (1, 13, 127, 129), 257: (1, 13, 113, 145), 513: (3, 13, 95, 115), 4113: (1, 16, 513, 513)}
ACC0 = 1000.0


def l1_blocks(N, Cc, H, W):
    return (N * R.planes(Cc) * H * W * 4 + 255) // 256


@functools.lru_cache(maxsize=None)
def int_case(nwg, seed=0):
    """(a, b, sum |a - b|) with a - b in {0, +-1, +-2, +-3} and |a|, |b| <= 7 (exact in bf16 too); made once per shape and shared"""
    N, Cc, H, W = L1_SHAPES[nwg]
    assert l1_blocks(N, Cc, H, W) == nwg
    g = gen(7000 + 13 * nwg + seed)
    d = torch.randint(-3, 4, (N, Cc, H, W), generator=g).float()
    b = torch.randint(-4, 5, (N, Cc, H, W), generator=g).float()
    a = b + d
    total = int(d.double().abs().sum())
    assert 0 < total and ACC0 + total < LIMIT, total               # the reference alone guarantees exactness
    assert bool((R.r16(a, 'bf16').float() == a).all()) and bool((R.r16(b, 'bf16').float() == b).all())
    return a, b, total


class L1Case:
    """the integer case of `nwg` workgroups on the device: a and b as planes of sentinel-filled slabs, garbage in their padding channels"""

    def __init__(self, dev, nwg, kind='f32', seed=0):
        self.nwg, self.kind, self.shape = nwg, kind, L1_SHAPES[nwg]
        N, Cc, H, W = self.shape
        a, b, self.total = int_case(nwg, seed)
        self.a = Slab(dev, kind, N, R.planes(Cc), H, W, R.pack(a, kind, pad=SENT))
        self.b = Slab(dev, kind, N, R.planes(Cc), H, W, R.pack(b, kind, pad=77.0), lead=2)

    def kw(self, acc_ptr, coef=1.0):
        N, Cc, H, W = self.shape
        return dict(a=self.a.view(), b=self.b.view(), is_f32=int(self.kind == 'f32'), N=N, C=Cc, H=H, W=W, coef=coef, gcoef=0.0, loss_acc=acc_ptr)

    def launch(self, acc_ptr, stream):
        """dasr_l1_diff on `stream`, no gradient, NOT synchronised; returns the code"""
        from dasr_amd.engine import NULL_T
        k = self.kw(acc_ptr)
        return _L().dasr_l1_diff(k['a'], k['b'], k['is_f32'], k['N'], k['C'], k['H'], k['W'], k['coef'], k['gcoef'], acc_ptr, NULL_T, C.c_void_p(stream.cuda_stream))

    def inputs_untouched(self):
        return self.a.untouched() and self.b.untouched()


def acc_buf(dev, v=ACC0):
    return Buf(dev, torch.tensor([SENT, v, SENT]))


def acc_is(acc, v):
    """the accumulator word holds exactly v, its neighbours and the guards what they held"""
    assert float(v) < LIMIT and float(v) == int(v)
    return biteq(acc.get(), torch.tensor([SENT, float(v), SENT])) and acc.guards_ok()


@gpu
@VIA
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('nwg', sorted(L1_SHAPES))
def test_grid_sum_exact_at_every_loop_length(nwg, kind, via):
    dev = _gpu()
    c = L1Case(dev, nwg, kind)
    acc = acc_buf(dev)
    assert call(via, 'l1_diff', **c.kw(acc.ptr + 4)) == 0
    assert acc_is(acc, ACC0 + c.total), (float(acc.get()[1]), ACC0 + c.total)
    assert c.inputs_untouched()


@gpu
def test_grid_sum_row_growth_on_two_streams():
    """one accumulator, per stream: 2 workgroups (a first row of 4096 floats), 4113 (the row grows; the old allocation stays, the new ticket is zeroed on the launch
    stream), 2 again.  The second stream is non-blocking and gets a row of its own: its first ticket must have been zeroed on THAT stream."""
    dev = _gpu()
    small, big = L1Case(dev, 2), L1Case(dev, 4113)
    acc, want = acc_buf(dev), ACC0
    assert ACC0 + 2 * (2 * small.total + big.total) < LIMIT
    torch.cuda.synchronize()
    assert _L().dasr_red_release() == 0                            # no row left from an accumulator that lived at this address before
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    for st in (torch.cuda.current_stream(), side):
        for c in (small, big, small):
            assert c.launch(acc.ptr + 4, st) == 0
            st.synchronize()
            want += c.total
            assert want < LIMIT
            assert acc_is(acc, want), (float(acc.get()[1]), want)
    assert small.inputs_untouched() and big.inputs_untouched()


@gpu
def test_grid_sum_two_streams_add_into_one_word():
    dev = _gpu()
    ca, cb = L1Case(dev, 513, seed=0), L1Case(dev, 513, seed=1)
    assert ACC0 + ca.total + cb.total < LIMIT
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert s1.cuda_stream != s2.cuda_stream
    acc = acc_buf(dev)
    for _ in range(4):                                             # (the first round allocates the two rows; the later ones go out back to back)
        acc.put(torch.tensor([SENT, ACC0, SENT]))
        torch.cuda.synchronize()
        rc = ca.launch(acc.ptr + 4, s1), cb.launch(acc.ptr + 4, s2)   # no ordering between the two
        torch.cuda.synchronize()
        assert rc == (0, 0)
        assert acc_is(acc, ACC0 + ca.total + cb.total), (float(acc.get()[1]), ACC0 + ca.total + cb.total)


# K = 2 (dasr_gan_loss: N H W = 2 * 196 * 196 pixels -> 301 workgroups) and K = 3 (dasr_ragan stage 1: 277 * 277 pixels -> 300 workgroups): two rounds of the
# last arriver's loop; references, coefficients and bounds as tests/test_gpu_norm_gan.py takes them (oracle/norm_gan_cases.py)
GAN_HW, RAGAN_HW = (196, 196), (277, 277)


@gpu
@VIA
@pytest.mark.parametrize('gan_type', [0, 1, 2])
def test_gan_loss_accumulators_beyond_256_workgroups(gan_type, via, margins):
    dev = _gpu()
    (H, W), Cc, N, target = GAN_HW, 3, K.PIX_N, K.TARGETS[2]
    nb = (N * H * W + 255) // 256
    assert 256 < nb <= 512 and _grid_chain(nb) == _grid_chain(1) + 1
    i, _ = K.ref_gan_loss(gan_type, target, Cc, H, W)
    coef, gcoef, scoef = K.gan_coefs(Cc, H, W)
    accs = K.gan_accs(gan_type, target, Cc, H, W)
    xs = slab(dev, i['x'], pad=9.0)
    acc = Buf(dev, torch.tensor([SENT, K.ACC0['loss'], K.ACC0['score'], SENT]))
    assert call(via, 'gan_loss', x=xs.view(), N=N, C=Cc, H=H, W=W, gan_type=gan_type, target=target, coef=coef, gcoef=gcoef, score_coef=scoef,
                loss_acc=acc.ptr + 4, score_acc=acc.ptr + 8) == 0
    a = acc.get()
    tag = 'runtime K=2 %d workgroups type %d %s' % (nb, gan_type, via)
    check_acc('gan_loss loss ' + tag, a[1], accs['loss'], margins)
    check_acc('gan_loss score ' + tag, a[2], accs['score'], margins)
    assert float(a[0]) == SENT and float(a[3]) == SENT and acc.guards_ok() and xs.untouched()


RAGAN = [(f, ts[0][0], ts[0][1]) for f, ts in sorted(K.RAGAN_T.items())]


@gpu
@VIA
@pytest.mark.parametrize('form,ta,tb', RAGAN, ids=['form%d' % r[0] for r in RAGAN])
def test_ragan_accumulators_beyond_256_workgroups(form, ta, tb, via, margins):
    dev = _gpu()
    (H, W), N = RAGAN_HW, K.PIX_N
    HW, nb = H * W, (H * W + 255) // 256
    assert 256 < nb <= 512
    i, ref = K.ref_ragan(form, ta, tb, H, W)
    coef, gcoef, scoef = K.gan_coefs(1, H, W)
    accs = K.ragan_accs(form, ta, tb, H, W)
    as_, bs = slab(dev, i['a'], pad=9.0), slab(dev, i['b'], pad=-9.0, lead=2)
    sums, part = Buf(dev, n=2 * HW), Buf(dev, n=2 * HW)
    base = dict(a=as_.view(), b=bs.view(), N=N, H=H, W=W, n_glob=K.N_GLOB, form=form, ta=ta, tb=tb, coef=coef, gcoef=gcoef, eps=K.RAGAN_EPS, score_coef=scoef,
                sums=sums.ptr, part=part.ptr)
    tag = 'runtime K=3 %d workgroups form %d %s' % (nb, form, via)
    # stage 0, then the all-reduce played by the host, as test_ragan sequences it
    assert call(via, 'ragan', stage=0, **base) == 0
    s = sums.get()
    bounded('ragan sums_a ' + tag, s[:HW], ref['sums_a'].v.view(-1), ref['sums_a'].tol().view(-1), margins)
    bounded('ragan sums_b ' + tag, s[HW:], ref['sums_b'].v.view(-1), ref['sums_b'].tol().view(-1), margins)
    sums.put(torch.cat([i['sums_a'].view(-1), i['sums_b'].view(-1)]))
    acc = Buf(dev, torch.tensor([SENT, K.ACC0['loss'], SENT, K.ACC0['score'], SENT, K.ACC0['score_b'], SENT]))
    assert call(via, 'ragan', stage=1, loss_acc=acc.ptr + 4, score_a=acc.ptr + 12, score_b=acc.ptr + 20, **base) == 0
    a = acc.get()
    check_acc('ragan loss ' + tag, a[1], accs['loss'], margins)
    check_acc('ragan score_a ' + tag, a[3], accs['score_a'], margins)
    check_acc('ragan score_b ' + tag, a[5], accs['score_b'], margins)
    assert bool((a[0::2] == SENT).all()) and acc.guards_ok() and part.guards_ok() and sums.guards_ok() and as_.untouched() and bs.untouched()


@gpu
def test_red_release_frees_the_rows_and_the_next_launch_allocates_again():
    dev = _gpu()
    L = _L()
    c = L1Case(dev, 257)
    acc = acc_buf(dev)
    torch.cuda.synchronize()
    assert L.dasr_red_release() == 0                               # whatever rows the tests before this one left
    torch.cuda.synchronize()
    assert L.dasr_red_release() == 0                               # no rows at all
    torch.cuda.synchronize()
    assert L.dasr_red_release() == 0                               # twice in a row
    want = ACC0
    for _ in range(2):
        assert call('abi', 'l1_diff', **c.kw(acc.ptr + 4)) == 0    # allocates the row again
        want += c.total
        assert acc_is(acc, want)
        assert call('abi', 'l1_diff', **c.kw(acc.ptr + 4)) == 0    # uses it
        want += c.total
        assert acc_is(acc, want)
        torch.cuda.synchronize()
        assert L.dasr_red_release() == 0                           # with a live row


@gpu
def test_grid_sum_is_deterministic_over_20_launches(margins):
    """4113 workgroups on random fp32 data: twenty launches onto a zeroed accumulator leave the same bits (and the value of the fp64 sum)"""
    dev = _gpu()
    N, Cc, H, W = L1_SHAPES[4113]
    g = gen(7100)
    a, b = torch.randn(N, Cc, H, W, generator=g), torch.randn(N, Cc, H, W, generator=g)
    as_, bs = Slab(dev, 'f32', N, 1, H, W, R.pack(a)), Slab(dev, 'f32', N, 1, H, W, R.pack(b), lead=2)
    coef = _f32(1.0 / a.numel())
    loss, lmag, _, _ = R.l1_diff(a, b, coef, 0.0)
    acc, seen = acc_buf(dev, 0.0), []
    for _ in range(20):
        acc.put(torch.tensor([SENT, 0.0, SENT]))
        assert call('abi', 'l1_diff', a=as_.view(), b=bs.view(), is_f32=1, N=N, C=Cc, H=H, W=W, coef=coef, gcoef=0.0, loss_acc=acc.ptr + 4) == 0
        seen.append(acc.get())
        assert acc.guards_ok()
    assert all(biteq(s, seen[0]) for s in seen[1:]), sorted(set(float(s[1]) for s in seen))
    # a - b (1), four terms per thread (4), the grid chain less the exact add into a zero word
    Lc = 1 + 4 + _grid_chain(4113) - 1
    err, bound = abs(float(seen[0][1].double()) - loss), Lc * U32 * lmag
    margins('runtime l1_diff 4113 workgroups random data: |err| / bound %.3f (L %d)' % (err / bound, Lc))
    assert err <= bound


@gpu
def test_grid_sum_refuses_to_allocate_under_stream_capture():
    """a first use of (accumulator, stream) needs a device allocation: under capture the launcher returns DASR_ECAPTURE and launches nothing, a warmed-up
    accumulator is captured, the capture stays valid.  The graph is never replayed (the product replays none)."""
    dev = _gpu()
    L = _L()
    c = L1Case(dev, 2)
    cold, warm = acc_buf(dev), acc_buf(dev)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert L.dasr_red_release() == 0                               # `cold` has no row on any stream, whoever lived at its address before
    assert c.launch(warm.ptr + 4, side) == 0                       # eager warm-up on the capture stream
    side.synchronize()
    assert acc_is(warm, ACC0 + c.total)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                     # (no assertion inside: it would leave the capture open)
        st = torch.cuda.current_stream()
        rc_cold = c.launch(cold.ptr + 4, st)
        rc_warm = c.launch(warm.ptr + 4, st)
    assert st.cuda_stream == side.cuda_stream
    assert rc_cold == ECAPTURE and rc_warm == 0
    torch.cuda.synchronize()
    assert cold.untouched()                                        # nothing was launched
    assert acc_is(warm, ACC0 + c.total)                            # captured, not executed
    assert c.launch(cold.ptr + 4, side) == 0                       # outside the capture the first accumulator gets its row
    side.synchronize()
    assert acc_is(cold, ACC0 + c.total)
    del graph


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# B. the threaded enqueuer
FILL_KIND, ADD_KIND = 7, 26


def program(seed, nops):
    """[('fill', buf, value) | ('add', dst, src)] over the buffers 'y' and 'z'.  y is filled once and then only added to -- mostly z, which is re-filled with
    fractions of 0.25 <= |z| <= 2 all along (z += z only straight behind a fill), up to six times something that doubles it (y += y, or z += y; y += z) -- so
    every add into y shows in the end value (|y| stays below 1e6, where an fp32 step is 1/16: no z is absorbed) and the fp32 roundings make the value depend
    on the order."""
    rng = random.Random(seed)
    prog = [('fill', 'y', 1.0), ('fill', 'z', 3.0)]
    doublings = set(rng.sample(range(2, nops), min(6, (nops - 2) // 2)))

    def fill_z():
        return ('fill', 'z', _f32(rng.uniform(0.25, 2.0) * rng.choice([-1.0, 1.0])))
    while len(prog) < nops:
        u = rng.random()
        if len(prog) in doublings:
            prog.extend(rng.choice([[('add', 'y', 'y')], [('add', 'z', 'y'), ('add', 'y', 'z'), fill_z()]]))
        elif u < 0.25:
            prog.append(fill_z())
        elif u < 0.35 and prog[-1][:2] == ('fill', 'z'):
            prog.append(('add', 'z', 'z'))
        else:
            prog.append(('add', 'y', 'z'))
    return prog[:nops]


def emulate(prog):
    """the values of y and z after `prog`, in fp32 (None: never written)"""
    v = {'y': None, 'z': None}
    for o in prog:
        if o[0] == 'fill':
            v[o[1]] = torch.tensor(o[2], dtype=torch.float32)
        else:
            v[o[1]] = v[o[1]] + v[o[2]]
    return v


class Lane:
    """one op list on its own stream with its private buffers"""

    def __init__(self, dev, k, nops=None, tags=False):
        from dasr_amd import _lib
        from dasr_amd.engine import OpList
        self.k, self.n = k, 300 + 37 * k                           # more than one workgroup of the fill / add kernels, never a multiple of 256
        self.prog = program(900 + k, nops or 200 + 7 * k)
        self.buf = {'y': Buf(dev, n=self.n), 'z': Buf(dev, n=self.n)}
        self.stream = torch.cuda.Stream()
        self.ol = OpList()
        for j, o in enumerate(self.prog):
            tag = dict(tag=1 + (j + k) % 5) if tags else {}
            if o[0] == 'fill':
                self.ol.add(_lib.make_op(_lib.OP_FILL, p=self.buf[o[1]].ptr, n=self.n, value=o[2], **tag))
            else:
                self.ol.add(_lib.make_op(_lib.OP_ADD_FLAT, y=self.buf[o[1]].ptr, x=self.buf[o[2]].ptr, n=self.n, **tag))

    def poison(self):
        for b in self.buf.values():
            b.put(torch.full((self.n,), SENT))

    def spoil(self, idx, how):
        """replace op `idx` by one that fails without launching"""
        from dasr_amd import _lib
        bad = _lib.make_op(_lib.OP_FILL, p=self.buf['y'].ptr, n=0, value=1.0) if how == 'fill_n0' else _lib.make_op(99)
        self.ol.ops[idx] = bad
        self.ol._arr = None
        return bad.op

    def holds(self, upto=None, prog=None):
        """both buffers hold what the first `upto` ops (default: all; or the ops `prog`) leave, bit for bit, guards intact"""
        want = emulate(self.prog[:upto] if prog is None else prog)
        for nm, b in self.buf.items():
            w = torch.full((self.n,), SENT) if want[nm] is None else want[nm].expand(self.n)
            if not (biteq(b.get(), w) and b.guards_ok()):
                return False
        return True


def run_lanes(lanes):
    from dasr_amd import engine
    torch.cuda.synchronize()                                       # the lanes' streams are non-blocking: the poison on the default stream is in place
    engine.run_parallel([l.ol for l in lanes], [l.stream for l in lanes])
    torch.cuda.synchronize()


def test_programs_show_a_dropped_or_moved_op():
    """(CPU) the end value of y stays small enough to show every add, changes when any add into y is dropped, and when the program runs backwards"""
    for k in range(8):
        p = program(900 + k, 200 + 7 * k)
        end = emulate(p)
        assert len(p) == 200 + 7 * k and 0.0 < float(end['y'].abs()) < 1e6 and bool(torch.isfinite(end['z']))
        into_y = [j for j, o in enumerate(p) if j >= 2 and o[:2] == ('add', 'y')]
        assert len(into_y) > 100
        assert all(not torch.equal(emulate(p[:j] + p[j + 1:])['y'], end['y']) for j in into_y)
        assert not torch.equal(emulate(p[:2] + p[:1:-1])['y'], end['y'])


@gpu
@pytest.mark.parametrize('nl', [2, 4, 8])
def test_run_parallel_threaded(nl, monkeypatch):
    dev = _gpu()
    monkeypatch.delenv('DASR_ENQ', raising=False)
    lanes = [Lane(dev, k) for k in range(nl)]
    for rep in range(50 if nl == 8 else 2):                        # 50 calls: the worker pool is reused
        for l in lanes:
            l.poison()
        run_lanes(lanes)
        assert all(l.holds() for l in lanes), rep


@gpu
def test_run_parallel_chunk_interleave_gives_the_same(monkeypatch):
    dev = _gpu()
    lanes = [Lane(dev, k) for k in range(4)]
    got = {}
    for mode in ('mt', 'chunk'):
        monkeypatch.setenv('DASR_ENQ', mode)
        for l in lanes:
            l.poison()
        run_lanes(lanes)
        assert all(l.holds() for l in lanes), mode
        got[mode] = [b.get() for l in lanes for b in l.buf.values()]
    assert all(biteq(a, b) for a, b in zip(got['mt'], got['chunk']))


def _raw_mt(lanes, nlists=None, null=None):
    from dasr_amd.engine import Op
    n = len(lanes)
    for l in lanes:
        if l.ol._arr is None:
            l.ol._arr = (Op * len(l.ol.ops))(*l.ol.ops)
    args = [(C.c_void_p * n)(*[C.addressof(l.ol._arr) for l in lanes]), (C.c_int32 * n)(*[len(l.ol.ops) for l in lanes]),
            (C.c_void_p * n)(*[l.stream.cuda_stream for l in lanes])]
    if null is not None:
        args[null] = None
    L = _L()
    rc = L.dasr_run_ops_mt(*args, n if nlists is None else nlists)
    return rc, L.dasr_last_failed_op()


@gpu
def test_run_ops_mt_argument_checks_launch_nothing():
    dev = _gpu()
    lanes = [Lane(dev, k, nops=12) for k in range(2)]
    torch.cuda.synchronize()
    for kw in (dict(nlists=0), dict(nlists=9), dict(nlists=-1), dict(null=0), dict(null=1), dict(null=2)):
        assert _raw_mt(lanes, **kw)[0] == EINVAL, kw
    torch.cuda.synchronize()
    assert all(b.untouched() for l in lanes for b in l.buf.values())
    assert _raw_mt(lanes)[0] == 0                                  # the same arrays are a good call
    torch.cuda.synchronize()
    assert all(l.holds() for l in lanes)


FAILS = [  # id, {list: index of its failing op}, the list and op reported
    ('list2_op5', {2: 5}, 2, 5),
    ('list0_op7', {0: 7}, 0, 7),
    ('list0_and_list3', {0: 7, 3: 3}, 0, 7),
    ('list1_and_list3', {1: 9, 3: 3}, 1, 9),                       # the lowest failing list is the one reported
]


@gpu
@pytest.mark.parametrize('how', ['fill_n0', 'unknown_kind'])
@pytest.mark.parametrize('case', FAILS, ids=[f[0] for f in FAILS])
def test_run_ops_mt_failure_report(case, how, monkeypatch):
    from dasr_amd import _lib, engine
    dev = _gpu()
    monkeypatch.delenv('DASR_ENQ', raising=False)
    _, bad, li, oi = case
    lanes = [Lane(dev, k, nops=40 + k) for k in range(4)]
    kinds = {k: lanes[k].spoil(idx, how) for k, idx in bad.items()}

    def check_buffers():
        torch.cuda.synchronize()
        # a failing list stops at its bad op; every other list has been enqueued completely
        assert all(l.holds(bad.get(l.k)) for l in lanes)

    for l in lanes:
        l.poison()
    torch.cuda.synchronize()
    rc, k = _raw_mt(lanes)
    assert rc == EINVAL and k == (oi | (li << 24)), (rc, hex(k))
    if li == 0:
        assert k >> 24 == 0                                        # list 0: the index carries no list bits
    check_buffers()
    for l in lanes:
        l.poison()
    torch.cuda.synchronize()
    with pytest.raises(_lib.DasrHipError) as e:
        engine.run_parallel([l.ol for l in lanes], [l.stream for l in lanes])
    msg = str(e.value)
    assert 'list %d op #%d (kind %d) failed with code %d' % (li, oi, kinds[li], EINVAL) in msg, msg
    check_buffers()
    # the pool survives: the next good call succeeds
    good = [Lane(dev, k, nops=40 + k) for k in range(4)]
    for l in good:
        l.poison()
    run_lanes(good)
    assert all(l.holds() for l in good)


@gpu
@pytest.mark.parametrize('how', ['fill_n0', 'unknown_kind'])
def test_oplist_run_reports_the_index_in_the_whole_list(how):
    from dasr_amd import _lib
    dev = _gpu()
    lane = Lane(dev, 0, nops=6)
    kind = lane.spoil(4, how)
    lane.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(lane.stream):
        lane.ol.run(0, 4)
        torch.cuda.synchronize()
        assert lane.holds(4)
        with pytest.raises(_lib.DasrHipError) as e:
            lane.ol.run(2)
        assert 'op #4 (kind %d) failed with code %d' % (kind, EINVAL) in str(e.value), str(e.value)
        with pytest.raises(_lib.DasrHipError) as e:
            lane.ol.run(4, 6)
        assert 'op #4 ' in str(e.value)
        lane.ol.run(5)                                             # behind the bad op
        lane.ol.run(3, 3)                                          # empty ranges: nothing to do
        lane.ol.run(6)
    torch.cuda.synchronize()
    p = lane.prog
    assert lane.holds(prog=p[:4] + p[2:4] + p[5:])                 # run(0, 4); ops 2 and 3 of the failed run(2); op 5


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# C. scheduling ops.  A consumer reads a value whose producer sits behind dasr_probe_spin on another stream
def _bench():
    from dasr_amd import _lib
    try:
        return _lib.bench_lib()
    except _lib.DasrHipError as e:
        pytest.skip(str(e))


def _spin(stream, micros):
    from dasr_amd import _lib
    _lib.check(_bench().dasr_probe_spin(1, micros, C.c_void_p(stream.cuda_stream)), 'spin')


def _oplist(*ops):
    from dasr_amd.engine import OpList
    ol = OpList()
    for o in ops:
        ol.add(o)
    return ol


class Sched:
    """three flat buffers (y, w, z), two non-blocking streams and an event"""

    def __init__(self, dev):
        self.n = 300
        self.y, self.w, self.z = (Buf(dev, torch.full((self.n,), v)) for v in (1.0, 2.0, 100.0))
        self.sa, self.sb = torch.cuda.Stream(), torch.cuda.Stream()
        assert self.sa.cuda_stream != self.sb.cuda_stream
        self.ev = _L().dasr_event_create()
        assert self.ev
        torch.cuda.synchronize()

    def close(self):
        torch.cuda.synchronize()
        assert _L().dasr_event_destroy(self.ev) == 0

    def fill(self, b, v):
        from dasr_amd import _lib
        return _lib.make_op(_lib.OP_FILL, p=b.ptr, n=self.n, value=v)

    def add(self, dst, src):
        from dasr_amd import _lib
        return _lib.make_op(_lib.OP_ADD_FLAT, y=dst.ptr, x=src.ptr, n=self.n)

    def record(self):
        from dasr_amd import _lib
        return _lib.make_op(_lib.OP_EVENT_RECORD, event=self.ev)

    def wait(self):
        from dasr_amd import _lib
        return _lib.make_op(_lib.OP_STREAM_WAIT, event=self.ev)

    def redirect(self, stream):
        from dasr_amd import _lib
        return _lib.make_op(_lib.OP_SET_STREAM, stream=stream.cuda_stream if stream is not None else None)

    def z_is(self, v):
        return biteq(self.z.get(), torch.full((self.n,), v)) and all(b.guards_ok() for b in (self.y, self.w, self.z))


@gpu
def test_event_record_and_stream_wait_order_two_streams(margins):
    dev = _gpu()
    _bench()
    s = Sched(dev)
    try:
        with torch.cuda.stream(s.sa):
            _spin(s.sa, 20000)                                     # y's producer sits behind 20 ms
            _oplist(s.fill(s.y, 5.0), s.record()).run()
        with torch.cuda.stream(s.sb):                              # a LATER call, as dasr_hip.h requires of a wait for another list's event
            _oplist(s.wait(), s.add(s.z, s.y)).run()
        torch.cuda.synchronize()
        assert s.z_is(105.0), float(s.z.get()[0])
        # what the same consumer reads WITHOUT the wait: logged, not asserted (two streams that share a hardware queue are ordered anyway)
        s.y.put(torch.full((s.n,), 1.0))
        s.z.put(torch.full((s.n,), 100.0))
        torch.cuda.synchronize()
        with torch.cuda.stream(s.sa):
            _spin(s.sa, 20000)
            _oplist(s.fill(s.y, 5.0)).run()
        with torch.cuda.stream(s.sb):
            _oplist(s.add(s.z, s.y)).run()
        torch.cuda.synchronize()
        margins('runtime stream wait: without the wait the consumer read y = %g (the old value is 1, the produced one 5)' % (float(s.z.get()[0]) - 100.0))
    finally:
        s.close()


def _redirect_case(dev, split):
    """The lists run on stream A and redirect to stream B.
    Phase 1, the redirect takes effect: B is busy for 20 ms and then sets w = 3; the list is [redirect to B, w += w, record ev | close, wait ev, z += w].  On B
    the add follows w = 3 (w = 6, z = 106); on A it would run at once on the old w = 2, and B's fill would leave w = 3.
    Phase 2, the redirect ends: A is busy for 20 ms and then sets y = 5; the list is [redirect to B, w = 1 | close, z += y].  Back on A the add follows y = 5
    (z = 111); still on B it would run at once on the old y = 1.
    split: each list is two dasr_run_ops calls cut at `|` with no closing op -- the first call ends with its redirect open, which must not leak into the second."""
    _bench()
    s = Sched(dev)
    try:
        for busy, producer, head, tail in (
                (s.sb, s.fill(s.w, 3.0), [s.redirect(s.sb), s.add(s.w, s.w), s.record()], [s.wait(), s.add(s.z, s.w)]),
                (s.sa, s.fill(s.y, 5.0), [s.redirect(s.sb), s.fill(s.w, 1.0)], [s.add(s.z, s.y)])):
            with torch.cuda.stream(busy):
                _spin(busy, 20000)
                _oplist(producer).run()
            with torch.cuda.stream(s.sa):
                if split:
                    _oplist(*head).run()
                    _oplist(*tail).run()
                else:
                    _oplist(*(head + [s.redirect(None)] + tail)).run()
            torch.cuda.synchronize()
            if busy is s.sb:
                assert biteq(s.w.get(), torch.full((s.n,), 6.0)), float(s.w.get()[0])
                assert s.z_is(106.0), float(s.z.get()[0])
        assert biteq(s.w.get(), torch.full((s.n,), 1.0)) and biteq(s.y.get(), torch.full((s.n,), 5.0))
        assert s.z_is(111.0), float(s.z.get()[0])
    finally:
        s.close()


@gpu
def test_set_stream_redirects_and_a_null_stream_closes_the_redirect():
    _redirect_case(_gpu(), split=False)


@gpu
def test_set_stream_left_open_does_not_leak_into_the_next_call():
    _redirect_case(_gpu(), split=True)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# D. profiling session
Rec = collections.namedtuple('Rec', 'tag us flops bytes op')


def session(fn, capacity=16, max_out=None, mid=None):
    """fn() inside a profiling session -> (records, host wall time of the session in us).  The session is closed and the filter reset whatever happens."""
    L = _L()
    room = max(capacity, 64)                                       # (more room than capacity: what limits the records is the session, not the output arrays)
    us, fl, by = (C.c_float * room)(), (C.c_double * room)(), (C.c_double * room)()
    op, tg = (C.c_int32 * room)(), (C.c_char_p * room)()
    torch.cuda.synchronize()
    rc = L.dasr_prof_begin(capacity)
    assert rc == 0, rc
    n = None
    try:
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e6
        if mid is not None:
            mid()
    finally:
        n = L.dasr_prof_end(room if max_out is None else max_out, us, fl, by, op, tg)
    assert n >= 0, n
    return [Rec(tg[i].decode(), us[i], fl[i], by[i], op[i]) for i in range(n)], wall


@pytest.fixture
def prof():
    """the library handle; afterwards no session is open and no filter is set, however the test ended"""
    _gpu()
    L = _L()
    yield L
    torch.cuda.synchronize()
    d = (C.c_double * 1)()
    L.dasr_prof_end(0, (C.c_float * 1)(), d, d, (C.c_int32 * 1)(), (C.c_char_p * 1)())
    assert L.dasr_prof_filter(None) == 0


class ThreeOps:
    """fill (tag 5, 1e6 flops, 2e6 bytes), add_flat (tag 7), prelu_grad (3e6 flops, two launches)"""
    TAGS = ['fill_kernel', 'add_flat_kernel', 'prelu_grad_partial_kernel<float>', 'prelu_grad_final_kernel']
    PRELU_KIND = 24
    OPS = [FILL_KIND | (5 << 8), ADD_KIND | (7 << 8), PRELU_KIND, PRELU_KIND]

    def __init__(self, dev):
        from dasr_amd import _lib
        N, Cc, H, W = 2, 20, 5, 7
        g = gen(7200)
        self.n = 300
        self.y, self.x = Buf(dev, n=self.n), Buf(dev, torch.full((self.n,), 2.0))
        self.ys = Slab(dev, 'f32', N, 2, H, W, R.pack(torch.randn(N, Cc, H, W, generator=g)))
        self.gs = Slab(dev, 'f32', N, 2, H, W, R.pack(torch.randn(N, Cc, H, W, generator=g)), lead=2)
        self.slope, self.scratch, self.dst = Buf(dev, torch.tensor([0.25])), Buf(dev, n=1024), Buf(dev, n=1)
        self.ol = _oplist(
            _lib.make_op(_lib.OP_FILL, flops=1e6, bytes=2e6, p=self.y.ptr, n=self.n, value=1.5, tag=5),
            _lib.make_op(_lib.OP_ADD_FLAT, y=self.y.ptr, x=self.x.ptr, n=self.n, tag=7),
            _lib.make_op(_lib.OP_PRELU_GRAD, flops=3e6, y=self.ys.view(), gx=self.gs.view(), N=N, C=Cc, H=H, W=W, slope=self.slope.ptr,
                         scratch256=self.scratch.ptr, dst=self.dst.ptr, scale=1.0))
        assert _lib.OP_FILL == FILL_KIND and _lib.OP_ADD_FLAT == ADD_KIND and _lib.OP_PRELU_GRAD == self.PRELU_KIND

    def check(self, recs, wall, first=0, count=4):
        assert [r.tag for r in recs] == self.TAGS[first:first + count], [r.tag for r in recs]
        assert [r.op for r in recs] == self.OPS[first:first + count], [hex(r.op) for r in recs]
        # an op's flops / bytes sit on its first launch
        assert [r.flops for r in recs] == [1e6, 0.0, 3e6, 0.0][first:first + count]
        assert [r.bytes for r in recs] == [2e6, 0.0, 0.0, 0.0][first:first + count]
        assert all(0.0 < r.us < wall for r in recs), ([r.us for r in recs], wall)
        assert biteq(self.y.get(), torch.full((self.n,), 3.5))      # (the session ran the ops, not only recorded them)


@gpu
def test_prof_records_in_issue_order(prof):
    t = ThreeOps(_gpu())
    recs, wall = session(t.ol.run)
    t.check(recs, wall)
    recs, wall = session(t.ol.run)                                 # a second session starts at record 0 again
    t.check(recs, wall)


@gpu
def test_prof_limits(prof):
    t = ThreeOps(_gpu())
    t.check(*session(t.ol.run, capacity=16))                       # (a larger session first: a later, smaller capacity still holds)
    recs, wall = session(t.ol.run, capacity=2)
    t.check(recs, wall, count=2)
    recs, wall = session(t.ol.run, capacity=16, max_out=1)
    t.check(recs, wall, count=1)
    assert prof.dasr_prof_begin(0) == EINVAL and prof.dasr_prof_begin(-1) == EINVAL
    assert session(lambda: None)[0] == []                          # (the refused begin opened nothing and recorded nothing)
    t.ol.run()                                                     # no session open: no records ...
    torch.cuda.synchronize()
    assert session(lambda: None)[0] == []                          # ... and the next session starts at 0
    t.check(*session(t.ol.run))


@gpu
def test_prof_filter(prof):
    t = ThreeOps(_gpu())
    assert prof.dasr_prof_filter(b'add_flat') == 0
    recs, wall = session(t.ol.run)
    t.check(recs, wall, first=1, count=1)
    assert prof.dasr_prof_filter(b'prelu_grad') == 0               # a family: both launches of the op, the op's flops on the first
    recs, wall = session(t.ol.run)
    t.check(recs, wall, first=2, count=2)
    for none in (None, b''):
        assert prof.dasr_prof_filter(b'no kernel has this name') == 0
        assert session(t.ol.run)[0] == []
        assert prof.dasr_prof_filter(none) == 0
        t.check(*session(t.ol.run))
    assert prof.dasr_prof_filter(b'f' * 128) == EINVAL and prof.dasr_prof_filter(b'f' * 4000) == EINVAL
    t.check(*session(t.ol.run))                                    # a refused filter changes nothing
    assert prof.dasr_prof_filter(b'f' * 127) == 0
    assert session(t.ol.run)[0] == []
    assert prof.dasr_prof_filter(None) == 0
    # while a session is open: refused, the session's records stay
    rcs = []
    recs, wall = session(t.ol.run, mid=lambda: rcs.extend([prof.dasr_prof_filter(b'add_flat'), prof.dasr_prof_filter(None)]))
    assert rcs == [EINVAL, EINVAL]
    t.check(recs, wall)
    t.check(*session(t.ol.run))                                    # and no filter was left behind


@gpu
def test_prof_session_around_the_threaded_enqueue(prof, monkeypatch):
    dev = _gpu()
    monkeypatch.delenv('DASR_ENQ', raising=False)
    lanes = [Lane(dev, k, tags=True) for k in range(4)]
    for l in lanes:
        l.poison()
    total = sum(len(l.ol.ops) for l in lanes)                      # one launch per op
    recs, wall = session(lambda: run_lanes(lanes), capacity=1024)
    assert total < 1024 and len(recs) == total
    assert all(l.holds() for l in lanes)
    want = collections.Counter(o.op | (o.get('tag') << 8) for l in lanes for o in l.ol.ops)
    assert collections.Counter(r.op for r in recs) == want         # per op kind the right tags, each the right number of times; the order across lists is free
    assert all(r.tag == {FILL_KIND: 'fill_kernel', ADD_KIND: 'add_flat_kernel'}[r.op & 0xff] for r in recs)
    assert all(r.flops == 0.0 and r.bytes == 0.0 and r.us > 0.0 for r in recs)


@gpu
@pytest.mark.parametrize('ending', ['success', 'failure'])
def test_prof_launch_outside_any_op_records_kind_0_bucket_0_no_flops(ending, prof):
    """dasr_run_ops leaves nothing of its last op behind: a launch through a plain entry point (dasr_adam, the fill of the loss accumulator, the add of the
    replica gradients) is recorded with kind 0, bucket 0 and no work, not with the kind, the bucket and the unconsumed flops of the last op dispatched"""
    from dasr_amd import _lib
    from dasr_amd.engine import _stream
    dev = _gpu()
    n = 300
    y, x, w = Buf(dev, n=n), Buf(dev, torch.full((n,), 2.0)), Buf(dev, torch.full((n,), 2.0))
    ops = [_lib.make_op(_lib.OP_ADD_FLAT, y=x.ptr, x=w.ptr, n=n, tag=3),
           _lib.make_op(_lib.OP_FILL, flops=1e6, bytes=2e6, p=y.ptr, n=n if ending == 'success' else 0, value=1.0, tag=9)]
    ol = _oplist(*ops)
    if ending == 'success':                                        # no session open: the fill's launch consumes nothing
        ol.run()
    else:                                                          # the last op dispatched fails before it launches
        with pytest.raises(_lib.DasrHipError):
            ol.run()
        y.put(torch.full((n,), 1.0))
    torch.cuda.synchronize()
    recs, wall = session(lambda: _lib.check(prof.dasr_add_flat(y.ptr, x.ptr, n, _stream()), 'add_flat'))
    assert len(recs) == 1 and recs[0].tag == 'add_flat_kernel'
    assert (recs[0].op, recs[0].flops, recs[0].bytes) == (0, 0.0, 0.0), recs[0]
    assert 0.0 < recs[0].us < wall
    assert biteq(y.get(), torch.full((n,), 5.0)) and y.guards_ok()
