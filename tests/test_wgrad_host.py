"""CPU tests of the weight-gradient planning (engine.WgradGroup / WgradGroup3 / Workspace, rrdbnet.rdb_wgrad_parts / TrunkStore): the part and reduce
descriptors the planners upload are decoded from their byte images and checked against Python copies of what csrc/wgrad.hip does with them --
the workgroup -> (part, split) map, the workspace floats every part writes and every reduce part reads, the gradient floats every reduce part
writes, and the few-splits reduce grid.  No GPU: the planners run with device='cpu' (or 'meta' where only the launch geometry is needed)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dasr_amd import _lib
from dasr_amd import rrdbnet
from dasr_amd.engine import BTensor, OpList, ParamStore, WgradGroup, WgradGroup3, Workspace, ceil_div

W3_SPLIT, W3_TAP, W3_BIAS = 9 * 3 * 2048, 3 * 2048, 96   # wgrad3_ld_kernel workspace strides (floats)


def decode(grp):
    """(parts, reduce parts) of a finalized group, decoded from the byte images it uploaded"""
    def arr(t, cls):
        raw = bytes(t.cpu().numpy().tobytes())
        assert len(raw) % C.sizeof(cls) == 0
        return list((cls * (len(raw) // C.sizeof(cls))).from_buffer_copy(raw))
    return arr(grp.w_dev, _lib.WgradPart), arr(grp.r_dev, _lib.WgradReducePart)


def w3_block_map(nsplit_flags, b):
    """Python copy of w3_block_map (csrc/wgrad.hip) on an array of workgroup ids b: (part_id, split)"""
    nsplit, ppu = nsplit_flags & 0xffff, (nsplit_flags >> 16) & 0xff
    if ppu == 0:
        return b // nsplit, b % nsplit
    xcd, slot = b & 7, b >> 3
    su, pin = slot // ppu, slot % ppu
    unit = su * 8 + xcd
    return (unit // nsplit) * ppu + pin, unit % nsplit


def assert_block_map_is_bijection(nparts, nsplit_flags):
    nsplit = nsplit_flags & 0xffff
    b = np.arange(nparts * nsplit, dtype=np.int64)
    part, split = w3_block_map(nsplit_flags, b)
    assert part.min() >= 0 and part.max() < nparts and split.min() >= 0 and split.max() < nsplit, (nparts, nsplit_flags)
    seen = np.zeros(nparts * nsplit, dtype=np.int64)
    np.add.at(seen, part * nsplit + split, 1)
    assert (seen == 1).all(), (nparts, nsplit_flags)


def _grid(*axes):
    """flattened sum of the outer sum of the index axes"""
    out = np.zeros(1, dtype=np.int64)
    for a in axes:
        out = np.add.outer(out, np.asarray(a, dtype=np.int64)).ravel()
    return out


def ws_writes(kind, wp, nsplit, tpp=None):
    """workspace floats a wgrad part writes over all its splits (idle splits write their zero partials too): kind 3 = wgrad3_ld_kernel, 4 = the 4-wave
    wgrad_kernel (tpp taps per part).  Returns (weight partial indices, bias partial indices)."""
    s = np.arange(nsplit)
    if kind == 3:
        n_ot = (wp.g_planes + 1) >> 1
        w = _grid([wp.ws_off], s * W3_SPLIT, np.arange(9) * W3_TAP, np.arange(n_ot) * 2048, np.arange(32) * 64, np.arange(32 * wp.n_ctiles))
        b = _grid([wp.ws_bias_off], s * W3_BIAS, np.arange(n_ot) * 32, np.arange(32)) if wp.want_bias else np.zeros(0, np.int64)
    else:
        ntl = min(tpp, wp.kh * wp.kh - wp.tap0)
        w = _grid([wp.ws_off], s * tpp * 2048, np.arange(ntl) * 2048, np.arange(32) * 64, np.arange(32 * wp.n_ctiles))
        b = _grid([wp.ws_bias_off], s * 32, np.arange(32)) if wp.want_bias else np.zeros(0, np.int64)
    return w, b


def reduce_io(rp, few_splits):
    """Python copy of wgrad_reduce_kernel's addressing for one reduce part: (workspace floats read, gradient floats written)"""
    NT = rp.ntaps_total if rp.ntaps_total > 0 else rp.ntaps
    ntaps = min(rp.ntaps, NT - rp.tap0)
    sstride = rp.split_stride if rp.split_stride > 0 else rp.ntaps * 2048
    tstride = rp.tap_stride if rp.tap_stride > 0 else 2048
    bstride = rp.bias_stride if rp.bias_stride > 0 else 32
    n_all = min(32 * rp.n_ctiles, rp.cin - rp.c0, 64)
    # a few-splits grid (one workgroup per oc) runs the general path for a part outside its limits with channel group 0 only
    if few_splits and not (rp.nsplit <= 4 and ntaps <= 16):
        n_all = min(n_all, 16)
    ocs = np.arange(32)
    ocs = ocs[rp.oc0 + ocs < rp.cout]
    reads = _grid([rp.ws_off], np.arange(rp.nsplit) * sstride, np.arange(ntaps) * tstride, ocs * 64, np.arange(n_all))
    writes = _grid([rp.dst_w_off], (rp.oc0 + ocs) * rp.cin * NT, (rp.c0 + np.arange(n_all)) * NT, rp.tap0 + np.arange(ntaps))
    if rp.dst_b_off >= 0:
        nb_ = rp.bias_nsplit if rp.bias_nsplit > 0 else rp.nsplit
        reads = np.concatenate([reads, _grid([rp.ws_bias_off], np.arange(nb_) * bstride, ocs)])
        writes = np.concatenate([writes, rp.dst_b_off + rp.oc0 + ocs])
    return reads, writes


def check_group(kind, grp, ops, P, owned, tpp=None):
    """the whole contract of one finalized group: parts write disjoint workspace ranges inside ws_floats, the reduce reads only floats some part wrote,
    writes every element of the `owned` parameters exactly once and nothing else, and few_splits is set exactly when the kernel allows it"""
    parts, reds = decode(grp)
    wop, rop = ops
    assert wop.get('nparts') == len(parts) and rop.get('nparts') == len(reds)
    nsplit = wop.get('nsplit') & 0xffff
    assert nsplit == grp.nsplit
    written = np.zeros(grp.ws_floats, dtype=np.int8)
    for wp in parts:
        for idx in ws_writes(kind, wp, nsplit, tpp):
            assert idx.size == 0 or (idx.min() >= 0 and idx.max() < grp.ws_floats)
            assert (written[idx] == 0).all(), 'two parts write the same workspace float'
            written[idx] = 1
    few = rop.get('few_splits')
    allowed = all(rp.nsplit <= 4 and min(rp.ntaps, (rp.ntaps_total or rp.ntaps) - rp.tap0) <= 16 for rp in reds)
    assert few == int(allowed)
    hits = np.zeros(P.total, dtype=np.int64)
    for rp in reds:
        rd, wr = reduce_io(rp, few)
        assert (written[rd] == 1).all(), 'the reduce reads workspace floats no part writes'
        np.add.at(hits, wr, 1)
    want = np.zeros(P.total, dtype=np.int64)
    for k in owned:
        o, _, n = P.spec[k]
        want[o:o + n] = 1
    bad = np.nonzero(hits != want)[0]
    assert bad.size == 0, 'reduce coverage: %d floats written %s times (first at %d), want %s' % (bad.size, hits[bad[:4]], bad[0], want[bad[:4]])


def _bt(N, C_, H, W, dev='cpu', f32=False, f16=False):
    return BTensor(N, C_, H, W, f32, dev, f16=f16)


def _finish(grp, ws, P, scale=1.0):
    ops = grp.ops(P.grad.data_ptr(), scale=scale)
    ws.finalize()
    return ops


def _rdb_group(nf, n_rdb, N, h, w, dev='cpu'):
    nb = ceil_div(n_rdb, 3)
    P = ParamStore(rrdbnet.rrdbnet_param_spec(3, 3, nf, nb), dev)
    sc = nf + 4 * rrdbnet.GC
    ws, grp, owned, ppu = Workspace(dev), WgradGroup3(), [], 0
    for r in range(n_rdb):
        pre = 'model.1.sub.%d.RDB%d.conv' % (r // 3, r % 3 + 1)
        ppu, _ = rrdbnet.rdb_wgrad_parts(grp, nf, pre, P, _bt(N, sc, h, w, dev), _bt(N, sc, h, w, dev), h, w, N)
        owned += ['%s%d.0.%s' % (pre, j, t) for j in range(1, 6) for t in ('weight', 'bias')]
    return P, ws, grp, owned, ppu


@pytest.mark.parametrize('nf,n_rdb,N,hw', [(64, 12, 1, (12, 20)), (64, 3, 2, (24, 40)), (32, 6, 1, (12, 20)), (32, 3, 3, (12, 20)), (64, 1, 1, (5, 7))])
def test_dense_block_group_layout_and_reduce_coverage(nf, n_rdb, N, hw):
    """the grouped dense-block weight gradient (rdb_wgrad_parts into one WgradGroup3): every conv weight and bias of every RDB written exactly once"""
    h, w = hw
    P, ws, grp, owned, ppu = _rdb_group(nf, n_rdb, N, h, w)
    grp.finalize(ws, 'cpu', target_wgs=256, ppu=ppu)
    ops = _finish(grp, ws, P)
    assert_block_map_is_bijection(len(grp.parts), ops[0].get('nsplit'))
    check_group(3, grp, ops, P, owned)


@pytest.mark.parametrize('cin,cout,Hout,Wout,ups,N', [(64, 3, 96, 160, 0, 1), (64, 64, 48, 80, 1, 2), (64, 256, 24, 40, 0, 1), (32, 48, 7, 15, 0, 3),
                                                      (192, 160, 9, 17, 0, 1)])
def test_tail_conv_layout_and_reduce_coverage(cin, cout, Hout, Wout, ups, N):
    """an HR-tail conv built by _Plan._wg3 (f16 tensors, odd plane counts, pixel-shuffle widths, nearest-x2 input)"""
    P = ParamStore([('pre', (5,)), ('c.weight', (cout, cin, 3, 3)), ('c.bias', (cout,)), ('post', (7,))], 'cpu')
    Hin, Win = (Hout // 2, Wout // 2) if ups else (Hout, Wout)
    plan = SimpleNamespace(net=SimpleNamespace(params=P, device='cpu'), N=N, ws=Workspace('cpu'), grad=P.grad, gscale=1024.0,
                           _wg3_target=lambda n: 256)
    ops = OpList()
    rrdbnet._Plan._wg3(plan, ops, 'c.', _bt(N, cout, Hout, Wout, f16=True), _bt(N, cin, Hin, Win, f16=True), cout, cin, Hin, Win, Hout, Wout, ups=ups)
    grp = ops.keep[-1]
    plan.ws.finalize()
    assert ops.ops[0].get('kh') == 33 and ops.ops[0].get('f32') == 2 and ops.ops[1].get('inv_prescale') == 1.0 / 1024
    assert_block_map_is_bijection(len(grp.parts), ops.ops[0].get('nsplit'))
    check_group(3, grp, ops.ops, P, ['c.weight', 'c.bias'])


@pytest.mark.parametrize('kh,stride,cin,cout,H,W,N,target,split,pairs', [
    (3, 1, 96, 32, 24, 40, 2, 24, False, 1), (3, 1, 48, 40, 11, 19, 1, 768, False, 1), (5, 1, 64, 40, 13, 21, 2, 768, False, 1),
    (5, 1, 3, 64, 19, 33, 1, 6, False, 1), (1, 1, 256, 1, 13, 17, 2, 768, False, 1), (3, 2, 64, 48, 24, 40, 2, 768, False, 1),
    (4, 2, 16, 64, 32, 40, 2, 768, True, 1), (4, 1, 64, 32, 15, 18, 1, 4, True, 1), (3, 1, 32, 64, 64, 128, 4, 768, False, 1),
    (3, 1, 64, 33, 10, 20, 2, 768, False, 3), (4, 2, 64, 128, 16, 16, 1, 768, True, 2)])
def test_four_wave_group_layout_and_reduce_coverage(kh, stride, cin, cout, H, W, N, target, split, pairs):
    """WgradGroup (the 4-wave kernel): 5x5 tap split, 1x1, stride 2, split operands (three variants of a part), more_pairs, > 128 splits"""
    pad = (kh - 1) // 2 if stride == 1 else 1
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kh) // stride + 1
    P = ParamStore([('pre', (3,)), ('c.weight', (cout, cin, kh, kh)), ('c.bias', (cout,)), ('post', (2,))], 'cpu')
    g, x = _bt(N, cout, Ho, Wo, f32=True), _bt(N, cin, H, W, f32=True)
    lo = (_bt(N, cout, Ho, Wo, f32=True).view, _bt(N, cin, H, W, f32=True).view) if split else None
    more = [(_bt(N, cout, Ho, Wo, f32=True).view, _bt(N, cin, H, W, f32=True).view) for _ in range(pairs - 1)]
    ws, grp = Workspace('cpu'), WgradGroup(kh, stride)
    grp.add_conv(g.view, True, g.planes, x.view, True, x.planes, cout, cin, H, W, Ho, Wo, N, P.off('c.weight'), P.off('c.bias'), pad=pad,
                 f16=split, g_scale=4096.0 if split else 0.0, split=lo, more_pairs=more)
    grp.finalize(ws, 'cpu', target_wgs=target)
    ops = _finish(grp, ws, P, scale=0.5)
    parts, reds = decode(grp)
    nvar = (3 if split else 1) + len(more)
    assert len(parts) == nvar * len(reds)
    assert all(rp.nsplit == nvar * grp.nsplit and rp.bias_nsplit == (grp.nsplit if nvar > 1 else 0) for rp in reds)
    assert sum(wp.want_bias for wp in parts) == ceil_div(cout, 32)   # the first variant of each oc tile's first part only
    if kh == 3 and cin == 32 and H == 64:
        assert grp.nsplit > 128   # the reduce's outer split loop
    check_group(4, grp, ops, P, ['c.weight', 'c.bias'], tpp=grp.tpp)


def test_few_splits_checker_sees_a_skipped_channel_group():
    """the reduce-coverage emulation notices what a few-splits grid does to a part outside its limits (channel groups 1-3 never written)"""
    P = ParamStore([('c.weight', (32, 64, 3, 3)), ('c.bias', (32,))], 'cpu')
    g, x = _bt(1, 32, 64, 64, f32=True), _bt(1, 64, 64, 64, f32=True)
    ws, grp = Workspace('cpu'), WgradGroup(3, 1)
    grp.add_conv(g.view, True, g.planes, x.view, True, x.planes, 32, 64, 64, 64, 64, 64, 1, P.off('c.weight'), P.off('c.bias'))
    grp.finalize(ws, 'cpu', target_wgs=2)
    ops = _finish(grp, ws, P)
    assert grp.nsplit == 2 and ops[1].get('few_splits') == 1
    check_group(4, grp, ops, P, ['c.weight', 'c.bias'], tpp=grp.tpp)
    grp.finalize(Workspace('cpu'), 'cpu', target_wgs=16)   # 16 splits: the general grid
    ops2 = grp.ops(P.grad.data_ptr())
    assert ops2[1].get('few_splits') == 0
    ops2[1].set('few_splits', 1)
    with pytest.raises(AssertionError):
        check_group(4, grp, ops2, P, ['c.weight', 'c.bias'], tpp=grp.tpp)


@pytest.mark.parametrize('nf', [32, 64])
def test_trunk_grouping_block_map_is_a_bijection(nf):
    """every grouped launch TrunkStore records, for nb 1..23 and several batch / crop sizes: w3_block_map covers (part, split) exactly once, the host's ppu
    is one the kernel accepts, and few_splits is set exactly when every reduce part has <= 4 splits"""
    seen_ppu = set()
    for nb in range(1, 24):
        for N in (1, 2, 8, 16):
            for h, w in ((8, 16), (12, 20), (24, 40), (5, 7)):
                net = SimpleNamespace(device=torch.device('meta'), nf=nf, nb=nb, rdb_f16=(N % 2 == 0),
                                      params=ParamStore(rrdbnet.rrdbnet_param_spec(3, 3, nf, nb), 'meta'))
                st = rrdbnet.TrunkStore(net, N, h, w)
                ops = st.phase.ops
                assert len(ops) == 2 * len(st.groups)
                for grp in st.phase.keep:
                    wop, rop = ops[2 * st.phase.keep.index(grp)], ops[2 * st.phase.keep.index(grp) + 1]
                    assert wop.op == _lib.OP_WGRAD and rop.op == _lib.OP_WGRAD_REDUCE
                    nparts, flags = wop.get('nparts'), wop.get('nsplit')
                    ns, ppu = flags & 0xffff, (flags >> 16) & 0xff
                    assert (ns, ppu, nparts) == (grp.nsplit, grp.ppu, len(grp.parts)) and flags >> 24 == 0
                    assert ns <= N * ceil_div(h, 8) * ceil_div(w, 16)
                    if ppu:   # the conditions dasr_wgrad checks before it launches
                        assert nparts % ppu == 0 and (nparts // ppu * ns) % 8 == 0 and ns % 8
                    assert rop.get('few_splits') == int(ns <= 4)
                    assert_block_map_is_bijection(nparts, flags)
                    seen_ppu.add(ppu > 0)
                    assert wop.get('f32') == (2 if net.rdb_f16 else 0)
    assert seen_ppu == {True, False}


def test_block_map_copy_matches_the_kernel_source():
    """the Python w3_block_map above is a line-by-line copy: the kernel's body must still be the one it copies"""
    import os
    src = open(os.path.join(os.path.dirname(rrdbnet.__file__), 'csrc', 'wgrad.hip')).read()
    body = src[src.index('void w3_block_map('):]
    body = body[:body.index('\n}\n')]
    for line in ('const int xcd = b & 7, slot = b >> 3;', 'const int su = slot / ppu, pin = slot - su * ppu;', 'const int unit = su * 8 + xcd;',
                 'const int rdb = unit / nsplit;', 'split = unit - rdb * nsplit;', 'part_id = rdb * ppu + pin;', 'part_id = b / nsplit;'):
        assert line in body, line
