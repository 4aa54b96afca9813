"""CPU tests of the host side of the op runtime: OpList.safe_cuts (dasr_amd/engine.py), which decides where run_interleaved may cut a list, and the
argument checks of dasr_run_ops_mt / dasr_prof_begin / dasr_prof_filter (csrc/misc.hip) that return before any HIP call.  The GPU side of the same
code is tests/test_gpu_runtime.py.

safe_cuts is held to a brute-force statement of its contract: dasr_run_ops forgets an OP_SET_STREAM redirect when it returns, so a list may only be
cut where no redirect is open; the cuts start at 0, end at len, rise strictly; every chunk but the last has at least `chunk` ops, and none is longer
than the redirects force it to be (a cut falls on the FIRST closed position `chunk` or more ops behind the previous one -- without this a single
chunk over the whole list would pass, and the interleave of the replica streams would be gone)."""
import pytest

from dasr_amd import _lib
from dasr_amd.engine import OpList

EINVAL = -22
A, B = 0x1000, 0x2000                     # stand-ins for two hipStream_t handles (safe_cuts only asks whether the pointer is null)


def _list(pattern):
    """'.': an ordinary op; 'a' / 'b': OP_SET_STREAM to stream A / B; '0': OP_SET_STREAM back to the call's stream"""
    ol = OpList()
    for ch in pattern:
        if ch == '.':
            ol.add(_lib.make_op(_lib.OP_FILL, p=0x100, n=1, value=0.0))
        else:
            ol.add(_lib.make_op(_lib.OP_SET_STREAM, stream={'a': A, 'b': B, '0': None}[ch]))
    return ol


def _closed(pattern):
    """closed[i]: no redirect is open between ops i - 1 and i (i = 0 .. len)"""
    out, is_open = [True], False
    for ch in pattern:
        if ch != '.':
            is_open = ch != '0'
        out.append(not is_open)
    return out


PATTERNS = {
    'empty': '',
    'one_op': '.',
    'no_redirect': '.' * 23,
    'one_redirect': '....a.......0......',
    'redirect_at_start': 'a...0........',
    'redirect_open_at_end': '.......a....',
    'two_in_sequence': '..a....0..a.....0....',
    'nested_in_sequence': '...a...b....0.....a.b.0.0..',      # A, then B without closing A: one NULL closes; a NULL with nothing open
    'redirect_longer_than_chunks': '.a' + '.' * 30 + '0....',
    'back_to_back': '.a0a0a0....',
}


@pytest.mark.parametrize('chunk', [1, 2, 3, 5, 8, 48])
@pytest.mark.parametrize('name', sorted(PATTERNS))
def test_safe_cuts_contract(name, chunk):
    pat = PATTERNS[name]
    ol, closed = _list(pat), _closed(pat)
    cuts = ol.safe_cuts(chunk)
    n = len(pat)
    assert cuts[0] == 0 and cuts[-1] == n
    assert all(a < b for a, b in zip(cuts, cuts[1:]))
    assert all(closed[c] for c in cuts[1:-1]), (cuts, pat)         # (the last cut is the end of the list, wherever that is)
    for a, b in zip(cuts[:-1], cuts[1:-1]):                          # every chunk but the last
        first = next(p for p in range(a + chunk, n + 1) if closed[p])
        assert b - a >= chunk and b == first, (cuts, pat)
    if len(cuts) > 1:                                                # the last chunk ends at len because nothing closed came `chunk` ops behind its start
        assert not any(closed[p] for p in range(cuts[-2] + chunk, n)), (cuts, pat)


def test_safe_cuts_stretch_over_a_redirect():
    """spelled out on one list: chunk 4, a redirect open over ops 3 .. 11"""
    ol = _list('...a.......0......')
    assert ol.safe_cuts(4) == [0, 12, 16, 18]
    assert ol.safe_cuts(1) == [0, 1, 2, 3, 12, 13, 14, 15, 16, 17, 18]
    assert ol.safe_cuts(100) == [0, 18]


def test_safe_cuts_cache_follows_the_list():
    ol = _list('.' * 10)
    first = ol.safe_cuts(4)
    assert first == [0, 4, 8, 10] and ol.safe_cuts(4) is first       # cached
    assert ol.safe_cuts(3) == [0, 3, 6, 9, 10]                       # another chunk size is another answer
    assert ol.safe_cuts(4) == [0, 4, 8, 10]
    ol.add(_lib.make_op(_lib.OP_SET_STREAM, stream=A))
    for _ in range(5):
        ol.add(_lib.make_op(_lib.OP_FILL, p=0x100, n=1, value=0.0))
    assert ol.safe_cuts(4) == [0, 4, 8, 16]                          # the list grew, by an open redirect: no cut behind op 10
    other = _list('0...')
    ol.extend(other)
    assert ol.safe_cuts(4) == [0, 4, 8, 17, 20]


# ---- argument checks that return before the first HIP call ------------------------------------------------------------------------------------
def test_run_ops_mt_rejects_bad_list_counts_without_a_device():
    import ctypes as C
    L = _lib.lib()
    ops = (_lib.Op * 1)(_lib.make_op(_lib.OP_SET_STREAM))
    ptrs, cnts, sts = (C.c_void_p * 9)(*[C.addressof(ops)] * 9), (C.c_int32 * 9)(*[1] * 9), (C.c_void_p * 9)()
    for nl in (0, -1, 9):
        assert L.dasr_run_ops_mt(ptrs, cnts, sts, nl) == EINVAL
    for args in ((None, cnts, sts), (ptrs, None, sts), (ptrs, cnts, None)):
        assert L.dasr_run_ops_mt(*args, 2) == EINVAL


def test_prof_argument_checks_without_a_device():
    L = _lib.lib()
    try:
        assert L.dasr_prof_begin(0) == EINVAL and L.dasr_prof_begin(-3) == EINVAL
        assert L.dasr_prof_filter(b'x' * 128) == EINVAL and L.dasr_prof_filter(b'x' * 500) == EINVAL
        assert L.dasr_prof_filter(b'x' * 127) == 0
        assert L.dasr_prof_filter(b'') == 0 and L.dasr_prof_filter(None) == 0
    finally:
        L.dasr_prof_filter(None)
