"""Host-side checks of the LPIPS, PReLU-slope and crop-gather launchers: every null-pointer clause of DASR_EINVAL is answered in front of the first
HIP call and in front of the host reads of scale4 / shift4.  The non-null pointers are made-up addresses, so this only fails cleanly where no kernel
can run: the test skips on a machine with a GPU, where tests/test_gpu_lpips_prelu.py::test_argument_checks passes the same nulls with real buffers."""
import ctypes as C

import pytest
import torch

EINVAL = -22


def test_launchers_reject_null_pointers_before_any_launch():
    """the non-null pointers stand for device addresses and are never dereferenced; the eight floats are real host memory"""
    if torch.cuda.is_available():
        pytest.skip('made-up device addresses: only for a machine without a GPU')
    from dasr_amd import build, _lib
    build.build()
    L = _lib.lib()
    p = 4096
    T, Z = _lib.Tensor(p, 1024, 64), _lib.Tensor(None, 0, 0)
    f4 = (C.c_float * 4)(1.0, 1.0, 1.0, 0.0)
    h = C.cast(f4, C.c_void_p)
    assert L.dasr_lpips_s2d(Z, 2, 8, 12, h, h, T, 0, None) == EINVAL and L.dasr_lpips_s2d(T, 2, 8, 12, h, h, Z, 0, None) == EINVAL
    assert L.dasr_lpips_s2d(T, 2, 8, 12, None, h, T, 0, None) == EINVAL and L.dasr_lpips_s2d(T, 2, 8, 12, h, None, T, 1, None) == EINVAL
    assert L.dasr_lpips_s2d(T, 2, 8, 12, None, None, T, 2, None) == EINVAL and L.dasr_lpips_s2d(T, 2, 6, 12, h, h, T, 0, None) == EINVAL
    assert L.dasr_maxpool3s2(Z, 2, 16, 7, 9, T, None) == EINVAL and L.dasr_maxpool3s2(T, 2, 16, 7, 9, Z, None) == EINVAL
    for x, gy, gx in ((Z, T, T), (T, Z, T), (T, T, Z)):
        assert L.dasr_maxpool3s2_bwd(x, gy, 2, 16, 7, 9, gx, 1, 0, None) == EINVAL
    assert L.dasr_lpips_head(Z, 2, 2, 16, 5, 7, p, 1e-10, 1.0, 1.0, p, T, 0, None) == EINVAL
    assert L.dasr_lpips_head(T, 2, 2, 16, 5, 7, None, 1e-10, 1.0, 1.0, p, T, 0, None) == EINVAL
    for fn in (L.dasr_prelu_grad, L.dasr_prelu_grad_f16):
        for k in range(5):
            y, gx = (Z if k == 0 else T), (Z if k == 1 else T)
            slope, scratch, dst = (None if k == j else p for j in (2, 3, 4))
            assert fn(y, gx, 2, 16, 5, 7, slope, scratch, dst, 1.0, None) == EINVAL, k
        assert fn(T, T, 0, 16, 5, 7, p, p, p, 1.0, None) == EINVAL and fn(T, T, 2, 16, -5, -7, p, p, p, 1.0, None) == EINVAL
    for k in range(3):
        part, sl, ds = (None if k == j else p for j in (0, 1, 2))
        assert L.dasr_prelu_final(part, 8, 16, 2, sl, ds, 1.0, None) == EINVAL
    assert L.dasr_gather_crops(None, 2, 3, 7, p, None) == EINVAL and L.dasr_gather_crops(p, 2, 3, 7, None, None) == EINVAL
    assert L.dasr_gather_crops(p, -1, -3, 7, p, None) == EINVAL and L.dasr_gather_crops(p, 2, 3, 0, p, None) == EINVAL
