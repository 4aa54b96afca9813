"""GPU: the two entry points of csrc/imgio.hip through ctypes, against numpy / the host functions of dasr_amd/data.py and the reference-made fixture
tests/golden/imresize.npz -- never against the device code itself.

Bounds.  dasr_u8_to_planar: bit-equal to `np.asarray(img, np.float32) / 255.0` followed by the crop (one correctly rounded fp32 division on either side).
dasr_imresize_down against the fixture: 5e-7, what tests/test_util_metrics.py holds imresize_matlab to on the same file.  Against imresize_matlab: 2^-23.  Both sides
add the same fp64 products (up to 18 x 18 per sample, |weight| sums under 1.5 per axis, |sample| <= 2) in a different order, which moves the fp64 value by a few 1e-16; each
side then rounds once to fp32, so the two results are equal or neighbouring fp32 numbers, and below magnitude 2 neighbours are at most 2^-23 apart.  A larger difference
means a wrong tap, weight or mirror rule."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EINVAL = -22
ULP = 2.0 ** -23


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _planar(dev, a, Hc, Wc):
    """dasr_u8_to_planar of the uint8 HWC array `a`: [3, Hc, Wc] fp32 on the host"""
    from dasr_amd import _lib
    H, W = a.shape[:2]
    src = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dst = torch.full((3, Hc, Wc), -7.0, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dasr_u8_to_planar(src.data_ptr(), H, W, Hc, Wc, dst.data_ptr(), _st()), 'dasr_u8_to_planar')
    return dst.cpu().numpy()


def _down(dev, x, s, check=True):
    """dasr_imresize_down of the fp32 CHW host tensor `x` with the tables of bicubic_taps: (return code, [C, H / s, W / s] fp32 host tensor)"""
    from dasr_amd import _lib
    from dasr_amd.data import bicubic_taps
    c, H, W = x.shape
    ok = s in (2, 3, 4)
    tabs = []
    for n in (H, W):     # (a refused call never reads its tables: any table stands in)
        j, w = bicubic_taps(n, 1.0 / s if ok else 0.25)
        tabs += [j.to(torch.int32).contiguous().to(dev), w.contiguous().to(dev)]
    Ho, Wo = (max(H // s, 1), max(W // s, 1)) if s > 0 else (1, 1)
    src = x.contiguous().to(dev)
    tmp = torch.empty((c, Ho, W), dtype=torch.float64, device=dev)
    dst = torch.full((c, Ho, Wo), -7.0, dtype=torch.float32, device=dev)
    rc = _lib.lib().dasr_imresize_down(src.data_ptr(), c, H, W, s, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), tabs[3].data_ptr(), tmp.data_ptr(),
                                       dst.data_ptr(), _st())
    if check:
        _lib.check(rc, 'dasr_imresize_down')
    return rc, dst.cpu()


@pytest.mark.parametrize('H,W', [(1, 1), (7, 5), (61, 83), (339, 510)])
def test_u8_to_planar_is_bit_equal_to_numpy_for_every_crop_remainder(H, W):
    dev = _gpu()
    a = np.random.RandomState(H * 1000 + W).randint(0, 256, (H, W, 3), dtype=np.uint8)
    want = np.ascontiguousarray(np.transpose(np.asarray(a, dtype=np.float32) / 255.0, (2, 0, 1)))     # load_image
    assert want.dtype == np.float32
    seen = set()
    for scale in (1, 2, 3, 4):
        for dh in range(scale):          # sizes H - dh, W - dw of the same bytes: every remainder modulo the scale
            for dw in range(scale):
                h, w = H - dh, W - dw
                if h < 1 or w < 1:
                    continue
                Hc, Wc = h - h % scale, w - w % scale    # modcrop
                if Hc < 1 or Wc < 1 or (h, w, Hc, Wc) in seen:
                    continue
                seen.add((h, w, Hc, Wc))
                sub = np.ascontiguousarray(a[:h, :w])
                got = _planar(dev, sub, Hc, Wc)
                ref = np.ascontiguousarray(np.transpose(np.asarray(sub, dtype=np.float32) / 255.0, (2, 0, 1))[:, :Hc, :Wc])
                assert got.dtype == np.float32 and got.shape == ref.shape
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (h, w, Hc, Wc)
    assert seen
    assert np.array_equal(_planar(dev, a, H, W).view(np.uint32), want.view(np.uint32))


def test_u8_to_planar_all_byte_values():
    dev = _gpu()
    a = np.zeros((16, 16, 3), dtype=np.uint8)
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    a[:, :, 0], a[:, :, 1], a[:, :, 2] = v, v[::-1, ::-1], v.T
    got = _planar(dev, a, 16, 16)
    ref = np.transpose(np.asarray(a, dtype=np.float32) / 255.0, (2, 0, 1))
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
    assert sorted(set(got[0].ravel().tolist())) == sorted(set((np.arange(256, dtype=np.float32) / 255.0).tolist())) and len(set(got[0].ravel().tolist())) == 256
    # the same through load_image and a PNG file's bytes is covered end to end in tests/test_gpu_eval_folder.py


def test_imresize_down_matches_the_reference_fixture(golden_dir, margins):
    """tests/golden/imresize.npz (the reference's imresize_np on five seeded images): all five cases at the host test's tolerance"""
    dev = _gpu()
    g = np.load(os.path.join(golden_dir, 'imresize.npz'))
    for i in range(5):
        x = torch.from_numpy(g['in%d' % i]).permute(2, 0, 1).contiguous().float()
        s = int(g['scale%d' % i])
        _, y = _down(dev, x, s)
        y = y.permute(1, 2, 0).numpy()
        err = float(np.abs(y - g['out%d' % i]).max())
        margins('imresize_down vs fixture case %d (%s, x1/%d): max abs %.3e (bound 5e-7)' % (i, tuple(x.shape), s, err))
        assert y.shape == g['out%d' % i].shape and err < 5e-7, (i, err)


def _image(kind, H, W, seed):
    if kind == 'noise':
        return torch.from_numpy(np.random.RandomState(seed).rand(3, H, W).astype(np.float32))
    if kind == 'ramp':
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
        return torch.stack([yy / max(H - 1, 1), xx / max(W - 1, 1), 1.9375 * (yy + xx) / max(H + W - 2, 1)]).contiguous()     # magnitudes in [1, 2) included, 2 itself not (there an fp32 unit is 2^-22)
    return torch.full((3, H, W), 0.7310585975646973, dtype=torch.float32)


@pytest.mark.parametrize('H,W', [(16, 16), (24, 36), (52, 44), (128, 96), (1356, 2040)])
def test_imresize_down_is_within_one_fp32_unit_of_imresize_matlab(H, W, margins):
    from dasr_amd.data import imresize_matlab
    dev = _gpu()
    ran = 0
    for s in (2, 3, 4):
        if H % s or W % s:
            continue
        for kind in ('noise', 'ramp', 'constant'):
            x = _image(kind, H, W, H + W + s)
            _, got = _down(dev, x, s)
            want = imresize_matlab(x, 1.0 / s)
            assert got.shape == want.shape == (3, H // s, W // s)
            err = float((got.double() - want.double()).abs().max())
            margins('imresize_down vs imresize_matlab %s %d x %d x1/%d: max abs %.3e (bound 2^-23 = %.3e)' % (kind, H, W, s, err, ULP))
            assert err <= ULP, (kind, H, W, s, err)
            if kind == 'constant':      # a constant image comes back constant
                cerr = float((got.double() - float(x[0, 0, 0])).abs().max())
                assert cerr <= ULP, (H, W, s, cerr)
            ran += 1
    assert ran >= 3


def test_imresize_down_two_runs_give_identical_bits():
    dev = _gpu()
    x = _image('noise', 128, 96, 5)
    for s in (2, 4):
        a, b = _down(dev, x, s)[1], _down(dev, x, s)[1]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_imresize_down_refuses_bad_geometry_and_launches_nothing():
    dev = _gpu()
    for (H, W, s) in ((25, 36, 4), (24, 37, 4), (26, 36, 3), (24, 36, 5), (24, 36, 1), (24, 36, 0), (24, 40, 8)):
        rc, out = _down(dev, torch.rand(3, H, W), s, check=False)
        torch.cuda.synchronize()
        assert rc == EINVAL, (H, W, s, rc)
        assert bool((out == -7.0).all()), (H, W, s)      # the output buffer was not written
