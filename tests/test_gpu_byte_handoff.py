"""GPU: imgio.planar_f32, the one hand-off of decoded bytes to a planar fp32 device image, against the arithmetic of data.load_image on the host
(`torch.from_numpy(a).permute(2, 0, 1).float() / 255`, one correctly rounded fp32 division per sample), bit for bit -- and the same bits through its three callers:
EvalFolderDataset._read, metrics.u8_planes and the call of the back_projection CLI.  Shapes: the smallest at which the window logic can go wrong (one sample; odd
sides; a window shorter on both axes, on each axis by a different amount; the batch axis)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [((1, 1), None, False), ((5, 7), None, False), ((5, 7), (4, 4), False), ((9, 6), (8, 4), False), ((5, 7), None, True)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda', torch.cuda.current_device())


def _bytes(H, W):
    a = np.random.RandomState(H * 16 + W).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    a.flat[:2] = (0, 255)
    return a


def _want(a, window, batch):
    want = torch.from_numpy(a).permute(2, 0, 1).float() / 255      # data.load_image
    Hc, Wc = window or a.shape[:2]
    want = want[:, :Hc, :Wc].contiguous()
    return want[None] if batch else want


def _same_bits(got, want):
    assert got.dtype == torch.float32 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == tuple(want.shape)
    return torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('size,window,batch', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_planar_f32_is_bit_equal_to_load_image_from_an_array_and_from_a_device_tensor(size, window, batch):
    from dasr_amd import imgio
    dev = _gpu()
    a = _bytes(*size)
    want = _want(a, window, batch)
    assert _same_bits(imgio.planar_f32(a, dev, window=window, batch=batch), want)
    assert _same_bits(imgio.planar_f32(torch.from_numpy(a).to(dev), window=window, batch=batch), want)


def test_the_three_callers_hand_over_the_same_bits(tmp_path, monkeypatch):
    """EvalFolderDataset._read (whole, and cut to a multiple of the scale: 9 x 6 at scale 4 is the 8 x 4 window), metrics.u8_planes, and the back_projection CLI:
    main() runs on a folder of one pair (SR 10 x 14, LR 5 x 7) with back_project replaced by a function that keeps its two inputs"""
    from PIL import Image
    from dasr_amd import back_projection, metrics
    from dasr_amd.data import EvalFolderDataset
    dev = _gpu()
    for H, W, crop_to, window in ((1, 1, None, None), (5, 7, None, None), (5, 7, 4, (4, 4)), (9, 6, 4, (8, 4))):
        a = _bytes(H, W)
        folder = tmp_path / ('d%d_%d_%s' % (H, W, crop_to))
        folder.mkdir()
        Image.fromarray(a).save(str(folder / 'img.png'))
        ds = EvalFolderDataset({'mode': 'LR', 'dataroot_LR': str(folder)}, 4, device=dev)
        assert _same_bits(ds._read(ds.paths_LR[0], crop_to=crop_to), _want(a, window, True))
        if window is None:
            f, u = metrics.u8_planes(torch.from_numpy(a).to(dev))
            assert _same_bits(f, _want(a, None, False)) and np.array_equal(u.cpu().numpy(), a.transpose(2, 0, 1))
    sr, lr, seen = _bytes(10, 14), _bytes(5, 7), []
    for name, a in (('sr', sr), ('lr', lr)):
        (tmp_path / name).mkdir()
        Image.fromarray(a).save(str(tmp_path / name / 'img.png'))
    monkeypatch.setattr(back_projection, 'back_project', lambda s, l, iters: seen.append((s, l, iters)) or s.clone())
    written = back_projection.main(['--sr_dir', str(tmp_path / 'sr'), '--lr_dir', str(tmp_path / 'lr'), '--out_dir', str(tmp_path / 'out'), '--iters', '3'])
    assert len(written) == 1 and len(seen) == 1 and seen[0][2] == 3
    assert _same_bits(seen[0][0], _want(sr, None, True)) and _same_bits(seen[0][1], _want(lr, None, True))
    assert np.array_equal(np.asarray(Image.open(written[0])), sr)      # (byte / 255 quantised back: the PNG of the untouched SR image)
