"""CPU: dasr_amd/imgio.py, the host side of csrc/imgio.hip that data.py and dsn_data.py share -- the one decode and its conversion to floats, the refusal of the
descriptor upload without a device, and the order of the random draws, which is what "equal seeds give equal batches" rests on: dsn_data._plan_window against
load_augmented_crop, and the call sequences of data.DeviceUnpairedDataset.sample / DevicePairedDataset._draw."""
import random

import numpy as np
import pytest
import torch


def _png(path, h, w, mode='RGB', seed=0):
    from PIL import Image
    a = np.random.RandomState(seed).randint(0, 256, (h, w, {'RGB': 3, 'L': 1, 'P': 1, 'RGBA': 4}[mode]), dtype=np.uint8)
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a, mode).save(str(path))
    return str(path)


def test_u8_to_chw_is_the_division_load_image_made_for_all_256_byte_values():
    from dasr_amd.imgio import u8_to_chw
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    a[:, :, 1], a[:, :, 2] = a[::-1, :, 0], a[:, ::-1, 0]
    want = torch.from_numpy(np.asarray(a, np.float32) / 255.0).permute(2, 0, 1)
    got = u8_to_chw(a)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 16, 16) and set(a[:, :, 0].ravel().tolist()) == set(range(256))
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))        # bit for bit


@pytest.mark.parametrize('mode', ['RGB', 'L', 'P', 'RGBA'])
def test_decode_u8_is_the_rgb_conversion_of_every_mode_and_the_byte_store_refuses_the_others(tmp_path, mode):
    from PIL import Image
    from dasr_amd.data import _u8_header, load_image
    from dasr_amd.imgio import decode_u8, image_size
    p = _png(tmp_path / ('m_%s.png' % mode), 6, 8, mode, 3)
    want = np.array(Image.open(p).convert('RGB'))
    got = decode_u8(p)
    assert got.dtype == np.uint8 and got.shape == (6, 8, 3) and np.array_equal(got, want) and image_size(p) == (6, 8)
    assert np.array_equal(decode_u8(p, (2, 1, 7, 5)), want[1:5, 2:7])
    t = load_image(p)
    assert t.is_contiguous() and torch.equal(t, torch.from_numpy(np.asarray(want, np.float32) / 255.0).permute(2, 0, 1))
    if mode == 'RGB':
        assert _u8_header(p) == (6, 8)
    else:
        with pytest.raises(ValueError, match=r"m_%s\.png: mode '%s'" % (mode, mode)):
            _u8_header(p)


def test_the_byte_store_refuses_a_npy_file_by_name(tmp_path):
    from dasr_amd.data import _u8_header
    np.save(str(tmp_path / 'map.npy'), np.zeros((3, 6, 8), np.float32))
    with pytest.raises(ValueError, match=r'map\.npy: a \.npy file in an image folder'):
        _u8_header(str(tmp_path / 'map.npy'))


def test_upload_names_the_missing_device():
    import ctypes
    from dasr_amd import _lib
    from dasr_amd.imgio import upload
    with pytest.raises(_lib.DasrHipError, match='batches are assembled by HIP kernels on images resident in device memory; this dataset was built on cpu'):
        upload(torch.device('cpu'), (_lib.CropDesc * 2)(), (ctypes.c_double * 3)())


@pytest.mark.parametrize('flips,rotations', [(False, False), (True, False), (False, True), (True, True)])
def test_load_augmented_crop_takes_its_draws_from_plan_window(tmp_path, flips, rotations):
    from dasr_amd.dsn_data import _plan_window, load_augmented_crop
    from dasr_amd.imgio import decode_u8, u8_to_chw
    p = _png(tmp_path / 'a.png', 12, 10, 'RGB', 5)
    whole = u8_to_chw(decode_u8(p))
    seen = set()
    for seed in range(24):
        random.seed(seed)
        y, x, flags = _plan_window(12, 10, 8, flips, rotations)
        state = random.getstate()
        random.seed(seed)
        got = load_augmented_crop(p, 8, flips, rotations)
        assert random.getstate() == state                            # the same draws, no more and no fewer
        want = whole[:, y:y + 8, x:x + 8]
        if flags & 1:
            want = want.flip(1)
        if flags & 2:
            want = want.flip(2)
        want = torch.rot90(want, flags >> 2, (1, 2))
        assert got.is_contiguous() and torch.equal(got, want), (seed, y, x, flags)
        assert 0 <= y <= 4 and 0 <= x <= 2 and flags >> 4 == 0 and (flips or not flags & 3) and (rotations or not flags >> 2)
        seen.add(flags)
    assert len(seen) > 1 or not (flips or rotations)


@pytest.mark.parametrize('on', [True, False])
def test_the_training_datasets_draw_in_the_order_of_the_reference(monkeypatch, on):
    """unpaired: np.random.randint for real_LR then HR, random.randint y_f x_f y_r x_r y_u x_u, then the coins; paired: random.randint twice, then the coins.
    The coins: one random.random() under use_flip, two under use_rot, none for a switch that is off"""
    from dasr_amd.data import DevicePairedDataset, DeviceUnpairedDataset
    calls = []

    def recording(name, fn):
        def wrapper(*a):
            calls.append((name,) + a)
            return fn(*a)
        return wrapper
    monkeypatch.setattr(random, 'randint', recording('randint', random.randint))
    monkeypatch.setattr(random, 'random', recording('random', random.random))
    monkeypatch.setattr(np.random, 'randint', recording('np.randint', np.random.randint))
    opt = {'batch_size': 2, 'HR_size': 16, 'use_flip': on, 'use_rot': on}
    coins = [('random',)] * 3 if on else []

    unp = DeviceUnpairedDataset(opt, 4, device='cpu', images={'fake_LR': [torch.zeros(3, 7, 9)] * 4, 'real_LR': [torch.zeros(3, 6, 8)] * 3,
                                                              'HR': [torch.zeros(3, 28, 36)] * 4, 'fake_w': [torch.zeros(1, 5, 6)] * 4})
    assert len(unp) == 2 and not calls
    smp = unp.sample(1)
    assert calls == [('np.randint', 0, 3), ('np.randint', 0, 4), ('randint', 0, 3), ('randint', 0, 5), ('randint', 0, 2), ('randint', 0, 4),
                     ('randint', 0, 12), ('randint', 0, 20)] + coins
    assert 0 <= smp['flags'] < 8 and (on or smp['flags'] == 0) and smp['fake_w'][1] == (7, 9) and smp['HR'][2:] == (4 * smp['LR_fake'][2], 4 * smp['LR_fake'][3])

    del calls[:]
    par = DevicePairedDataset(opt, 4, device='cpu', images={'HR': [torch.zeros(3, 28, 36)] * 2, 'LR': [torch.zeros(3, 7, 9)] * 2})
    assert len(par) == 1 and not calls
    y0, x0, flags = par._draw(1)
    assert calls == [('randint', 0, 3), ('randint', 0, 5)] + coins and 0 <= flags < 8 and (on or flags == 0)
    del calls[:]
    par.img['LR'] = None                                             # (`resident_u8` without LR files) the window is drawn in the H / 4 x W / 4 image
    par._draw(0)
    assert calls == [('randint', 0, 3), ('randint', 0, 5)] + coins


def test_the_coins_set_the_flag_bits_hflip_1_vflip_2_transpose_4(monkeypatch):
    from dasr_amd.data import DevicePairedDataset
    ds = DevicePairedDataset.__new__(DevicePairedDataset)
    for flip, rot, draws, want in ((True, True, [0.1, 0.9, 0.9], 1), (True, True, [0.9, 0.1, 0.9], 2), (True, True, [0.9, 0.9, 0.1], 4), (True, True, [0.1, 0.1, 0.1], 7),
                                   (True, False, [0.1], 1), (False, True, [0.1, 0.9], 2), (False, False, [], 0)):
        ds.use_flip, ds.use_rot = flip, rot
        left = list(draws)
        monkeypatch.setattr(random, 'random', lambda: left.pop(0))
        assert ds._coins() == want and not left
