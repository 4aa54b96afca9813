"""CPU: the host parts of `"resident_u8": true` (data.DeviceUnpairedDataset / DevicePairedDataset and the two entry points of csrc/imgio.hip behind them) -- the symbols,
the descriptor layout, the argument checks made in front of the first HIP call, the single weight row dasr_crops_down4_u8 is fed with, the refusals and the routing."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def _png(path, h, w, seed=0, mode='RGB'):
    from PIL import Image
    a = np.random.RandomState(seed).randint(0, 256, (h, w, {'RGB': 3, 'L': 1, 'RGBA': 4}[mode]), dtype=np.uint8)
    Image.fromarray(a[:, :, 0] if mode == 'L' else a, mode).save(str(path))


def _folder(tmp_path, name, sizes, seed=0):
    d = tmp_path / name
    d.mkdir()
    for i, (h, w) in enumerate(sizes):
        _png(d / ('%s_%02d.png' % (name, i)), h, w, seed + i)
    return str(d)


def test_symbols_are_declared_bound_and_exported_and_the_abi_number_stays():
    from dasr_amd import build, _lib
    hdr = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    declared = set(re.findall(r'^\s*int\s+(dasr_\w+)\s*\(', hdr, flags=re.M))
    build.build()
    L = _lib.lib()
    for name in ('dasr_gather_srn_u8', 'dasr_crops_down4_u8'):
        assert name in declared and name in _lib._SIGS and hasattr(L, name), name
    assert 'dasr_srn_u8_desc' in hdr
    assert _lib.ABI_VERSION == 22 and '#define DASR_ABI_VERSION 22' in hdr and L.dasr_abi_version() == 22


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of dasr_srn_u8_desc as the host compiler lays it out = the ctypes structure the descriptors are packed with (40 bytes, like dasr_crop_desc: the
    two kinds share one staging block)"""
    from dasr_amd import _lib
    fields = [f for f, _ in _lib.SrnU8Desc._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dasr_hip.h"\nint main(void){printf("%zu", sizeof(dasr_srn_u8_desc));\n' +
                   ''.join('printf(" %%zu", offsetof(dasr_srn_u8_desc, %s));\n' % f for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.SrnU8Desc)] + [getattr(_lib.SrnU8Desc, f).offset for f in fields]
    assert ctypes.sizeof(_lib.SrnU8Desc) == 40 and ctypes.sizeof(_lib.SrnU8Desc) % 8 == 0 and ctypes.sizeof(_lib.CropDesc) % 8 == 0


def test_entry_points_reject_bad_arguments_before_any_launch():
    """every DASR_EINVAL clause, in front of the first HIP call (the non-null pointers stand for device addresses and are never dereferenced)"""
    from dasr_amd import _lib
    from dasr_amd.data import down4_weights
    L = _lib.lib()
    p = 4096
    assert L.dasr_gather_srn_u8(None, 2, 64, None) == EINVAL
    assert L.dasr_gather_srn_u8(p, 0, 64, None) == EINVAL and L.dasr_gather_srn_u8(p, -1, 64, None) == EINVAL and L.dasr_gather_srn_u8(p, 65536, 64, None) == EINVAL
    assert L.dasr_gather_srn_u8(p, 2, 0, None) == EINVAL and L.dasr_gather_srn_u8(p, 2, -4, None) == EINVAL and L.dasr_gather_srn_u8(p, 2, 4097, None) == EINVAL
    w = ctypes.addressof(down4_weights())

    def down(n=2, size=8, dev=p, host=True, wt=w, **bad):
        descs = (_lib.SrnU8Desc * 2)()
        for d in descs:
            d.src, d.H, d.W, d.y0, d.x0, d.size, d.flags, d.dst = p, 64, 48, 8, 4, 8, 0, p
        for k, v in bad.items():
            setattr(descs[1], k, v)
        return L.dasr_crops_down4_u8(dev, ctypes.addressof(descs) if host else None, n, size, wt, None)
    assert down(dev=None) == EINVAL and down(host=False) == EINVAL and down(wt=None) == EINVAL
    assert down(n=0) == EINVAL and down(n=-1) == EINVAL and down(n=65536) == EINVAL
    assert down(size=0) == EINVAL and down(size=-8) == EINVAL and down(size=129) == EINVAL and down(size=132, H=1024, W=1024) == EINVAL
    assert down(H=66) == EINVAL and down(W=50) == EINVAL and down(H=0) == EINVAL and down(W=-4) == EINVAL          # H, W: positive multiples of 4
    assert down(src=None) == EINVAL and down(dst=None) == EINVAL
    assert down(size=4) == EINVAL and down(size=12) == EINVAL                                                       # every descriptor has the size of the call
    assert down(y0=-1) == EINVAL and down(x0=-1) == EINVAL and down(y0=9) == EINVAL and down(x0=5) == EINVAL        # the window lies in the 16 x 12 LR image


@pytest.mark.parametrize('n', [32, 36, 52, 128, 2040])
def test_the_single_weight_row_is_every_row_of_the_tap_table_and_the_indices_are_formed_from_the_position(n):
    from dasr_amd.data import bicubic_taps, down4_weights
    j, w = bicubic_taps(n, 0.25)
    row = torch.tensor(list(down4_weights()), dtype=torch.float64)
    assert w.shape == (n // 4, 18) and all(torch.equal(r, row) for r in w)
    assert float(row.abs().sum()) < 1.5                         # with samples in [0, 1] every output is below 2 in magnitude: the 2^-23 bound of the GPU test
    # what the kernel computes instead of reading a table: tap t of output o is input 4 o - 7 + t, mirrored (j < 0 -> -j - 1, then j >= n -> 2 n - 1 - j), clamped
    raw = 4 * torch.arange(n // 4)[:, None] - 7 + torch.arange(18)[None, :]
    m = torch.where(raw < 0, -raw - 1, raw)
    m = torch.where(m >= n, 2 * n - 1 - m, m).clamp(0, n - 1)
    assert torch.equal(j, m)


def test_refusals_name_their_cause_and_need_no_device(tmp_path):
    from dasr_amd.data import DevicePairedDataset, DeviceUnpairedDataset
    hr = _folder(tmp_path, 'hr', [(40, 56), (40, 56)])
    lr = _folder(tmp_path, 'lr', [(10, 14), (10, 14)], 10)
    base = {'batch_size': 1, 'HR_size': 32, 'resident_u8': True, 'n_workers': 2, 'phase': 'train', 'dataroot_HR': hr, 'dataroot_LR': lr}
    unp = dict(base, dataroot_fake_LR=lr, dataroot_real_LR=lr, dataroot_fake_weights=lr)
    # a caller-supplied images= dict
    for cls, o in ((DevicePairedDataset, base), (DeviceUnpairedDataset, unp)):
        with pytest.raises(ValueError, match='images='):
            cls(dict(o), 4, images={'HR': [torch.rand(3, 40, 56)], 'LR': None})
    # a .npy file in an image folder
    np.save(os.path.join(lr, 'lr_00.npy'), np.zeros((3, 10, 14), np.float32))
    for cls, o in ((DevicePairedDataset, base), (DeviceUnpairedDataset, unp)):
        with pytest.raises(ValueError, match=r'lr_00\.npy.*\.npy file in an image folder'):
            cls(dict(o), 4, device='cpu')
    os.remove(os.path.join(lr, 'lr_00.npy'))
    # grey and alpha files
    for mode in ('L', 'RGBA'):
        bad = os.path.join(hr, 'zz_%s.png' % mode)
        _png(bad, 40, 56, 3, mode)
        with pytest.raises(ValueError, match=r"zz_%s\.png: mode '%s'" % (mode, mode)):
            DevicePairedDataset(dict(base, dataroot_LR=None), 4, device='cpu')
        with pytest.raises(ValueError, match=r"zz_%s\.png: mode '%s'" % (mode, mode)):
            DeviceUnpairedDataset(dict(unp), 4, device='cpu')
        os.remove(bad)
    # a scale other than 4 without LR files
    with pytest.raises(NotImplementedError, match='scale 4 .*got scale 2'):
        DevicePairedDataset(dict(base, dataroot_LR=None), 2, device='cpu')
    # files smaller than their window (the byte kernel would clamp where the fp32 one writes zeros)
    with pytest.raises(ValueError, match=r'lr_00\.png: image 10x14 is smaller than the crop size 12'):
        DevicePairedDataset(dict(base, HR_size=48), 4, device='cpu')
    # HR sizes that are no multiple of the scale: as without the key
    odd = _folder(tmp_path, 'odd', [(42, 56)])
    with pytest.raises(NotImplementedError, match='42 x 56 is not a multiple of scale 4'):
        DevicePairedDataset(dict(base, dataroot_HR=odd, dataroot_LR=None), 4, device='cpu')
    # the cap
    total = 3 * 2 * (40 * 56 + 10 * 14)
    with pytest.raises(MemoryError) as e:
        DevicePairedDataset(dict(base), 4, max_bytes=total - 1)
    assert str(total) in str(e.value) and 'drop "resident_u8"' in str(e.value)
    with pytest.raises(MemoryError, match='drop "resident_u8"'):
        DevicePairedDataset(dict(base, resident_max_bytes=100), 4)
    with pytest.raises(MemoryError, match='drop "resident_u8"'):
        DeviceUnpairedDataset(dict(unp, dataroot_fake_weights=hr), 4, max_bytes=100)
    # at the cap, on the host: stored as the decoded bytes; batches need the device
    ds = DevicePairedDataset(dict(base), 4, device='cpu', max_bytes=total)
    assert ds.resident_bytes == total and all(t.dtype == torch.uint8 and tuple(t.shape) == (40, 56, 3) for t in ds.img['HR']) and len(ds) == 2
    from dasr_amd._lib import DasrHipError
    with pytest.raises(DasrHipError):
        ds.batch([0])


def test_subset_file_and_routing(tmp_path):
    from dasr_amd import train
    from dasr_amd.data import DevicePairedDataset
    hr = _folder(tmp_path, 'hr', [(40, 56)] * 4)
    sub = tmp_path / 'subset.txt'
    sub.write_text('hr_03.png\nhr_00.png\n')
    ds_opt = {'mode': 'LRHR', 'phase': 'train', 'batch_size': 1, 'HR_size': 32, 'dataroot_HR': hr, 'subset_file': str(sub)}
    assert DevicePairedDataset.hr_paths(ds_opt) == [os.path.join(hr, 'hr_00.png'), os.path.join(hr, 'hr_03.png')]
    assert len(DevicePairedDataset.hr_paths(dict(ds_opt, subset_file=None))) == 4
    assert len(DevicePairedDataset.hr_paths(dict(ds_opt, phase='val'))) == 4           # a training-phase list
    with pytest.raises(NotImplementedError, match='Now subset only supports generating LR on-the-fly.'):
        train.create_dataset(dict(ds_opt, dataroot_LR=hr), {'scale': 4, 'model': 'sr'})
    with pytest.raises(NotImplementedError, match='Now subset only supports generating LR on-the-fly.'):
        train.create_dataset(dict(ds_opt, dataroot_LR=hr, resident_u8=True), {'scale': 4, 'model': 'sr'})
    # the key routes an HR-only train set to the paired dataset (refused here for its scale, before any device is touched); without it nothing changed
    with pytest.raises(NotImplementedError, match='got scale 3'):
        train.create_dataset({'mode': 'LRHR', 'phase': 'train', 'batch_size': 1, 'HR_size': 33, 'dataroot_HR': hr, 'resident_u8': True}, {'scale': 3, 'model': 'sr'})
    with pytest.raises(NotImplementedError, match='not recognized'):
        train.create_dataset({'mode': 'LRHR', 'phase': 'train', 'batch_size': 1, 'HR_size': 32, 'dataroot_HR': hr}, {'scale': 4, 'model': 'sr'})
    with pytest.raises(NotImplementedError, match='not recognized'):
        train.create_dataset({'mode': 'LRHR', 'phase': 'train', 'batch_size': 1, 'HR_size': 32, 'dataroot_HR': hr, 'resident_u8': False}, {'scale': 4, 'model': 'sr'})
