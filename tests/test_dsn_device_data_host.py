"""CPU: the host parts of `--device_data` (dsn_data.DeviceTrainDeresnet / DeviceValDeresnet / DeviceDeresnetLoader and the two entry points of csrc/imgio.hip behind
them) -- the symbols, the argument checks made in front of the first HIP call, the tap table dasr_crops_bicubic_down is fed with, the order of the random draws and
the meaning of a crop descriptor (a numpy emulation of dasr_gather_crops_u8 against TrainDeresnetDataset.__getitem__), and the refusals."""
import collections
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def _png(path, h, w, seed=0):
    from PIL import Image
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)).save(str(path))


def _folders(tmp_path, noisy_sizes, clean_sizes):
    noisy, clean = tmp_path / 'noisy', tmp_path / 'clean'
    noisy.mkdir()
    clean.mkdir()
    for i, (h, w) in enumerate(noisy_sizes):
        _png(noisy / ('n%02d.png' % i), h, w, 100 + i)
    for i, (h, w) in enumerate(clean_sizes):
        _png(clean / ('c%02d.png' % i), h, w, 200 + i)
    return str(noisy), str(clean)


def emulate_gather(plan):
    """what dasr_gather_crops_u8 writes for one descriptor, in numpy on the decoded uint8 array: [3, size, size] fp32"""
    a = plan.image.numpy()[plan.y0:plan.y0 + plan.crop, plan.x0:plan.x0 + plan.crop]
    if plan.flags & 1:
        a = a[::-1]                                  # vertical flip
    if plan.flags & 2:
        a = a[:, ::-1]                               # horizontal flip
    a = np.rot90(a, (plan.flags >> 2) & 3, (0, 1))   # quarter-turns counter-clockwise
    a = a[plan.sub_y:plan.sub_y + plan.size, plan.sub_x:plan.sub_x + plan.size]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0))


def test_symbols_are_declared_bound_and_exported_and_the_abi_number_stays():
    from dasr_amd import build, _lib
    hdr = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    declared = set(re.findall(r'^\s*int\s+(dasr_\w+)\s*\(', hdr, flags=re.M))
    build.build()
    L = _lib.lib()
    for name in ('dasr_gather_crops_u8', 'dasr_crops_bicubic_down'):
        assert name in declared and name in _lib._SIGS and hasattr(L, name), name
    assert 'dasr_crop_u8_desc' in hdr
    assert _lib.ABI_VERSION == 22 and '#define DASR_ABI_VERSION 22' in hdr and L.dasr_abi_version() == 22
    src = open(os.path.join(ROOT, 'dasr_amd', 'csrc', 'imgio.hip')).read()
    assert '#pragma clang fp contract(off)' in src and '/ 255.0f' in src


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of dasr_crop_u8_desc as the host compiler lays it out = the ctypes structure the descriptors are packed with"""
    import ctypes
    import subprocess
    from dasr_amd import _lib
    fields = [f for f, _ in _lib.CropU8Desc._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dasr_hip.h"\nint main(void){printf("%zu", sizeof(dasr_crop_u8_desc));\n' +
                   ''.join('printf(" %%zu", offsetof(dasr_crop_u8_desc, %s));\n' % f for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.CropU8Desc)] + [getattr(_lib.CropU8Desc, f).offset for f in fields]


def test_entry_points_reject_bad_arguments_before_any_launch():
    """every DASR_EINVAL clause, in front of the first HIP call (the non-null pointers stand for device addresses and are never dereferenced)"""
    from dasr_amd import _lib
    L = _lib.lib()
    p = 4096
    assert L.dasr_gather_crops_u8(None, 2, 64, p, None) == EINVAL and L.dasr_gather_crops_u8(p, 2, 64, None, None) == EINVAL
    assert L.dasr_gather_crops_u8(p, 0, 64, p, None) == EINVAL and L.dasr_gather_crops_u8(p, -1, 64, p, None) == EINVAL
    assert L.dasr_gather_crops_u8(p, 2, 0, p, None) == EINVAL and L.dasr_gather_crops_u8(p, 2, -4, p, None) == EINVAL
    assert L.dasr_gather_crops_u8(p, 2, 4097, p, None) == EINVAL and L.dasr_gather_crops_u8(p, 65536, 64, p, None) == EINVAL    # (n is a grid dimension)

    def down(n=2, c=256, s=4, ptrs=(p,) * 4):
        hr, idx, wt, dst = ptrs
        return L.dasr_crops_bicubic_down(hr, n, c, s, idx, wt, dst, None)
    for k in range(4):
        assert down(ptrs=tuple(None if i == k else p for i in range(4))) == EINVAL
    assert down(s=2) == EINVAL and down(s=3) == EINVAL and down(s=8) == EINVAL and down(s=0) == EINVAL
    assert down(c=258) == EINVAL and down(c=255) == EINVAL and down(c=1028) == EINVAL and down(c=2048) == EINVAL and down(c=0) == EINVAL and down(c=-4) == EINVAL
    assert down(n=0) == EINVAL and down(n=-1) == EINVAL and down(n=65536) == EINVAL
    assert down(ptrs=(4100, p, p, p)) == EINVAL and down(ptrs=(4104, p, p, p)) == EINVAL      # hr is staged with 16-byte loads


@pytest.mark.parametrize('c', [64, 256, 260])
def test_tap_table_scatters_to_the_resize_matrix_of_the_host_path(c):
    """the table the kernel is fed with (data.bicubic_taps) and the dense matrix the host imresize multiplies with are one set of weights"""
    from dasr_amd.data import bicubic_taps
    from dasr_amd.dsn_data import resize_matrix
    j, w = bicubic_taps(c, 0.25)
    assert j.shape == w.shape == (c // 4, 18) and w.dtype == torch.float64
    assert int(j.min()) >= 0 and int(j.max()) <= c - 1
    M = torch.zeros(c // 4, c, dtype=torch.float64)
    M.scatter_add_(1, j, w)
    assert float((M - resize_matrix(c, 0.25, True, torch.float64)).abs().max()) <= 1e-15
    # what the kernel's staging relies on: before mirroring the taps of output row o are the 18 consecutive rows from 4 o - 7 on
    o = torch.arange(c // 4)[:, None]
    raw = 4 * o - 7 + torch.arange(18)[None, :]
    mirrored = torch.where(raw < 0, -raw - 1, torch.where(raw >= c, 2 * c - 1 - raw, raw))
    assert torch.equal(j, mirrored)


@pytest.mark.parametrize('flips,rotations', [(False, False), (True, False), (False, True), (True, True)])
def test_plan_item_draws_like_the_host_dataset_and_the_descriptors_mean_its_crops(tmp_path, flips, rotations):
    from dasr_amd.dsn_data import DeviceTrainDeresnet, TrainDeresnetDataset
    noisy, clean = _folders(tmp_path, [(40, 52), (33, 47), (64, 36), (32, 32), (45, 45)], [(70, 90), (61, 83), (64, 64)])
    crop = 32
    host = TrainDeresnetDataset(noisy, clean, crop, 4, cropped=True, flips=flips, rotations=rotations)
    dev = DeviceTrainDeresnet(noisy, clean, crop, 4, flips=flips, rotations=rotations, device='cpu', threads=3)
    assert len(dev) == len(host) == 5 and dev.noisy_dir_files == host.noisy_dir_files and dev.cleandir_files == host.cleandir_files
    seen = collections.Counter()
    rounds = 40 if flips and rotations else 4
    for rnd in range(rounds):
        for index in range(len(host)):
            seed = 1000 * rnd + index
            random.seed(seed)
            np.random.seed(seed)
            hr, bic, real = host[index]
            state_host = (random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2])
            random.seed(seed)
            np.random.seed(seed)
            p_noisy, p_clean = dev.plan_item(index)
            assert (random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2]) == state_host   # the same number of draws from both generators
            assert (p_clean.size, p_clean.crop, p_clean.sub_y, p_clean.sub_x) == (crop, crop, 0, 0) and (p_noisy.size, p_noisy.crop) == (crop // 4, crop)
            assert torch.equal(emulate_gather(p_clean), hr)
            assert torch.equal(emulate_gather(p_noisy), real)
            for p in (p_noisy, p_clean):
                seen[(p.flags & 1, (p.flags >> 1) & 1, (p.flags >> 2) & 3)] += 1
                assert p.flags >> 4 == 0
    expected = {(v, h, k) for v in ((0, 1) if flips else (0,)) for h in ((0, 1) if flips else (0,)) for k in ((0, 1, 2, 3) if rotations else (0,))}
    assert set(seen) == expected and sum(seen.values()) == 2 * rounds * len(host)     # all 16 (vflip, hflip, k) cases with both switches on, only the allowed ones otherwise


def test_loader_batches_follow_the_sampler_with_a_short_last_batch():
    from dasr_amd.dsn_data import DeviceDeresnetLoader, ShardSampler

    class Recorder:
        def batch(self, indices):
            return list(indices)
    for world, rank in ((1, 0), (2, 1)):
        loader = DeviceDeresnetLoader(Recorder(), 3, ShardSampler(11, True, 5, rank, world))
        ref = ShardSampler(11, True, 5, rank, world)
        for _ in range(2):
            order = list(ref)
            got = list(loader)
            assert [i for b in got for i in b] == order and len(got) == len(loader) == (len(order) + 2) // 3
            assert all(len(b) == 3 for b in got[:-1]) and len(got[-1]) == len(order) - 3 * (len(got) - 1)


def test_memory_cap_and_small_images_are_refused_at_construction_without_a_device(tmp_path):
    from dasr_amd.dsn_data import DeviceTrainDeresnet, DeviceValDeresnet
    noisy, clean = _folders(tmp_path, [(40, 52), (33, 47)], [(70, 90), (64, 64)])
    total = 3 * (40 * 52 + 33 * 47 + 70 * 90 + 64 * 64)
    with pytest.raises(MemoryError) as e:
        DeviceTrainDeresnet(noisy, clean, 32, 4, max_bytes=total - 1)        # (device None: the sum is taken before the device is looked for)
    assert str(total) in str(e.value) and str(total - 1) in str(e.value) and 'host loader' in str(e.value)
    assert len(DeviceTrainDeresnet(noisy, clean, 32, 4, device='cpu', max_bytes=total)) == 2   # at the cap: accepted
    with pytest.raises(MemoryError):
        DeviceValDeresnet(clean, 4, lr_dir=noisy, max_bytes=100)
    with pytest.raises(ValueError, match=r'n01\.png: image 33x47 is smaller than the crop size 36') as e:
        DeviceTrainDeresnet(noisy, clean, 36, 4, max_bytes=1 << 30)
    # the message of the host path for the same file
    from dasr_amd.dsn_data import load_augmented_crop
    with pytest.raises(ValueError) as h:
        load_augmented_crop(os.path.join(noisy, 'n01.png'), 36, False, False)
    assert str(h.value) == str(e.value)
    with pytest.raises(FileNotFoundError):
        DeviceTrainDeresnet(str(tmp_path), clean, 32, 4, device='cpu')
    # what the bicubic kernel does not do is refused at construction, not at the first batch; so is a misspelt argument
    for bad in (dict(crop_size=34), dict(crop_size=1028), dict(crop_size=32, upscale_factor=2)):
        with pytest.raises(NotImplementedError, match='host loader'):
            DeviceTrainDeresnet(noisy, clean, device='cpu', **dict(dict(upscale_factor=4), **bad))
    with pytest.raises(TypeError):
        DeviceTrainDeresnet(noisy, clean, 32, 4, device='cpu', max_byte=10)
    with pytest.raises(TypeError):
        DeviceValDeresnet(clean, 4, lr_dir=noisy, device='cpu', thread=2)
    with pytest.raises(NotImplementedError, match='host loader'):
        DeviceValDeresnet(clean, 2, lr_dir=noisy, device='cpu')
    (tmp_path / 'big').mkdir()
    for i in range(2):
        _png(tmp_path / 'big' / ('b%02d.png' % i), 160, 170, i)
    with pytest.raises(ValueError, match=r'n01\.png: image 33x47 is smaller than the crop size 40'):      # an LR file too small for its HR file's crop / 4: at construction
        DeviceValDeresnet(str(tmp_path / 'big'), 4, lr_dir=noisy, device='cpu')
    # host-resident images plan items but do not assemble batches: no quiet host path
    from dasr_amd._lib import DasrHipError
    with pytest.raises(DasrHipError):
        DeviceTrainDeresnet(noisy, clean, 32, 4, device='cpu').batch([0])


def test_check_supported_refuses_device_data_without_folders_and_the_flag_is_off_by_default():
    from dasr_amd import dsn_train
    parse = dsn_train.build_parser().parse_args
    assert parse([]).device_data is False and parse(['--device_data']).device_data is True
    dsn_train.check_supported(parse(['--dataset', 'aim2019', '--device_data']), have_loader=False)
    dsn_train.check_supported(parse(['--dataset', 'synthetic']), have_loader=False)
    with pytest.raises(ValueError, match='--device_data'):
        dsn_train.check_supported(parse(['--dataset', 'synthetic', '--device_data']), have_loader=False)
    with pytest.raises(ValueError, match='--device_data'):
        dsn_train.check_supported(parse(['--dataset', 'aim2019', '--device_data']), have_loader=True)
    with pytest.raises(ValueError, match='--device_data'):
        dsn_train.main(['--dataset', 'synthetic', '--device_data', '--no_saving'])      # refused before any model is built
