"""CPU: the host parts of data.EvalFolderDataset (mode "LRHR" in the val / test phase, mode "LR") -- folder listing and pairing, the modcrop geometry, the refused
options, the routing in train.create_dataset, the tap tables dasr_imresize_down is fed with, and the argument checks of the two entry points of csrc/imgio.hip
(made in front of the first HIP call, so they run without a device)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def _png(path, h, w, seed=0):
    from PIL import Image
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)).save(str(path))


def test_listing_and_pairing_order(tmp_path):
    from dasr_amd.data import EvalFolderDataset, eval_folder_pairs
    hr, lr = tmp_path / 'hr', tmp_path / 'lr'
    (hr / 'sub').mkdir(parents=True)
    lr.mkdir()
    for name in ('b.png', 'a.png', 'sub/c.png', '10.png', '9.png'):
        _png(hr / name, 8, 8)
    (hr / 'notes.txt').write_text('not an image')
    for name in ('b.png', 'a.png', 'c.npy', '10.png', '9.png'):
        if name.endswith('.npy'):
            np.save(str(lr / name), np.zeros((3, 2, 2), np.float32))
        else:
            _png(lr / name, 2, 2)
    ph, pl = eval_folder_pairs({'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': str(lr)})
    assert [os.path.relpath(p, str(hr)) for p in ph] == ['10.png', '9.png', 'a.png', 'b.png', 'sub/c.png']      # sorted as strings, sub-folders included
    assert [os.path.basename(p) for p in pl] == ['10.png', '9.png', 'a.png', 'b.png', 'c.npy']                     # paired by index
    ds = EvalFolderDataset({'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': str(lr), 'phase': 'val'}, 4)    # (construction needs no GPU)
    assert len(ds) == 5 and ds.paths_HR == ph and ds.paths_LR == pl
    # no LR folder (or one that lists nothing): the LR images are made from the HR images
    assert eval_folder_pairs({'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': None}) == (ph, None)
    empty = tmp_path / 'empty'
    empty.mkdir()
    assert eval_folder_pairs({'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': str(empty)}) == (ph, None)
    # mode LR: the LR folder alone
    assert eval_folder_pairs({'mode': 'LR', 'dataroot_HR': None, 'dataroot_LR': str(lr)}) == (None, pl)
    assert len(EvalFolderDataset({'mode': 'LR', 'dataroot_LR': str(lr)}, 4)) == 5
    # the reference's assertions
    with pytest.raises(AssertionError, match='Error: HR path is empty.'):
        eval_folder_pairs({'mode': 'LRHR', 'dataroot_HR': str(empty), 'dataroot_LR': str(lr)})
    with pytest.raises(AssertionError, match='Error: LR paths are empty.'):
        eval_folder_pairs({'mode': 'LR', 'dataroot_LR': str(empty)})
    os.remove(str(lr / '9.png'))
    with pytest.raises(AssertionError, match='HR and LR datasets have different number of images - 4, 5.'):
        eval_folder_pairs({'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': str(lr)})
    with pytest.raises(AssertionError, match='is not a valid directory'):
        eval_folder_pairs({'mode': 'LRHR', 'dataroot_HR': str(tmp_path / 'nope')})


def test_modcrop_geometry_for_every_remainder():
    from dasr_amd.data import modcrop_size
    for s in (2, 3, 4):
        for rh in range(s):
            for rw in range(s):
                H, W = 5 * s + rh, 7 * s + rw
                assert modcrop_size(H, W, s) == (5 * s, 7 * s)
    assert [modcrop_size(64 + r, 90 + q, 4) for r, q in ((0, 0), (1, 1), (2, 2), (3, 3))] == [(64, 88), (64, 88), (64, 92), (64, 92)]
    assert modcrop_size(1356, 2040, 4) == (1356, 2040) and modcrop_size(3, 3, 4) == (0, 0)
    # the window is the top-left one: what the reference's modcrop keeps of an array
    a = np.arange(11 * 14).reshape(11, 14)
    Hc, Wc = modcrop_size(11, 14, 4)
    assert np.array_equal(a[:Hc, :Wc], a[:11 - 11 % 4, :14 - 14 % 4])


@pytest.mark.parametrize('extra,what', [({'data_type': 'lmdb'}, 'lmdb'), ({'color': 'y'}, 'colour-space conversion'), ({'subset_file': '/x/list.txt'}, 'subset_file')])
def test_refused_options(tmp_path, extra, what):
    from dasr_amd.data import EvalFolderDataset
    (tmp_path / 'hr').mkdir()
    _png(tmp_path / 'hr' / 'a.png', 8, 8)
    for mode in ('LRHR', 'LR'):
        opt = {'mode': mode, 'dataroot_HR': str(tmp_path / 'hr'), 'dataroot_LR': str(tmp_path / 'hr'), 'phase': 'test', 'data_type': 'img', 'color': None,
               'subset_file': None}
        EvalFolderDataset(opt, 4)
        with pytest.raises(NotImplementedError, match=what) as e:
            EvalFolderDataset(dict(opt, **extra), 4)
        assert '\n' not in str(e.value)
    with pytest.raises(NotImplementedError):
        EvalFolderDataset({'mode': 'LRHR_wavelet_unpair_fake_weights_EQ', 'dataroot_HR': str(tmp_path / 'hr')}, 4)


def test_create_dataset_routes_folders_and_keeps_the_rest(tmp_path):
    from dasr_amd import train
    from dasr_amd.data import EvalFolderDataset
    (tmp_path / 'hr').mkdir()
    _png(tmp_path / 'hr' / 'a.png', 8, 8)
    opt = {'scale': 4, 'model': 'sr'}
    root = str(tmp_path / 'hr')
    for ds in ({'mode': 'LRHR', 'phase': 'val', 'dataroot_HR': root}, {'mode': 'LRHR', 'phase': 'test', 'dataroot_HR': root, 'dataroot_LR': root},
               {'mode': 'LR', 'phase': 'test', 'dataroot_LR': root}, {'mode': 'LR', 'dataroot_LR': root}):
        d = train.create_dataset(ds, opt)
        assert isinstance(d, EvalFolderDataset) and len(d) == 1 and d.scale == 4
    # what worked before returns what it returned; what did not work still says so
    assert isinstance(train.create_dataset({'mode': 'synthetic', 'phase': 'val'}, opt), train.SyntheticValDataset)
    assert isinstance(train.create_dataset({'mode': 'synthetic', 'phase': 'train', 'batch_size': 2, 'HR_size': 32}, opt), train.SyntheticDataset)
    with pytest.raises(NotImplementedError):
        train.create_dataset({'mode': 'LRHR', 'phase': 'train', 'dataroot_HR': root}, opt)
    with pytest.raises(NotImplementedError):
        train.create_dataset({'mode': 'LRHR_wavelet_unpair_fake_weights_EQ', 'phase': 'val'}, opt)


@pytest.mark.parametrize('n_in,s', [(24, 4), (52, 4), (40, 2), (27, 3)])
def test_tap_tables_scatter_to_the_resample_matrix(n_in, s):
    """the tables the device is fed with and the dense matrix of imresize_matlab are one computation: scattering the table gives the identical fp64 matrix"""
    from dasr_amd.data import _bicubic_resample_matrix, bicubic_taps
    j, w = bicubic_taps(n_in, 1.0 / s)
    assert j.shape == w.shape == (n_in // s, 4 * s + 2) and j.dtype == torch.int64 and w.dtype == torch.float64
    assert int(j.min()) >= 0 and int(j.max()) <= n_in - 1
    M = torch.zeros(n_in // s, n_in, dtype=torch.float64)
    for o in range(j.shape[0]):
        for t in range(j.shape[1]):
            M[o, int(j[o, t])] += w[o, t]
    assert torch.equal(M, _bicubic_resample_matrix(n_in, 1.0 / s))
    assert float((w.sum(1) - 1).abs().max()) < 1e-15
    # mirror rule at both ends: output 1 of a x1/4 table sits at u = 2.5 with a 16-wide kernel, so its taps start at the 1-based position floor(2.5 - 8) = -6, seven
    # samples over the edge, each mirrored with the edge sample repeated (-1 -> 0, -2 -> 1, ...); the last output is the mirror image
    if s == 4:
        n = n_in
        assert j[0].tolist()[:9] == [6, 5, 4, 3, 2, 1, 0, 0, 1] and j[-1].tolist()[-9:] == [n - 2, n - 1, n - 1, n - 2, n - 3, n - 4, n - 5, n - 6, n - 7]


def test_imgio_entry_points_are_bound_declared_built_and_documented():
    from dasr_amd import build, _lib
    new = ('dasr_u8_to_planar', 'dasr_imresize_down')
    hdr = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    declared = set(re.findall(r'^\s*int\s+(dasr_\w+)\s*\(', hdr, flags=re.M))
    assert 'imgio.hip' in build.SOURCES
    build.build()
    L = _lib.lib()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in new:
        assert name in _lib._SIGS and name in declared and hasattr(L, name), name
        assert '`%s`' % name in doc, name
    src = open(os.path.join(ROOT, 'dasr_amd', 'csrc', 'imgio.hip')).read()
    assert '#pragma clang fp contract(off)' in src and 'atomic' not in src.split('#include')[1]


def test_imgio_entry_points_reject_bad_arguments_before_any_launch():
    """DASR_EINVAL in front of the first HIP call (the non-null pointers stand for device addresses and are never dereferenced)"""
    from dasr_amd import _lib
    L = _lib.lib()
    p = 4096
    assert L.dasr_u8_to_planar(None, 8, 8, 8, 8, p, None) == EINVAL and L.dasr_u8_to_planar(p, 8, 8, 8, 8, None, None) == EINVAL
    assert L.dasr_u8_to_planar(p, 8, 8, 9, 8, p, None) == EINVAL and L.dasr_u8_to_planar(p, 8, 8, 8, 9, p, None) == EINVAL    # a window larger than the image
    assert L.dasr_u8_to_planar(p, 8, 8, 0, 8, p, None) == EINVAL and L.dasr_u8_to_planar(p, 0, 8, 0, 8, p, None) == EINVAL

    def down(C=3, H=24, W=36, s=4, ptrs=(p,) * 7):
        src, ih, wh, iw, ww, tmp, dst = ptrs
        return L.dasr_imresize_down(src, C, H, W, s, ih, wh, iw, ww, tmp, dst, None)
    for k in range(7):
        assert down(ptrs=tuple(None if i == k else p for i in range(7))) == EINVAL
    assert down(H=25) == EINVAL and down(W=37) == EINVAL                # not a multiple of s
    assert down(H=25, W=35, s=5) == EINVAL and down(s=1) == EINVAL and down(s=0) == EINVAL and down(H=24, W=40, s=8) == EINVAL
    assert down(C=0) == EINVAL and down(H=0) == EINVAL
