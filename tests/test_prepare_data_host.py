"""Host side of the dataset preparation and the reverse filter (dasr_amd/bicubic.py, prepare_data.py, backproject.reverse_filter_fp64, csrc/imgio.hip; reference:
codes/SRN/scripts/extract_subimgs_single.py, generate_mod_LR_bic.m, back_projection/main_reverse_filter.m): the entry points in header, binding and library; the window
grid against hand-stated expectations; what the CLI refuses, before it writes; the fp64 restatements.  No device."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'dasr_windows_down_u8': 16, 'dasr_imresize_up': 14}


def test_entry_points_in_header_binding_and_library():
    from dasr_amd import _lib, bicubic
    header = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert name in _lib._SIGS and len(_lib._SIGS[name]) == nargs, name
    assert re.search(r'^#define DASR_ABI_VERSION 22$', header, flags=re.M) and _lib.ABI_VERSION == 22
    defs = {k: int(v) for k, v in re.findall(r'^#define DASR_((?:WD|UP)_\w+) (\d+)$', header, flags=re.M)}
    assert (defs['WD_TILE_H'], defs['WD_TILE_W']) == bicubic.DOWN_TILE and (defs['UP_TILE_H'], defs['UP_TILE_W']) == bicubic.UP_TILE
    assert (defs['UP_F32'], defs['UP_F32_ACC'], defs['UP_U8']) == (bicubic.UP_F32, bicubic.UP_F32_ACC, bicubic.UP_U8)
    import ctypes
    assert ctypes.sizeof(_lib.WindowDesc) == 8   # dasr_window_desc: two int32
    from dasr_amd import build
    assert os.path.exists(build.build())
    L = _lib.lib()   # (binds every name of _SIGS: no device is touched)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    assert L.dasr_abi_version() == 22
    data = open(_lib.LIB_PATH, 'rb').read()
    assert b'windows_down_u8_kernel' in data and b'imresize_up_kernel' in data


def test_window_grid_of_a_div2k_image():
    """1356 x 2040 with 480 / 240 / 48: rows 0 .. 720 by 240 leave 156 > 48 pixels, so 876 is appended; columns 0 .. 1440 leave 120 > 48, so 1560 is appended"""
    from dasr_amd.prepare_data import axis_grid, window_grid
    assert axis_grid(1356, 480, 240, 48) == [0, 240, 480, 720, 876]
    assert axis_grid(2040, 480, 240, 48) == [0, 240, 480, 720, 960, 1200, 1440, 1560]
    grid = window_grid(1356, 2040, 480, 240, 48)
    assert len(grid) == 40
    assert grid[0] == (0, 0) and grid[1] == (0, 240) and grid[7] == (0, 1560) and grid[8] == (240, 0) and grid[39] == (876, 1560)   # row-major: _s001 .. _s040
    assert grid == sorted(grid)


def test_window_grid_appends_nothing_under_the_threshold():
    """1000 x 1000: 0, 240, 480 leave 1000 - 960 = 40 <= 48 pixels"""
    from dasr_amd.prepare_data import axis_grid, window_grid
    assert axis_grid(1000, 480, 240, 48) == [0, 240, 480]
    assert window_grid(1000, 1000, 480, 240, 48) == [(y, x) for y in (0, 240, 480) for x in (0, 240, 480)]
    assert axis_grid(480, 480, 240, 48) == [0]
    with pytest.raises(ValueError):
        window_grid(479, 1000, 480, 240, 48)


def _png(path, mode, size=(130, 100)):
    from PIL import Image
    rng = np.random.RandomState(3)
    shape = {'RGB': (size[1], size[0], 3), 'RGBA': (size[1], size[0], 4), 'L': (size[1], size[0]), 'P': (size[1], size[0])}[mode]
    a = rng.randint(0, 256, shape).astype(np.uint8)
    im = Image.fromarray(a, 'L' if mode == 'P' else mode)
    if mode == 'P':
        im = im.convert('P')
    im.save(str(path))


def _outputs(tmp_path):
    return [p for k in ('sub', 'mod', 'lr', 'bic') for p in (tmp_path / k).glob('*')]


def test_cli_refuses_before_it_writes(tmp_path):
    from dasr_amd import prepare_data as cli
    hr = tmp_path / 'HR'
    hr.mkdir()
    _png(hr / 'a.png', 'RGB')
    out = ['--sub_dir', str(tmp_path / 'sub'), '--mod_dir', str(tmp_path / 'mod'), '--lr_dir', str(tmp_path / 'lr'), '--bic_dir', str(tmp_path / 'bic')]
    small = ['--crop_sz', '48', '--step', '24', '--thres_sz', '8']

    def refused(argv, *words):
        with pytest.raises(ValueError) as e:
            cli.main(argv)
        assert all(w in str(e.value) for w in words), str(e.value)
        assert not _outputs(tmp_path)   # nothing was written
    refused(['--input_dir', str(hr)], 'no output folder')
    refused(['--input_dir', str(hr), '--scale', '5'] + out, '--scale')
    refused(['--input_dir', str(hr)] + out, 'a.png', 'crop_sz')            # 100 x 130 under the default crop_sz 480
    for mode in ('L', 'P', 'RGBA'):
        bad = hr / ('b_%s.png' % mode)
        _png(bad, mode)
        refused(['--input_dir', str(hr)] + small + out, bad.name, 'RGB')   # a.png in front of it is fine: nothing of it was written either
        bad.unlink()
    (tmp_path / 'lr').mkdir()
    (tmp_path / 'lr' / 'old.png').write_bytes(b'x')
    with pytest.raises(ValueError) as e:
        cli.main(['--input_dir', str(hr)] + small + out)
    assert '--lr_dir' in str(e.value) and '--overwrite' in str(e.value)
    assert sorted(p.name for p in _outputs(tmp_path)) == ['old.png'] and (tmp_path / 'lr' / 'old.png').read_bytes() == b'x'
    empty = tmp_path / 'empty'
    empty.mkdir()
    (tmp_path / 'lr' / 'old.png').unlink()
    refused(['--input_dir', str(empty)] + out, 'no PNG files')


def test_plan_lists_units_without_decoding(tmp_path):
    from dasr_amd import prepare_data as cli
    hr = tmp_path / 'HR'
    hr.mkdir()
    _png(hr / 'b.png', 'RGB')
    _png(hr / 'a.png', 'RGB')
    o = cli.parse_args(['--input_dir', str(hr), '--sub_dir', str(tmp_path / 'sub'), '--crop_sz', '48', '--step', '24', '--thres_sz', '8'])
    dirs, files = cli.plan(o)
    assert dirs == {'sub': str(tmp_path / 'sub')} and [f[1] for f in files] == ['a', 'b']
    # 100 rows: 0, 24, 48 leave 4 <= 8; 130 columns: 0, 24, 48, 72 leave 10 > 8, so 82 is appended
    assert files[0][2:4] == (100, 130) and files[0][4] == [(y, x) for y in (0, 24, 48) for x in (0, 24, 48, 72, 82)] and files[0][5] == (48, 48)
    o = cli.parse_args(['--input_dir', str(hr), '--lr_dir', str(tmp_path / 'lr'), '--scale', '3'])
    _, files = cli.plan(o)
    assert files[0][4] == [(0, 0)] and files[0][5] == (100, 130)
    assert not (tmp_path / 'sub').exists() and not (tmp_path / 'lr').exists()


def test_upsample_fp64_matches_the_reference(golden_dir):
    """bicubic.upsample_fp64 against the reference's imresize_np(x, s, True) (tests/golden/imresize_up.npz).  Bound 1e-6, as tests/test_back_projection_host.py states it
    for data.imresize_matlab on the same fixture (the reference forms its weights and sums in float32; the fixture stores float32)."""
    from dasr_amd.bicubic import upsample_fp64
    z = np.load(os.path.join(golden_dir, 'imresize_up.npz'))
    n = len([k for k in z.files if k.startswith('in')])
    assert n >= 8
    for i in range(n):
        x, s = torch.from_numpy(z['in%d' % i]).permute(2, 0, 1).double(), int(z['scale%d' % i])
        want = z['out%d' % i].astype(np.float64)
        got3 = upsample_fp64(x, s)
        got4 = upsample_fp64(x[None].float().double(), s)
        assert got3.dtype == torch.float64 and tuple(got4.shape) == (1, 3, s * x.shape[1], s * x.shape[2])
        err = float(np.abs(got3.permute(1, 2, 0).numpy() - want).max())
        print('upsample_fp64 %s x%d: %.2e' % (tuple(x.shape[1:]), s, err))
        assert err <= 1e-6 and torch.equal(got4[0], got3)


def test_quantise_is_matlabs_im2uint8():
    from dasr_amd.bicubic import quantise
    x = torch.tensor([-0.2, 0.0, 0.4999 / 255, 0.5 / 255, 1.5 / 255, 254.4 / 255, 1.0, 1.7], dtype=torch.float64)
    assert quantise(x).tolist() == [0, 0, 0, 1, 2, 254, 255, 255] and quantise(x).dtype == torch.uint8


def test_down_windows_fp64_mirrors_at_the_window_edge():
    """an interior window gives what the same pixels give as an image of their own, and not the crop of the whole image's LR image"""
    from dasr_amd.bicubic import down_windows_fp64
    img = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (40, 52, 3)).astype(np.uint8))
    u8, f64 = down_windows_fp64(img, [(8, 12), (0, 0)], (16, 24), 4)
    assert tuple(u8.shape) == (2, 4, 6, 3) and tuple(f64.shape) == (2, 3, 4, 6) and u8.dtype == torch.uint8
    own_u8, own_f64 = down_windows_fp64(img[8:24, 12:36].contiguous(), [(0, 0)], (16, 24), 4)
    assert torch.equal(f64[0], own_f64[0]) and torch.equal(u8[0], own_u8[0])
    _, whole = down_windows_fp64(img, [(0, 0)], (40, 52), 4)
    assert float((whole[0][:, 2:6, 3:9] - f64[0]).abs().max()) > 1e-3
    with pytest.raises(ValueError):
        down_windows_fp64(img, [(30, 0)], (16, 24), 4)   # 30 + 16 > 40
    with pytest.raises(ValueError):
        down_windows_fp64(img, [(0, 0)], (15, 24), 4)


def test_reverse_filter_fp64_literal_form_equals_the_device_form():
    """main_reverse_filter.m:21 as it stands, out + (J - up(down(out))) with J = up(lr) formed once, against out + up(lr - down(out)), the form the device runs: the
    up-sampling is linear, so the two differ by fp64 rounding only.  Bound: down(out) is the same computation in both; per iteration the forms differ in three
    up-samplings (up(lr) and up(down) against up(lr - down)), each a sum of 6 x 6 products whose absolute weights sum to at most 1.25^2 = 1.5625 (error at most
    38 x 2^-53 x 1.5625 x the largest input magnitude), and three elementwise roundings: (3 x 38 x 1.5625 + 3) x 2^-53 < 182 x 2^-53 per unit of magnitude.  The inputs
    of the up-samplings are lr, down(out) and their difference, at most 2 M with M the largest magnitude among lr and the result; the iteration is taken not to
    amplify earlier differences (as the 20-iteration bound of the back-projection test does).  Total: iters x 2 x 182 x 2^-53 x max(1, M)."""
    from dasr_amd.backproject import reverse_filter_fp64
    from dasr_amd.data import imresize_matlab
    g = torch.Generator().manual_seed(21)
    s, iters = 4, 20
    hr = torch.rand(3, 8, 12, generator=g, dtype=torch.float64)
    lr = imresize_matlab(hr, 1.0 / s)
    sr = hr + 0.05 * torch.randn(hr.shape, generator=g, dtype=torch.float64)
    lit = reverse_filter_fp64(sr, lr, iters)
    dev = reverse_filter_fp64(sr, lr, iters, literal=False)
    assert lit.dtype == torch.float64 and tuple(lit.shape) == (3, 8, 12)
    M = max(1.0, float(lr.abs().max()), float(lit.abs().max()))
    err, bound = float((lit - dev).abs().max()), iters * 2 * 182 * 2.0 ** -53 * M
    print('reverse_filter_fp64 literal vs up(lr - down): max difference %.3e, bound %.3e' % (err, bound))
    assert err <= bound
    # one iteration by hand, the batched form, and iters = 0
    one = sr + (imresize_matlab(lr, 4.0) - imresize_matlab(imresize_matlab(sr, 0.25), 4.0))
    assert torch.equal(reverse_filter_fp64(sr, lr, 1), one)
    assert torch.equal(reverse_filter_fp64(sr[None], lr[None], 1)[0], one)
    assert torch.equal(reverse_filter_fp64(sr, lr, 0), sr)
    assert float((lit - sr).abs().max()) > 1e-3   # the filter moves the image
    with pytest.raises(ValueError):
        reverse_filter_fp64(sr, lr[:, :, :2], 1)
