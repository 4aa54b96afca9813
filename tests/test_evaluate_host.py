"""CPU: the folder evaluator (dasr_amd/dsn_evaluate.py, metrics.pair_metrics_u8, csrc/metrics.hip, dasr_lpips_s2d_any) as far as it goes without a GPU -- the
C ABI lists the new entry points and refuses bad arguments before it launches anything, the block grid of the any-size LPIPS input stage follows the first
conv's output size, the CLI pairs and crops files as codes/DSN/evaluate.py:25-43 does, and the two host formulas agree with numpy on the arrays themselves."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dasr_img_ssim_box', 'dasr_img_channel_sums', 'dasr_lpips_s2d_any')
EINVAL = -22


def test_evaluator_entry_points_are_bound_declared_exported_and_documented():
    from dasr_amd import build, _lib
    hdr = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    declared = set(re.findall(r'^\s*int\s+(dasr_\w+)\s*\(', hdr, flags=re.M))
    for name in NEW:
        assert name in _lib._SIGS and name in declared, name
    assert _lib.ABI_VERSION == 22 and '#define DASR_ABI_VERSION 22' in hdr
    assert build.SOURCES == ['conv.hip', 'resblock.hip', 'wgrad.hip', 'misc.hip', 'gan.hip', 'lpips.hip', 'metrics.hip', 'imgio.hip', 'rccl.hip']
    build.build()
    L = _lib.lib()
    assert L.dasr_abi_version() == 22
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert hasattr(L, name) and '`%s`' % name in doc, name
    # the recorded form of the any-size input stage: appended at the end of the slot-layout table, the older op codes unchanged
    assert _lib.OP_LPIPS_S2D_ANY == 54 == max(_lib.OP_ARGS) and list(_lib.OP_ARGS)[-1] == _lib.OP_LPIPS_S2D_ANY and _lib.OP_LPIPS_S2D == 35
    assert 'DASR_OP_LPIPS_S2D_ANY = 54' in hdr


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    """checked in front of the first HIP call, so this runs without a device; the non-null pointers are never dereferenced"""
    from dasr_amd import _lib
    L = _lib.lib()
    p, ws = 4096, 1 << 20   # p stands for a device address
    assert L.dasr_img_ws_bytes(1, 3, 7, 7, 0) >= 3 * 8 and L.dasr_img_ws_bytes(1, 3, 7, 32768, 0) >= 3 * 512 * 8   # covers the box SSIM where the 11 x 11 one has no region
    assert L.dasr_img_ws_bytes(2, 3, 64, 64, 4) >= 2 * 3 * 56 * 8                                                 # and the channel sums
    box = lambda a=p, b=p, N=1, Cc=3, H=64, W=64, crop=4, out=p, w=p, size=ws: L.dasr_img_ssim_box(a, b, N, Cc, H, W, crop, out, w, size, None)
    chan = lambda a=p, N=1, Cc=3, H=64, W=64, crop=4, out=p, w=p, size=ws: L.dasr_img_channel_sums(a, N, Cc, H, W, crop, out, w, size, None)
    for bad in (dict(a=None), dict(b=None), dict(out=None), dict(w=None), dict(N=0), dict(N=-1), dict(Cc=2), dict(Cc=4), dict(H=14), dict(W=14),   # cropped side 6
                dict(crop=-1), dict(crop=32), dict(size=8), dict(size=3 * 8 - 1, H=15, W=15)):
        assert box(**bad) == EINVAL, bad
    for bad in (dict(a=None), dict(out=None), dict(w=None), dict(N=0), dict(N=-1), dict(Cc=2), dict(crop=32), dict(crop=-1), dict(size=8),
                dict(size=3 * 56 * 8 - 1)):
        assert chan(**bad) == EINVAL, bad
    T, Z, h = _lib.Tensor(p, 1 << 20, 1 << 16), _lib.Tensor(None, 0, 0), (C.c_float * 4)(1, 1, 1, 0)
    s2d = lambda x=T, N=1, H=33, W=46, sc=h, sh=h, y=T: L.dasr_lpips_s2d_any(x, N, H, W, sc, sh, y, None)
    for bad in (dict(x=Z), dict(y=Z), dict(sc=None), dict(sh=None), dict(N=0), dict(N=-2), dict(H=30), dict(W=30), dict(H=0), dict(W=-5)):
        assert s2d(**bad) == EINVAL, bad
    # the older entry point keeps its refusal of sizes that are no multiple of 4
    assert L.dasr_lpips_s2d(T, 1, 33, 46, h, h, T, 0, None) == EINVAL


def test_block_grid_rule_is_the_first_convs_output_size_plus_two():
    from dasr_amd.lpips import s2d_grid, MIN_SIDE
    w = torch.zeros(1, 3, 11, 11)
    for n in range(31, 49):
        out = torch.nn.functional.conv2d(torch.zeros(1, 3, n, 31), w, stride=4, padding=2).shape[2]
        assert s2d_grid(n) == out + 2, n
        if n % 4 == 0:
            assert s2d_grid(n) == n // 4 + 1
        # the grid covers every padded row the conv reads: output o reads padded rows 4 o .. 4 o + 10 = blocks o .. o + 2
        assert 4 * (out - 1) + 10 <= n + 3 and 4 * s2d_grid(n) >= 4 * (out - 1) + 11
    assert MIN_SIDE == 31
    for n in (8, 12, 64, 128, 512):
        assert s2d_grid(n) == (n + 4) // 4   # what the plans of the trainers have always used


def test_tensor2img_of_byte_over_255_gives_the_byte_back():
    """metrics.u8_planes makes the planar bytes from the planar fp32 image with dasr_tensor2img_u8: rint(float32(u / 255) * 255) == u for all 256 bytes"""
    u = np.arange(256, dtype=np.float32)
    q = (u / np.float32(255.0)) * np.float32(255.0)
    assert q.dtype == np.float32 and np.array_equal(np.rint(q).astype(np.uint8), np.arange(256, dtype=np.uint8))


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(str(path))


def _bytes(seed, *shape):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def test_cli_pairs_and_crops_files_like_the_reference(tmp_path):
    from dasr_amd import dsn_evaluate as E
    res, gt = tmp_path / 'res', tmp_path / 'gt'
    res.mkdir()
    gt.mkdir()
    a = {n: _bytes(i, 40, 52, 4) for i, n in enumerate(('b.png', 'a.png', 'c.png'))}      # RGBA results
    g = {n: _bytes(10 + i, 44, 56, 3) for i, n in enumerate(('b.png', 'a.png', 'c.png'))}  # larger RGB ground truth
    for n in a:
        _png(res / n, a[n])
        _png(gt / n, g[n])
    (res / 'notes.txt').write_text('not an image')
    pairs = E.list_pairs(str(res), str(gt))
    assert [(os.path.basename(x), os.path.basename(y)) for x, y in pairs] == [('a.png', 'a.png'), ('b.png', 'b.png'), ('c.png', 'c.png')]
    for f, gf in pairs:
        n = os.path.basename(f)
        img, gti = E.load_pair(f, gf, border=4)
        assert img.dtype == np.uint8 and gti.dtype == np.uint8 and img.shape == gti.shape == (40, 52, 3)
        assert np.array_equal(img, a[n][..., :3]) and np.array_equal(gti, g[n][:40, :52, :])   # evaluate.py:35-40
    # equal sizes: nothing is cut
    _png(gt / 'a.png', g['a.png'][:40, :52])
    img, gti = E.load_pair(str(res / 'a.png'), str(gt / 'a.png'))
    assert np.array_equal(gti, g['a.png'][:40, :52])
    # unequal file counts: a ValueError (the deliberate deviation), naming both folders
    _png(gt / 'd.png', g['a.png'])
    with pytest.raises(ValueError) as e:
        E.list_pairs(str(res), str(gt))
    assert str(res) in str(e.value) and str(gt) in str(e.value)
    with pytest.raises(ValueError):
        E.list_pairs(str(tmp_path), str(tmp_path))   # no image files at all


def test_cli_refuses_files_it_cannot_score_and_names_them(tmp_path):
    from dasr_amd import dsn_evaluate as E
    rgb, small, grey, rgba = str(tmp_path / 'rgb.png'), str(tmp_path / 'small.png'), str(tmp_path / 'grey.png'), str(tmp_path / 'rgba.png')
    _png(rgb, _bytes(1, 40, 52, 3))
    _png(small, _bytes(2, 40, 51, 3))
    _png(grey, _bytes(3, 40, 52))
    _png(rgba, _bytes(4, 40, 52, 4))

    def refused(*args, **kw):
        with pytest.raises(ValueError) as e:
            E.load_pair(*args, **kw)
        return str(e.value)
    assert grey in refused(grey, rgb)                        # result not RGB / RGBA
    assert grey in refused(rgb, grey)                        # ground truth not RGB
    assert rgba in refused(rgb, rgba)                        # RGBA is accepted on the result side only
    msg = refused(rgb, small)                                # ground truth smaller than its result on one axis
    assert rgb in msg and small in msg
    assert rgb in refused(rgb, rgb, border=5)                # 30 x 42 left: under 31 x 31 with LPIPS
    E.load_pair(rgb, rgb, border=5, lpips=False)
    E.load_pair(rgb, rgb, border=4)                          # 32 x 44
    assert rgb in refused(rgb, rgb, border=17, lpips=False)  # 6 x 18 left: under the 7 x 7 window
    E.load_pair(small, rgb, border=16, lpips=False)          # 8 x 19
    assert rgb in refused(rgb, rgb, border=-1)


def test_cli_flags():
    from dasr_amd import dsn_evaluate as E
    o = E.parse_args(['--dir', 'x', '--gt_dir', 'y'])
    assert (o.dir, o.gt_dir, o.border_crop, o.lpips_alexnet, o.lpips_lin, o.allow_random_perceptual, o.num_workers) == ('x', 'y', None, None, None, False, 6)
    o = E.parse_args(['--dir', 'x', '--gt_dir', 'y', '--border_crop', '4', '--lpips_alexnet', 'a.pth', '--lpips_lin', 'l.pth', '--allow_random_perceptual',
                      '--num_workers', '3'])
    assert (o.border_crop, o.lpips_alexnet, o.lpips_lin, o.allow_random_perceptual, o.num_workers) == (4, 'a.pth', 'l.pth', True, 3)


def test_host_formulas_against_numpy_on_the_arrays():
    """psnr from the integer squared-error sum and psnr_col from the integer channel sums, against evaluate.py:44-45 restated with numpy in double"""
    from dasr_amd import metrics
    for seed, (h, w) in enumerate(((40, 52), (7, 7), (61, 45))):
        a = _bytes(seed, h, w, 3)
        b = np.clip(a.astype(np.int64) + np.random.RandomState(100 + seed).randint(-20, 21, size=a.shape) + np.array([3, -2, 5]), 0, 255).astype(np.uint8)
        d = a.astype(np.int64) - b.astype(np.int64)
        sse = int((d * d).sum())
        mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)               # compare_psnr on uint8: data range 255
        assert abs(metrics.psnr_from_sse(sse, a.size) - 10 * np.log10(255.0 ** 2 / mse)) < 1e-12
        assert metrics.psnr_from_sse(sse, a.size) == 10.0 * math.log10(255.0 ** 2 / (sse / a.size))
        ca, cb = a.mean(1).mean(0) / 255., b.mean(1).mean(0) / 255.                       # compare_psnr on float vectors in [0, 1]: data range 1
        want = 10 * np.log10(1.0 / np.mean((ca - cb) ** 2))
        sa, sb = [int(v) for v in a.reshape(-1, 3).sum(0, dtype=np.int64)], [int(v) for v in b.reshape(-1, 3).sum(0, dtype=np.int64)]
        assert abs(metrics.psnr_col_from_sums(sa, sb, h * w) - want) < 1e-9
    assert metrics.psnr_from_sse(0, 100) == float('inf') and metrics.psnr_col_from_sums([5, 6, 7], [5, 6, 7], 4) == float('inf')


def test_pair_metrics_refuses_what_it_cannot_score_without_a_device():
    from dasr_amd import metrics
    a = torch.zeros(3, 16, 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        metrics.pair_metrics_u8(a, a, border=5)          # 6 x 6 left
    with pytest.raises(TypeError):
        metrics.pair_metrics_u8(a.float(), a.float())
    with pytest.raises(TypeError):
        metrics.pair_metrics_u8(a, a[:, :15])
    from dasr_amd._lib import DasrHipError
    with pytest.raises(DasrHipError):
        metrics.pair_metrics_u8(a, a)                    # host tensors: an error, not a quiet host evaluation
