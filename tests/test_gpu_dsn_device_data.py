"""GPU: `--device_data` -- dasr_gather_crops_u8 and dasr_crops_bicubic_down through ctypes, the device datasets and loader against the host datasets of
dasr_amd/dsn_data.py (which tests/test_dsn_data.py pins to the reference), and the training driver with the flag.  Never against the device code itself.

Bounds.  dasr_gather_crops_u8: bit-equal to the host transform of the same window (one correctly rounded fp32 division on either side, everything else is indexing).
dasr_crops_bicubic_down against the fp64 evaluation (resize_matrix in float64, rows first, then columns, clamp): 2^-23, the bound tests/test_gpu_imgio.py holds
dasr_imresize_down to -- both sides add the same fp64 products in a different order (a few 1e-16 apart) and the device rounds once to fp32; results lie in [0, 1],
where neighbouring fp32 numbers are at most 2^-24 apart, so 2^-23 leaves a factor two.  Against the host's fp32 imresize: e_host + 2^-23, e_host being the largest
distance of the host result from the same fp64 evaluation on the same crops, computed here (triangle inequality; the host multiplies fp32 matrices)."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda', torch.cuda.current_device())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _png(path, h, w, seed):
    from PIL import Image
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)).save(str(path))


def host_transform(a, y0, x0, crop, vflip, hflip, k, sub_y, sub_x, size):
    """the torch operations of dsn_data.load_augmented_crop + random_crop on the decoded uint8 array `a`"""
    img = torch.from_numpy(np.ascontiguousarray(a[y0:y0 + crop, x0:x0 + crop])).permute(2, 0, 1).float().div_(255.0)
    if vflip:
        img = img.flip(1)
    if hflip:
        img = img.flip(2)
    img = torch.rot90(img, k, (1, 2))
    return img[:, sub_y:sub_y + size, sub_x:sub_x + size].contiguous()


def fp64_down(x):
    """[..., c, c] -> (clamped, unclamped) fp64 evaluation of imresize(., 1/4, True): rows first, then columns"""
    from dasr_amd.dsn_data import resize_matrix
    R = resize_matrix(x.shape[-1], 0.25, True, torch.float64)
    y = torch.matmul(torch.matmul(R, x.double()), R.t())
    return y.clamp(0, 1), y


def device_down(dev, x):
    """dasr_crops_bicubic_down of the host tensor x [n, 3, c, c]: [n, 3, c/4, c/4] on the host"""
    from dasr_amd import _lib
    from dasr_amd.data import bicubic_taps
    n, _, c, _ = x.shape
    j, w = bicubic_taps(c, 0.25)
    j, w = j.to(torch.int32).contiguous().to(dev), w.contiguous().to(dev)
    src = x.contiguous().to(dev)
    dst = torch.full((n, 3, c // 4, c // 4), -7.0, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dasr_crops_bicubic_down(src.data_ptr(), n, c, 4, j.data_ptr(), w.data_ptr(), dst.data_ptr(), _st()), 'dasr_crops_bicubic_down')
    return dst.cpu()


@pytest.mark.parametrize('H,W,crop', [(37, 53, 32), (32, 32, 32), (61, 45, 20)])
def test_gather_crops_u8_is_bit_equal_to_the_host_transform_for_all_16_flag_cases(H, W, crop):
    """odd image sizes, windows touching every edge of the image (and one in the middle), clean-crop form (size == crop) and source-crop form (size == crop / 4 at
    sub-origins touching every edge of the crop)"""
    dev = _gpu()
    from dasr_amd import _lib
    a = np.random.RandomState(H * W).randint(0, 256, (H, W, 3), dtype=np.uint8)
    a[0, 0], a[-1, -1] = (0, 1, 255), (254, 128, 127)
    src = torch.from_numpy(a).to(dev)
    small = crop // 4
    origins = sorted({(0, 0), (0, W - crop), (H - crop, 0), (H - crop, W - crop), ((H - crop) // 2, (W - crop) // 2)})
    subs = [(0, 0), (0, crop - small), (crop - small, 0), (crop - small, crop - small), (3, 5)]
    for size, sub_list in ((crop, [(0, 0)]), (small, subs)):
        cases = [(y0, x0, v, h, k, sy, sx) for (y0, x0) in origins for v in (0, 1) for h in (0, 1) for k in range(4) for (sy, sx) in sub_list]
        descs = (_lib.CropU8Desc * len(cases))()
        for d, (y0, x0, v, h, k, sy, sx) in zip(descs, cases):
            d.src, d.H, d.W, d.y0, d.x0, d.crop, d.flags, d.sub_y, d.sub_x = src.data_ptr(), H, W, y0, x0, crop, v | (h << 1) | (k << 2), sy, sx
        dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        dst = torch.full((len(cases), 3, size, size), -7.0, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().dasr_gather_crops_u8(dd.data_ptr(), len(cases), size, dst.data_ptr(), _st()), 'dasr_gather_crops_u8')
        got = dst.cpu()
        assert len({c[2:5] for c in cases}) == 16
        for i, (y0, x0, v, h, k, sy, sx) in enumerate(cases):
            want = host_transform(a, y0, x0, crop, v, h, k, sy, sx, size)
            assert torch.equal(got[i], want), (H, W, crop, size, cases[i])


def test_gather_crops_u8_all_byte_values():
    dev = _gpu()
    from dasr_amd import _lib
    a = np.arange(16 * 16 * 3, dtype=np.int64).reshape(16, 16, 3) % 256
    a = a.astype(np.uint8)
    src = torch.from_numpy(a).to(dev)
    d = (_lib.CropU8Desc * 1)()
    d[0].src, d[0].H, d[0].W, d[0].y0, d[0].x0, d[0].crop, d[0].flags, d[0].sub_y, d[0].sub_x = src.data_ptr(), 16, 16, 0, 0, 16, 0, 0, 0
    dd = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(dev)
    dst = torch.empty((1, 3, 16, 16), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dasr_gather_crops_u8(dd.data_ptr(), 1, 16, dst.data_ptr(), _st()), 'dasr_gather_crops_u8')
    assert set(a.reshape(-1).tolist()) == set(range(256))
    assert torch.equal(dst.cpu()[0], torch.from_numpy(a).permute(2, 0, 1).float().div_(255.0))


def _step_edges(n, c, seed):
    """crops in [0, 1] with hard 0 / 1 edges (bicubic overshoot on both sides of every edge) next to random texture"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, c, c, generator=g)
    x[:, :, : c // 2, : c // 3] = 0.0
    x[:, :, : c // 2, c // 3: 2 * c // 3] = 1.0
    x[:, :, c // 3:c // 2, :] = (torch.arange(c) // 5 % 2).float()          # stripes, five samples wide
    x[:, 1] = x[:, 1].transpose(1, 2).clone()
    return x


@pytest.mark.parametrize('n,c', [(8, 256), (3, 260), (2, 64), (1, 12), (1, 1024)])
def test_bicubic_down_is_within_one_fp32_unit_of_the_fp64_evaluation(n, c, margins):
    """tile edges inside the crop (c / 4 not a multiple of the 4 output rows of a tile: 260, 12), the smallest side that has all 18 taps mirrored on both ends (12),
    the largest side (1024: the whole LDS budget); step edges so that the clamp works on both sides"""
    dev = _gpu()
    x = _step_edges(n, c, c + n)
    want, raw = fp64_down(x)
    if c >= 64:   # (a side of 12 is three output samples of a 16-wide kernel: nothing overshoots)
        assert float(raw.max()) > 1.0 and float(raw.min()) < 0.0             # some unclamped fp64 values do leave [0, 1]: the clamp works on both sides
    got = device_down(dev, x)
    err = float((got.double() - want).abs().max())
    margins('crops_bicubic_down vs fp64, %d crops of %d: max abs %.3e (bound 2^-23 = %.3e); unclamped range [%.4f, %.4f]' % (n, c, err, ULP, float(raw.min()),
                                                                                                                              float(raw.max())))
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert err <= ULP


def test_bicubic_down_against_the_host_fp32_imresize(margins):
    dev = _gpu()
    from dasr_amd.dsn_data import imresize
    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.rand(4, 3, 256, 256, generator=g), _step_edges(4, 256, 12)])
    want64, _ = fp64_down(x)
    host = torch.stack([imresize(t, 0.25, True) for t in x])
    e_host = float((host.double() - want64).abs().max())
    got = device_down(dev, x)
    err = float((got.double() - host.double()).abs().max())
    margins('crops_bicubic_down vs host fp32 imresize, 8 crops of 256: max abs %.3e; e_host (host vs fp64) %.3e; bound e_host + 2^-23 = %.3e' % (err, e_host, e_host + ULP))
    assert err <= e_host + ULP


def test_bicubic_down_two_runs_give_identical_bits():
    dev = _gpu()
    x = _step_edges(8, 256, 5)
    assert torch.equal(device_down(dev, x), device_down(dev, x))


def _folders(tmp_path):
    """seeded PNGs of mixed sizes: 7 source, 4 clean, 3 validation pairs"""
    dirs = {}
    sizes = {'src': [(140, 150), (128, 128), (131, 177), (150, 129), (128, 200), (137, 137), (160, 128)], 'tgt': [(140, 132), (128, 128), (201, 135), (129, 160)],
             'vhr': [(130, 150), (128, 128), (141, 135)], 'vlr': [(36, 40), (32, 32), (40, 37)]}
    for k, (sub, sz) in enumerate(sizes.items()):
        d = tmp_path / sub
        d.mkdir()
        for i, (h, w) in enumerate(sz):
            _png(d / ('%02d.png' % i), h, w, 100 * k + i)
        dirs[sub] = str(d)
    return dirs


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _check_bicubic(got, host, hr, margins, what):
    want64, _ = fp64_down(hr.cpu())
    e_host = float((host.double() - want64).abs().max())
    err64, err = float((got.cpu().double() - want64).abs().max()), float((got.cpu().double() - host.double()).abs().max())
    margins('%s: bicubic vs fp64 %.3e (bound %.3e), vs host %.3e (bound e_host + 2^-23 = %.3e)' % (what, err64, ULP, err, e_host + ULP))
    assert err64 <= ULP and err <= e_host + ULP


@pytest.mark.parametrize('world,rank', [(1, 0), (2, 1)])
def test_device_loader_gives_the_batches_of_the_host_loader(tmp_path, world, rank, margins):
    dev = _gpu()
    from dasr_amd import dsn_data
    dirs = _folders(tmp_path)
    kw = dict(crop_size=128, upscale_factor=4, flips=True, rotations=True)
    host_set = dsn_data.TrainDeresnetDataset(dirs['src'], dirs['tgt'], cropped=True, **kw)
    host_loader = dsn_data.make_loader(host_set, 3 * world, True, 0, seed=4, rank=rank, world=world)
    dev_set = dsn_data.DeviceTrainDeresnet(dirs['src'], dirs['tgt'], device=dev, threads=4, **kw)
    dev_loader = dsn_data.DeviceDeresnetLoader(dev_set, 3, dsn_data.ShardSampler(len(dev_set), True, 4, rank, world))
    _seed(21)
    host_batches = [[b for b in host_loader] for _ in range(2)]
    _seed(21)
    dev_batches = [[b for b in dev_loader] for _ in range(2)]
    per_epoch = 7 if world == 1 else 3
    for ep in range(2):
        assert len(host_batches[ep]) == len(dev_batches[ep]) == len(dev_loader) == (per_epoch + 2) // 3
        assert [b[0].shape[0] for b in dev_batches[ep]] == [b[0].shape[0] for b in host_batches[ep]]
        assert dev_batches[ep][-1][0].shape[0] == per_epoch - 3 * (len(dev_batches[ep]) - 1)        # 7 items: 3 + 3 + 1, the short last batch
        for i, ((hr, bic, real), (hhr, hbic, hreal)) in enumerate(zip(dev_batches[ep], host_batches[ep])):
            assert hr.device == dev and bic.device == dev and real.device == dev and hr.dtype == bic.dtype == real.dtype == torch.float32
            assert hr.shape == hhr.shape and bic.shape == hbic.shape and real.shape == hreal.shape
            assert torch.equal(hr.cpu(), hhr) and torch.equal(real.cpu(), hreal)
            _check_bicubic(bic, hbic, hr, margins, 'world %d rank %d epoch %d batch %d' % (world, rank, ep, i))


def test_device_validation_set_gives_the_items_of_the_host_set(tmp_path, margins):
    dev = _gpu()
    from dasr_amd import dsn_data
    dirs = _folders(tmp_path)
    host_loader = dsn_data.make_loader(dsn_data.ValDeresnetDataset(dirs['vhr'], 4, lr_dir=dirs['vlr'], crop_size_val=128), 1, False, 0)
    dev_set = dsn_data.DeviceValDeresnet(dirs['vhr'], 4, lr_dir=dirs['vlr'], crop_size_val=128, device=dev)
    _seed(8)
    host_items = list(host_loader)
    _seed(8)
    dev_items = list(dev_set)
    assert len(host_items) == len(dev_items) == len(dev_set) == 3
    for i, (d, h) in enumerate(zip(dev_items, host_items)):
        assert [tuple(t.shape) for t in d] == [tuple(t.shape) for t in h] and all(t.device == dev for t in d)
        assert torch.equal(d[0].cpu(), h[0]) and torch.equal(d[2].cpu(), h[2]) and torch.equal(d[3].cpu(), h[3])
        _check_bicubic(d[1], h[1], d[0], margins, 'validation item %d' % i)
    # without the cap on the crop: the side comes from the image (141 x 135 -> 132, two sizes -> one tap table per size)
    host_set = dsn_data.ValDeresnetDataset(dirs['vhr'], 4, lr_dir=dirs['vlr'], crop_size_val=None)
    dev_set = dsn_data.DeviceValDeresnet(dirs['vhr'], 4, lr_dir=dirs['vlr'], crop_size_val=None, device=dev)
    _seed(9)
    h = host_set[2]
    _seed(9)
    d = dev_set[2]
    assert tuple(d[0].shape) == (3, 132, 132) and torch.equal(d[0].cpu(), h[0]) and torch.equal(d[2].cpu(), h[2]) and torch.equal(d[3].cpu(), h[3])
    _check_bicubic(d[1], h[1], d[0], margins, 'validation item 2 at its own size')
    dev_set[1]
    assert sorted(dev_set._down._tables) == [128, 132]


def test_dsn_train_cli_with_device_data(tmp_path):
    _gpu()
    import json
    import yaml
    from dasr_amd import dsn_train, tb_writer
    dirs = _folders(tmp_path)
    paths = tmp_path / 'paths.yml'
    paths.write_text(yaml.safe_dump({'aim2019': {'tdsr': {'source': dirs['src'], 'target': dirs['tgt'], 'valid_hr': dirs['vhr'], 'valid_lr': dirs['vlr']}}}))
    save = str(tmp_path / 'exp')
    m = dsn_train.main(['--dataset', 'aim2019', '--artifacts', 'tdsr', '--paths', str(paths), '--device_data', '--debug', '--batch_size', '4', '--crop_size', '128',
                        '--crop_size_val', '128', '--val_interval', '1', '--val_img_interval', '5', '--save_model_interval', '1', '--flips', '--rotations',
                        '--num_workers', '3', '--filter', 'wavelet', '--allow_random_perceptual', '--save_path', save])
    assert m.epoch == 2 and m.iteration_count == 4                      # 7 source images / batch 4 -> 2 iterations per epoch (the second one short)
    assert os.path.exists(os.path.join(save, 'checkpoints', 'iteration_4.tar')) and os.path.exists(os.path.join(save, 'checkpoints', 'last_iteration.tar'))
    assert json.load(open(os.path.join(save, 'commandline_args.txt')))['device_data'] is True
    ev = tb_writer.read_events([os.path.join(save, 'logs', f) for f in os.listdir(os.path.join(save, 'logs'))][0])
    tags = {}
    for step, tag, val in ev:
        tags.setdefault(tag, []).append((step, val))
    losses = [k for k in tags if k.startswith('loss/')]
    assert losses and 'val/psnr' in tags
    for k in losses + ['val/mse', 'val/psnr']:
        assert [s for s, _ in tags[k]] == [2, 4] and all(np.isfinite(v) for _, v in tags[k]), (k, tags[k])
