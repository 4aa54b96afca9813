"""GPU: the drivers that write their images with the device PNG encoder -- the option key `"device_png": true` of `python -m dasr_amd.test` and of the validation pass of
`python -m dasr_amd.train`, `python -m dasr_amd.back_projection --device_png` and `python -m dasr_amd.dsn_create_dataset --device_png` -- against the files, scores and log
lines of their default path.  Every driver run is a fresh child process with a time limit (independent runs of one comparison side by side); the files are compared by
their decoded pixels (the device files carry no LZ77 matches, their bytes differ from PIL's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_metrics import _CHILD, _opt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE = 'device_png: SR images are encoded on the device (csrc/png.hip)'
CLI_NOTE = 'encoded on the device'
TIME_LIMIT = 300


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


def _children(codes):
    """every code string in a fresh python process, all at once; their outputs (stdout and stderr together), in order"""
    procs = [subprocess.Popen([sys.executable, '-c', 'import sys\nsys.path.insert(0, %r)\n' % ROOT + c], cwd=ROOT, env=dict(os.environ), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for c in codes]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=TIME_LIMIT)[0].decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-3000:]
    return outs


def _main(module, argv):
    return 'from dasr_amd import %s\n%s.main(%r)\n' % (module, module, [str(a) for a in argv])


def _pixels(folder, mode='RGB'):
    """{relative path: (mode, pixels)} of every PNG file under folder"""
    from PIL import Image
    out = {}
    for f in sorted(folder.rglob('*.png')):
        with Image.open(str(f)) as im:
            assert im.format == 'PNG' and im.mode == mode, f
            out[str(f.relative_to(folder))] = np.array(im)
    return out


def _same(a, b):
    assert a.keys() == b.keys() and a
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _seeded_generator(tmp_path, nc=3):
    from oracle import fixtures, nets
    g_path = tmp_path / 'seeded_G.pth'
    torch.save(fixtures.seeded_state_dict(nets.RRDBNet(nc, nc, 32, 1, 4).state_dict(), 3, 0.1), g_path)
    return g_path


def _with_key(opt_file, device_png, **extra):
    opt = json.load(open(opt_file))
    if device_png is not None:
        opt['device_png'] = device_png
    opt.update(extra)
    json.dump(opt, open(opt_file, 'w'))
    return opt_file


def test_evaluation_cli_four_ways(tmp_path):
    """`device_png` on / off x `device_metrics` on / off: the same file names and pixels everywhere; the summaries and the per-image scores of a `device_metrics` setting are
    EQUAL with and without the key (the scores are formed from the same bytes by the same code); the note is logged once with the key and never without it"""
    _gpu()
    g_path = _seeded_generator(tmp_path)
    ways = [(png, met) for met in (False, True) for png in (False, True)]
    codes, names = [], []
    for png, met in ways:
        name = 'eval_png%d_met%d' % (png, met)
        names.append(name)
        opt = _with_key(_opt(tmp_path, name, False, g_path, met), True if png else None)
        codes.append(_CHILD % {'root': ROOT, 'opt': opt, 'out': str(tmp_path / (name + '.json'))})
    logs = _children(codes)
    runs = {}
    for way, name, log in zip(ways, names, logs):
        assert log.count(NOTE) == (1 if way[0] else 0), (way, log[-2000:])
        assert ('device_metrics: SR images are quantised' in log) == way[1]
        runs[way] = (json.load(open(str(tmp_path / (name + '.json')))), _pixels(tmp_path / 'results' / name / 'synset' / 'imgs'))
    base = runs[(False, False)]
    assert len(base[1]) == 3 and len(base[0]['per_image'][0]['psnr']) == 3
    for way in ways[1:]:
        _same(base[1], runs[way][1])
    for met in (False, True):
        assert runs[(True, met)][0] == runs[(False, met)][0], met           # summary and per-image lists, exact
        assert set(runs[(True, met)][0]['summary']['synset']) == {'psnr', 'ssim', 'psnr_y', 'ssim_y'}


def test_key_with_chop_self_ensemble_back_projection_and_lpips(tmp_path):
    _gpu()
    g_path = _seeded_generator(tmp_path)
    full = {'chop': True, 'self_ensemble': True, 'back_projection': 2, 'val_lpips': True, 'allow_random_perceptual': True}
    codes, names = [], []
    for png in (False, True):
        for met in (False, True):
            name = 'full_png%d_met%d' % (png, met)
            names.append(name)
            opt = _with_key(_opt(tmp_path, name, False, g_path, met), True if png else None, **full)
            codes.append(_CHILD % {'root': ROOT, 'opt': opt, 'out': str(tmp_path / (name + '.json'))})
    _children(codes)
    res = [json.load(open(str(tmp_path / (n + '.json')))) for n in names]
    pix = [_pixels(tmp_path / 'results' / n / 'synset' / 'imgs') for n in names]
    assert res[0] == res[2] and res[1] == res[3] and 'lpips' in res[2]['summary']['synset'] and len(res[2]['per_image'][0]['lpips']) == 3
    for p in pix[1:]:
        _same(pix[0], p)


def test_one_validation_round_of_the_trainer(tmp_path):
    """the same PNG pixels under val_images and the same logged PSNR line; with the key and without `device_metrics` the image is read back once for util.host_scores"""
    _gpu()
    g_path = _seeded_generator(tmp_path)
    names = ['train_host', 'train_png']
    codes = [_main('train', ['-opt', _with_key(_opt(tmp_path, n, True, g_path, False), True if n == 'train_png' else None)]) for n in names]
    logs = _children(codes)
    val, pix = [], []
    for n, log in zip(names, logs):
        val.append([l.split(' - INFO: ')[-1] for l in log.splitlines() if '# Validation # PSNR' in l])
        pix.append(_pixels(tmp_path / 'experiments' / n / 'val_images'))
        assert log.count(NOTE) == (1 if n == 'train_png' else 0)
    assert len(val[0]) == 1 and val[0] == val[1], val
    assert len(pix[0]) == 2
    _same(pix[0], pix[1])


_GREY_CHILD = r'''
import json, torch
from dasr_amd import test as dtest
g = torch.Generator().manual_seed(5)
pairs = []
for i in range(2):
    hr = torch.nn.functional.interpolate(torch.rand(1, 1, 8, 8, generator=g), size=(96, 96), mode='bilinear', align_corners=False).clamp(0, 1)
    pairs.append({'LR': torch.nn.functional.avg_pool2d(hr, 4), 'HR': hr, 'LR_path': ['grey/g_%%03d.png' %% i], 'HR_path': ['grey/g_%%03d.png' %% i]})
summary = dtest.main(['-opt', %(opt)r], loaders=[('greyset', pairs)])
json.dump(summary, open(%(out)r, 'w'))
'''


def test_one_channel_model_writes_grey_files(tmp_path):
    _gpu()
    g_path = _seeded_generator(tmp_path, nc=1)
    names = ['grey_host', 'grey_png']
    codes = []
    for n in names:
        opt_file = _opt(tmp_path, n, False, g_path, True)
        opt = json.load(open(opt_file))
        opt['network_G'].update(in_nc=1, out_nc=1)
        json.dump(opt, open(opt_file, 'w'))
        codes.append(_GREY_CHILD % {'opt': _with_key(opt_file, True if n == 'grey_png' else None), 'out': str(tmp_path / (n + '.json'))})
    _children(codes)
    pix = [_pixels(tmp_path / 'results' / n / 'greyset' / 'imgs', mode='L') for n in names]
    assert len(pix[0]) == 2 and all(v.shape == (96, 96) for v in pix[0].values())
    _same(pix[0], pix[1])
    res = [json.load(open(str(tmp_path / (n + '.json')))) for n in names]
    assert res[0] == res[1] and set(res[0]['greyset']) == {'psnr', 'ssim'}


def test_back_projection_cli(tmp_path):
    """three pairs at LR 16 x 16, 10 x 6 and 13 x 9, scales 4, 2 and 3"""
    _gpu()
    from PIL import Image
    from dasr_amd.png import photo
    lr_dir, sr_dir = tmp_path / 'LR', tmp_path / 'SR'
    lr_dir.mkdir()
    sr_dir.mkdir()
    for k, ((h, w), s) in enumerate((((16, 16), 4), ((10, 6), 2), ((13, 9), 3))):
        Image.fromarray(photo(h, w, 70 + k)).save(str(lr_dir / ('p%d.png' % k)))
        Image.fromarray(photo(s * h, s * w, 80 + k)).save(str(sr_dir / ('p%d.png' % k)))
    base = ['--lr_dir', lr_dir, '--sr_dir', sr_dir, '--iters', '5', '--num_workers', '2']
    logs = _children([_main('back_projection', base + ['--out_dir', tmp_path / 'host']), _main('back_projection', base + ['--out_dir', tmp_path / 'dev', '--device_png'])])
    assert [l.count(CLI_NOTE) for l in logs] == [0, 1]
    host, dev = _pixels(tmp_path / 'host'), _pixels(tmp_path / 'dev')
    assert sorted(host) == ['p0.png', 'p1.png', 'p2.png'] and [host['p%d.png' % k].shape for k in range(3)] == [(64, 64, 3), (20, 12, 3), (39, 27, 3)]
    _same(host, dev)
    assert not np.array_equal(host['p0.png'], np.array(Image.open(str(sr_dir / 'p0.png'))))   # the images were moved


def test_dsn_create_dataset_cli(tmp_path):
    """the checkpoint as the CLI test of tests/test_gpu_dsn.py makes it; fake LR images of --dataset synthetic --n_synthetic 2"""
    _gpu()
    save = tmp_path / 'dsn'
    _children([_main('dsn_train', ['--debug', '--batch_size', '2', '--crop_size', '128', '--filter', 'wavelet', '--save_path', save, '--save_model_interval', '1',
                                   '--no_per_loss', '--dataset', 'synthetic'])])
    ck = save / 'checkpoints' / 'last_iteration.tar'
    assert ck.exists()
    base = ['--checkpoint', ck, '--filter', 'wavelet', '--out_root', tmp_path / 'res', '--dataset', 'synthetic', '--n_synthetic', '2', '--including_source_ddm']
    logs = _children([_main('dsn_create_dataset', base + ['--name', 'host']), _main('dsn_create_dataset', base + ['--name', 'dev', '--device_png'])])
    assert [l.count(CLI_NOTE) for l in logs] == [0, 1]
    host, dev = _pixels(tmp_path / 'res' / 'host' / 'imgs_from_target'), _pixels(tmp_path / 'res' / 'dev' / 'imgs_from_target')
    assert sorted(host) == ['target_000.png', 'target_001.png'] and host['target_000.png'].shape == (40, 48, 3)
    _same(host, dev)
    for sub, n in (('ddm_target', 2), ('ddm_source', 2)):
        files = sorted(os.listdir(str(tmp_path / 'res' / 'host' / sub)))
        assert len(files) == n and files == sorted(os.listdir(str(tmp_path / 'res' / 'dev' / sub)))
        for f in files:
            assert (tmp_path / 'res' / 'host' / sub / f).read_bytes() == (tmp_path / 'res' / 'dev' / sub / f).read_bytes(), f


def test_file_writer_device_and_host_mode(tmp_path):
    """7 x 5 x 3, a 39 x 27 window of a 64 x 64 x 3 tensor (row pitch 192 bytes for rows of 81) and 20 x 12 grey: the device mode writes the files of png.encode_batch,
    through write_many (one batch) and through three write calls; the host mode reads the tensors back and writes the same pixels"""
    _gpu()
    from dasr_amd import png
    dev = torch.device('cuda')
    big = torch.from_numpy(png.photo(64, 64, 2)).to(dev)
    colour = [torch.from_numpy(png.photo(7, 5, 1)).to(dev), big[11:50, 20:47]]
    grey = torch.from_numpy(np.ascontiguousarray(png.photo(20, 12, 3)[:, :, 1])).to(dev)
    assert colour[1].stride(0) == 192 and tuple(colour[1].shape) == (39, 27, 3)
    want = png.encode_batch(colour) + png.encode_batch([grey], fmt='grey')
    names = ['a.png', 'window.png', 'grey.png']

    def run(folder, device, many):
        folder.mkdir()
        paths = [str(folder / n) for n in names]
        with png.FileWriter(device, 2, note=None) as w:
            if many:
                w.write_many(colour, paths[:2])
            else:
                w.write(colour[0], paths[0])
                w.write(colour[1], paths[1])
            w.write(grey, paths[2], 'grey')
        assert w.paths == paths
        return [open(p, 'rb').read() for p in paths]
    assert run(tmp_path / 'many', True, True) == want
    assert run(tmp_path / 'single', True, False) == want
    from PIL import Image

    def decoded(folder):
        out = []
        for n in names:
            with Image.open(str(folder / n)) as im:
                assert im.format == 'PNG'
                out.append((im.mode, np.array(im)))
        return out
    dev_files = decoded(tmp_path / 'many')
    assert [(m, a.shape) for m, a in dev_files] == [('RGB', (7, 5, 3)), ('RGB', (39, 27, 3)), ('L', (20, 12))]
    for (_, a), t in zip(dev_files, colour + [grey]):
        assert np.array_equal(a, t.cpu().numpy())
    for many in (True, False):
        run(tmp_path / ('host%d' % many), False, many)
        for (m, a), (hm, ha) in zip(dev_files, decoded(tmp_path / ('host%d' % many))):
            assert m == hm and np.array_equal(a, ha)
