"""GPU: data.EvalFolderDataset behind the evaluation CLI (`python -m dasr_amd.test`) and the validation pass of the training driver, on folders of PNG files built
here with PIL.  Model: `model: sr`, RRDB_net nf 32 nb 1, seeded weights loaded from `pretrain_model_G`.  Every CLI run is a fresh process (as a user starts it).

What the folder run is compared with is the same run fed through `loaders=` with batch dicts built on the HOST (load_image + crop, imresize_matlab): the device input
stage is bit-equal to the host one for image files, so PNG files and numbers must be identical; the LR image made on the device is within one fp32 unit (2^-23) of
the host-made one (bound derived in tests/test_gpu_imgio.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((67, 90), (64, 64), (50, 76))      # HR sizes with remainders 3 / 2, 0 / 0 and 2 / 0 modulo 4
ULP = 2.0 ** -23


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def _seeded_generator(tmp_path):
    from oracle import fixtures, nets
    net = nets.RRDBNet(3, 3, 32, 1, 4)
    g_path = tmp_path / 'seeded_G.pth'
    torch.save(fixtures.seeded_state_dict(net.state_dict(), 3, 0.1), g_path)
    return g_path


def _smooth_png(path, h, w, seed):
    """an 8-bit image with structure (smooth field + noise), so that PSNR / SSIM are ordinary numbers"""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, h // 8 + 2, w // 8 + 2, generator=g), size=(h, w), mode='bilinear', align_corners=False)[0]
    img = (base + 0.05 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(str(path))


def _folders(tmp_path, sizes=SIZES, with_lr=True):
    """HR PNGs and, for each, the LR image imresize_matlab makes of the cropped HR on the host, saved as .npy (no 8-bit rounding of the LR)"""
    from dasr_amd.data import imresize_matlab, load_image
    hr, lr = tmp_path / 'HR', tmp_path / 'LR'
    hr.mkdir()
    lr.mkdir()
    for i, (h, w) in enumerate(sizes):
        _smooth_png(hr / ('img_%02d.png' % i), h, w, 100 + i)
        if with_lr:
            t = load_image(str(hr / ('img_%02d.png' % i)))
            t = t[:, :h - h % 4, :w - w % 4].contiguous()
            np.save(str(lr / ('img_%02d.npy' % i)), imresize_matlab(t, 0.25).numpy())
    return hr, lr


def _opt(tmp_path, name, g_path, datasets, extra=None, train=False):
    opt = {'name': name, 'use_tb_logger': False, 'model': 'sr', 'scale': 4, 'gpu_ids': [0], 'chop': False, 'val_lpips': False, 'datasets': datasets,
           'path': {'root': str(tmp_path), 'pretrain_model_G': str(g_path)},
           'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 32, 'nb': 1, 'in_nc': 3, 'out_nc': 3, 'gc': 32}}
    if train:
        opt['train'] = {'lr_G': 2e-4, 'weight_decay_G': 0, 'beta1_G': 0.9, 'lr_scheme': 'MultiStepLR', 'lr_steps': [100], 'lr_gamma': 0.5,
                        'pixel_criterion': 'l1', 'pixel_weight': 1.0, 'manual_seed': 0, 'niter': 2, 'val_freq': 1}
        opt['logger'] = {'print_freq': 1, 'save_checkpoint_freq': 4}
    opt.update(extra or {})
    p = tmp_path / (name + '.json')
    p.write_text(json.dumps(opt))
    return str(p)


# the CLI in a child process; HOST_LOADERS: the same datasets as batch dicts built on the host and passed through `loaders=`
_CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
import torch
from dasr_amd import test as dtest
kept = []
ev = dtest.evaluate
def wrapped(*a, **k):
    r = ev(*a, **k)
    kept.append({k2: list(v) for k2, v in r.items()})
    return r
dtest.evaluate = wrapped
loaders = None
if %(host)r:
    from dasr_amd.data import image_paths, load_image
    def host_items(hr_root, lr_root, scale=4):
        for ph, pl in zip(image_paths(hr_root), image_paths(lr_root)):
            hr = load_image(ph)
            hr = hr[:, :hr.shape[1] - hr.shape[1] %% scale, :hr.shape[2] - hr.shape[2] %% scale].contiguous()
            yield {'LR': load_image(pl)[None], 'HR': hr[None], 'LR_path': [pl], 'HR_path': [ph]}
    loaders = [(name, list(host_items(h, l))) for name, h, l in %(host)r]
summary = dtest.main(['-opt', %(opt)r], loaders=loaders)
json.dump({'summary': summary, 'per_image': kept}, open(%(out)r, 'w'))
'''


def _child(code, timeout=600):
    p = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    return p.stdout.decode()


def _run_cli(tmp_path, name, g_path, datasets, extra=None, host=None):
    out = tmp_path / (name + '_result.json')
    log = _child(_CHILD % {'root': ROOT, 'opt': _opt(tmp_path, name, g_path, datasets, extra), 'out': str(out), 'host': host})
    res = json.load(open(out))
    pngs = {}
    for ds in datasets.values():
        imgs = tmp_path / 'results' / name / ds['name'] / 'imgs'
        pngs[ds['name']] = {f: (imgs / f).read_bytes() for f in sorted(os.listdir(imgs))}
    return res, pngs, log


def _png_size(data):
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return im.size[1], im.size[0]


@pytest.mark.parametrize('device_metrics', [False, True])
def test_cli_on_lrhr_folders_equals_the_run_on_host_built_batches(tmp_path, device_metrics):
    """(a) `mode: "LRHR"` with two folders.  On the parent of this change create_dataset raises NotImplementedError for this option file."""
    _gpu()
    g_path = _seeded_generator(tmp_path)
    hr, lr = _folders(tmp_path)
    datasets = {'test_1': {'name': 'folderset', 'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': str(lr)}}
    extra = {'device_metrics': True} if device_metrics else None
    f_res, f_png, f_log = _run_cli(tmp_path, 'folder_run', g_path, datasets, extra)
    h_res, h_png, _ = _run_cli(tmp_path, 'host_run', g_path, datasets, extra, host=[('folderset', str(hr), str(lr))])
    assert sorted(f_png['folderset']) == ['img_00.png', 'img_01.png', 'img_02.png']
    assert f_png == h_png                                                      # PNG files identical
    assert [_png_size(f_png['folderset']['img_%02d.png' % i]) for i in range(3)] == [(h - h % 4, w - w % 4) for h, w in SIZES]
    fi, hi = f_res['per_image'][0], h_res['per_image'][0]
    for k in ('psnr', 'ssim', 'psnr_y', 'ssim_y'):                             # the four numbers per image: equal
        assert len(fi[k]) == 3 and fi[k] == hi[k], (k, fi[k], hi[k])
        assert all(np.isfinite(v) for v in fi[k])
    assert f_res['summary'] == h_res['summary'] and set(f_res['summary']['folderset']) == {'psnr', 'ssim', 'psnr_y', 'ssim_y'}
    assert sum('PSNR_Y' in l and 'img_0' in l for l in f_log.splitlines()) == 3


def test_cli_on_an_hr_folder_alone_makes_the_lr_images_on_the_device(tmp_path, margins):
    """(b) no dataroot_LR: LR = dasr_imresize_down of the cropped HR, within 2^-23 of the host-made image; LR_path is the HR path; one PNG per HR file"""
    dev = _gpu()
    from dasr_amd import train
    from dasr_amd.data import EvalFolderDataset, imresize_matlab, load_image
    g_path = _seeded_generator(tmp_path)
    hr, _ = _folders(tmp_path, with_lr=False)
    ds_opt = {'name': 'hronly', 'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': None, 'phase': 'test', 'data_type': 'img'}
    ds = train.create_dataset(dict(ds_opt), {'scale': 4, 'model': 'sr'})
    assert isinstance(ds, EvalFolderDataset) and len(ds) == 3
    items = list(ds)
    assert len(items) == 3
    for item, (h, w) in zip(items, SIZES):
        assert item['LR_path'] == item['HR_path'] and len(item['HR_path']) == 1 and os.path.dirname(item['HR_path'][0]) == str(hr)
        host_hr = load_image(item['HR_path'][0])[:, :h - h % 4, :w - w % 4].contiguous()
        assert item['HR'].is_cuda and item['HR'].dtype == torch.float32 and tuple(item['HR'].shape) == (1, 3, h - h % 4, w - w % 4)
        assert torch.equal(item['HR'][0].cpu(), host_hr)                       # bit for bit load_image + modcrop
        host_lr = imresize_matlab(host_hr, 0.25)
        assert item['LR'].is_cuda and tuple(item['LR'].shape) == (1, 3, h // 4, w // 4)
        err = float((item['LR'][0].cpu().double() - host_lr.double()).abs().max())
        margins('EvalFolderDataset LR made on the device vs imresize_matlab, HR %d x %d: max abs %.3e (bound 2^-23 = %.3e)' % (h, w, err, ULP))
        assert err <= ULP, (h, w, err)
    res, png, log = _run_cli(tmp_path, 'hronly_run', g_path, {'test_1': {k: v for k, v in ds_opt.items() if k not in ('phase', 'data_type')}})
    assert sorted(png['hronly']) == ['img_00.png', 'img_01.png', 'img_02.png']
    assert len(res['per_image'][0]['psnr']) == 3 and all(np.isfinite(v) for v in res['per_image'][0]['psnr'] + res['per_image'][0]['ssim_y'])


def test_cli_on_an_lr_folder_writes_images_and_no_metrics(tmp_path):
    """(c) `mode: "LR"`: PNGs of 4 x the input size, one name line per image, no metric lines, empty summary"""
    _gpu()
    g_path = _seeded_generator(tmp_path)
    lr = tmp_path / 'LRonly'
    lr.mkdir()
    sizes = ((17, 23), (16, 16))
    for i, (h, w) in enumerate(sizes):
        _smooth_png(lr / ('lr_%02d.png' % i), h, w, 7 + i)
    res, png, log = _run_cli(tmp_path, 'lr_run', g_path, {'test_1': {'name': 'lrset', 'mode': 'LR', 'dataroot_HR': None, 'dataroot_LR': str(lr)}})
    assert sorted(png['lrset']) == ['lr_00.png', 'lr_01.png']
    assert [_png_size(png['lrset']['lr_%02d.png' % i]) for i in range(2)] == [(4 * h, 4 * w) for h, w in sizes]
    assert res['summary'] == {} and all(v == [] for v in res['per_image'][0].values())
    assert 'PSNR' not in log.split('Testing [lrset]')[1] and 'SSIM' not in log.split('Testing [lrset]')[1]


def test_training_driver_validates_on_lrhr_folders(tmp_path):
    """(d) `python -m dasr_amd.train`, two iterations on the synthetic train set, val_freq 1, `datasets.val` an LRHR folder pair: the validation images of both
    passes are written and each pass logs one `# Validation # PSNR` line"""
    _gpu()
    g_path = _seeded_generator(tmp_path)
    hr, lr = _folders(tmp_path)
    datasets = {'train': {'name': 'syn', 'mode': 'synthetic', 'batch_size': 4, 'HR_size': 64, 'n_batches': 8},
                'val': {'name': 'folderval', 'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': str(lr)}}
    opt = _opt(tmp_path, 'train_folder_val', g_path, datasets, train=True)
    log = _child('import sys\nsys.path.insert(0, %r)\nfrom dasr_amd import train\ntrain.main([\'-opt\', %r])\n' % (ROOT, opt))
    val = [l for l in log.splitlines() if '# Validation # PSNR' in l]
    assert len(val) == 2, log[-3000:]
    assert all(np.isfinite(float(l.split('PSNR:')[1])) and float(l.split('PSNR:')[1]) > 0 for l in val)
    root = tmp_path / 'experiments' / 'train_folder_val' / 'val_images'
    got = sorted(str(f.relative_to(root)) for f in root.rglob('*.png'))
    assert got == sorted('img_%02d/img_%02d_%d.png' % (i, i, step) for i in range(3) for step in (1, 2))


def test_mismatched_pair_sizes_raise_value_error_naming_both_files(tmp_path):
    """(e) both folders given and the cropped HR is not scale x the LR size"""
    _gpu()
    from dasr_amd.data import EvalFolderDataset
    hr, lr = tmp_path / 'HR', tmp_path / 'LR'
    hr.mkdir()
    lr.mkdir()
    _smooth_png(hr / 'a.png', 67, 90, 1)      # cropped: 64 x 88
    _smooth_png(lr / 'a.png', 16, 22, 2)
    _smooth_png(hr / 'b.png', 64, 64, 3)
    _smooth_png(lr / 'b.png', 16, 17, 4)      # 64 x 68 expected of the HR
    ds = EvalFolderDataset({'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': str(lr), 'phase': 'val'}, 4)
    ok = ds.item(0)
    assert tuple(ok['HR'].shape) == (1, 3, 64, 88) and tuple(ok['LR'].shape) == (1, 3, 16, 22)
    with pytest.raises(ValueError) as e:
        ds.item(1)
    assert str(hr / 'b.png') in str(e.value) and str(lr / 'b.png') in str(e.value)


def test_cli_on_folders_with_chop_and_val_lpips(tmp_path):
    """the loops of test.evaluate need no change for the quadrant inference (`chop`) and the LPIPS column (`val_lpips`, seeded network by explicit opt-in):
    same folders, device metrics, four numbers and the LPIPS value per image, PSNR close to the run without chop"""
    _gpu()
    g_path = _seeded_generator(tmp_path)
    hr, lr = _folders(tmp_path, sizes=((192, 160), (163, 170)))      # LR sides of 40 and more: the quadrants' 20-pixel overlap needs them
    datasets = {'test_1': {'name': 'folderset', 'mode': 'LRHR', 'dataroot_HR': str(hr), 'dataroot_LR': str(lr)}}
    plain, _, _ = _run_cli(tmp_path, 'plain_run', g_path, datasets, {'device_metrics': True})
    res, png, log = _run_cli(tmp_path, 'chop_lpips_run', g_path, datasets, {'chop': True, 'val_lpips': True, 'allow_random_perceptual': True, 'device_metrics': True})
    assert sorted(png['folderset']) == ['img_00.png', 'img_01.png']
    pi = res['per_image'][0]
    assert len(pi['lpips']) == 2 and all(np.isfinite(v) for v in pi['lpips'] + pi['psnr'] + pi['ssim_y'])
    assert all(abs(a - b) < 1.0 for a, b in zip(pi['psnr'], plain['per_image'][0]['psnr']))
    assert np.isfinite(res['summary']['folderset']['lpips'])
