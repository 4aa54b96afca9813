"""GPU: `"resident_u8": true` of the SRN training datasets -- dasr_gather_srn_u8 and dasr_crops_down4_u8 through ctypes, the two datasets on PNG folders against
their own fp32 store (which tests/test_gpu_data.py pins to the reference's dataset class), and the training driver with and without the key.

Bounds.  dasr_gather_srn_u8: bit-equal to numpy indexing on the bytes (one correctly rounded fp32 division on either side, everything else is indexing).
dasr_crops_down4_u8 against the crop + augment of dasr_imresize_down(dasr_u8_to_planar(image)): bit-equal -- the same fp64 products added in the same order from the
same fp32 samples and rounded once; the two older kernels are the yardstick (tests/test_gpu_imgio.py holds them to the fp64 reference).  Against the host's
imresize_matlab: 2^-23 absolute -- each side is ONE rounding to fp32 of an fp64 evaluation of the same sum (orders differ: a few 1e-16) whose value is below 2 in
magnitude (the weights' absolute values sum to under 1.5, samples in [0, 1]), where neighbouring fp32 numbers are at most 2^-23 apart."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda', torch.cuda.current_device())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bytes(h, w, seed):
    a = np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)
    a[0, 0], a[-1, -1], a[0, -1], a[-1, 0] = (0, 1, 255), (254, 128, 127), (255, 255, 0), (3, 2, 1)
    return a


def _png(path, h, w, seed):
    from PIL import Image
    Image.fromarray(_bytes(h, w, seed)).save(str(path))


def _upload(descs, dev):
    return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)


def augment_np(win, flags):
    """util.augment on an [h, w, c] window: hflip (bit 0), vflip (bit 1), transpose (bit 2), in that order"""
    if flags & 1:
        win = win[:, ::-1]
    if flags & 2:
        win = win[::-1]
    if flags & 4:
        win = win.transpose(1, 0, 2)
    return win


def augment_t(x, flags):
    """the same on a [c, h, w] tensor"""
    if flags & 1:
        x = x.flip(2)
    if flags & 2:
        x = x.flip(1)
    if flags & 4:
        x = x.transpose(1, 2)
    return x.contiguous()


def test_gather_srn_u8_is_bit_equal_to_numpy_indexing_for_mixed_sizes_and_all_flags():
    """two non-square images, windows of 12 and 20 in ONE launch (144 samples: under one block; 400: two blocks, the second partly masked), at every corner of the
    image and in the middle, all eight flag values, one descriptor left zeroed in the middle of the block"""
    dev = _gpu()
    from dasr_amd import _lib
    images = [_bytes(37, 53, 1), _bytes(41, 29, 2)]
    srcs = [torch.from_numpy(a).to(dev) for a in images]
    cases = []
    for size in (12, 20):
        for i, a in enumerate(images):
            H, W = a.shape[:2]
            for (y0, x0) in ((0, 0), (0, W - size), (H - size, 0), (H - size, W - size), ((H - size) // 2, (W - size) // 3)):
                for flags in range(8):
                    cases.append((i, y0, x0, size, flags))
    random.Random(5).shuffle(cases)                     # sizes mixed inside the launch
    cases.insert(len(cases) // 2, None)                 # a zeroed descriptor
    slot = 3 * 20 * 20
    dst = torch.full((len(cases), slot), -7.0, dtype=torch.float32, device=dev)
    descs = (_lib.SrnU8Desc * len(cases))()
    for k, c in enumerate(cases):
        if c is not None:
            i, y0, x0, size, flags = c
            d = descs[k]
            d.src, d.H, d.W, d.y0, d.x0, d.size, d.flags, d.dst = srcs[i].data_ptr(), images[i].shape[0], images[i].shape[1], y0, x0, size, flags, dst[k].data_ptr()
    dd = _upload(descs, dev)
    _lib.check(_lib.lib().dasr_gather_srn_u8(dd.data_ptr(), len(cases), 20, _st()), 'dasr_gather_srn_u8')
    got = dst.cpu()
    assert {c[4] for c in cases if c} == set(range(8)) and {c[3] for c in cases if c} == {12, 20}
    for k, c in enumerate(cases):
        if c is None:
            assert bool((got[k] == -7.0).all())
            continue
        i, y0, x0, size, flags = c
        win = augment_np(images[i][y0:y0 + size, x0:x0 + size], flags)
        want = torch.from_numpy(np.ascontiguousarray(win.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0))
        assert torch.equal(got[k, :3 * size * size].view(3, size, size), want), c
        assert bool((got[k, 3 * size * size:] == -7.0).all()), c        # a smaller window is masked: nothing written behind it


_DOWN_REF = {}


def _down_ref(dev, a):
    """(device yardstick, host imresize_matlab) of the whole image `a` (uint8 [H, W, 3]): [3, H / 4, W / 4] each, computed once per image"""
    key = a.shape[:2]
    if key not in _DOWN_REF:
        from dasr_amd import _lib
        from dasr_amd.data import bicubic_taps, imresize_matlab
        H, W = key
        L = _lib.lib()
        u8 = torch.from_numpy(a).to(dev)
        planar = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        _lib.check(L.dasr_u8_to_planar(u8.data_ptr(), H, W, H, W, planar.data_ptr(), _st()), 'dasr_u8_to_planar')
        (jh, wh), (jw, ww) = ([t.contiguous().to(dev) for t in (j.to(torch.int32), w)] for j, w in (bicubic_taps(H, 0.25), bicubic_taps(W, 0.25)))
        tmp = torch.empty((3, H // 4, W), dtype=torch.float64, device=dev)
        lr = torch.empty((3, H // 4, W // 4), dtype=torch.float32, device=dev)
        _lib.check(L.dasr_imresize_down(planar.data_ptr(), 3, H, W, 4, jh.data_ptr(), wh.data_ptr(), jw.data_ptr(), ww.data_ptr(), tmp.data_ptr(), lr.data_ptr(), _st()),
                   'dasr_imresize_down')
        host = imresize_matlab(torch.from_numpy(a.astype(np.float32) / np.float32(255.0)).permute(2, 0, 1).contiguous(), 0.25)
        _DOWN_REF[key] = (lr.cpu(), host)
    return _DOWN_REF[key]


@pytest.mark.parametrize('H,W,size', [(36, 52, 5), (32, 32, 8), (96, 112, 20)])
def test_crops_down4_u8_is_bit_equal_to_the_crop_of_the_whole_image_resize(H, W, size, margins):
    """36 x 52: the LR image is 9 x 13, windows of 5 at its four corners and inside; 32 x 32 with a window of 8: the whole LR image, both mirrored borders of either
    axis in one window; 96 x 112 with windows of 20: four tiles per window, three of them partial.  All eight flags each."""
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.data import down4_weights
    a = _bytes(H, W, H + W)
    a[:H // 2, :W // 3], a[:H // 2, W // 3:2 * W // 3] = 0, 255          # hard edges: the resize overshoots [0, 1] and nothing clamps it
    want_dev, want_host = _down_ref(dev, a)
    h, w = H // 4, W // 4
    origins = sorted({(0, 0), (0, w - size), (h - size, 0), (h - size, w - size), ((h - size) // 2, (w - size) // 2)})
    cases = [(y0, x0, flags) for (y0, x0) in origins for flags in range(8)]
    src = torch.from_numpy(a).to(dev)
    dst = torch.full((len(cases), 3, size, size), -7.0, dtype=torch.float32, device=dev)
    descs = (_lib.SrnU8Desc * len(cases))()
    for k, (y0, x0, flags) in enumerate(cases):
        d = descs[k]
        d.src, d.H, d.W, d.y0, d.x0, d.size, d.flags, d.dst = src.data_ptr(), H, W, y0, x0, size, flags, dst[k].data_ptr()
    dd = _upload(descs, dev)
    _lib.check(_lib.lib().dasr_crops_down4_u8(dd.data_ptr(), C.addressof(descs), len(cases), size, C.addressof(down4_weights()), _st()), 'dasr_crops_down4_u8')
    got = dst.cpu()
    worst = 0.0
    for k, (y0, x0, flags) in enumerate(cases):
        assert torch.equal(got[k], augment_t(want_dev[:, y0:y0 + size, x0:x0 + size], flags)), (H, W, size, cases[k])
        worst = max(worst, float((got[k].double() - augment_t(want_host[:, y0:y0 + size, x0:x0 + size], flags).double()).abs().max()))
    margins('crops_down4_u8 vs host imresize_matlab, image %d x %d, windows of %d: max abs %.3e (bound 2^-23 = %.3e); range of the resize [%.4f, %.4f]' % (
        H, W, size, worst, ULP, float(want_host.min()), float(want_host.max())))
    assert worst <= ULP


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _folders(tmp_path, n=6):
    """HR 40 x 56, LR 10 x 14 (fake and real), domain-distance maps 5 x 7 as .npy"""
    dirs = {}
    for k, (sub, h, w, count) in enumerate((('HR', 40, 56, n), ('fake_LR', 10, 14, n), ('real_LR', 10, 14, 4))):
        d = tmp_path / sub
        d.mkdir()
        for i in range(count):
            _png(d / ('img_%02d.png' % i), h, w, 100 * k + i)
        dirs[sub] = str(d)
    d = tmp_path / 'ddm'
    d.mkdir()
    for i in range(n):
        np.save(str(d / ('img_%02d.npy' % i)), np.random.RandomState(900 + i).rand(1, 5, 7).astype(np.float32))
    dirs['ddm'] = str(d)
    return dirs


def _batches(ds, seed, count=3):
    _seed(seed)
    out = []
    for b in ds:
        out.append({k: v.cpu() for k, v in b.items() if k != '_keep'})
        if len(out) == count:
            break
    return out


BASE = {'batch_size': 2, 'HR_size': 32, 'use_flip': True, 'use_rot': True, 'use_shuffle': True, 'n_workers': 3, 'name': 'tiny', 'phase': 'train'}


def test_unpaired_dataset_gives_the_batches_of_the_fp32_store(tmp_path):
    dev = _gpu()
    from dasr_amd.data import DeviceUnpairedDataset
    dirs = _folders(tmp_path)
    opt = dict(BASE, mode='LRHR_wavelet_unpair_fake_weights_EQ', dataroot_fake_LR=dirs['fake_LR'], dataroot_real_LR=dirs['real_LR'], dataroot_HR=dirs['HR'],
               dataroot_fake_weights=dirs['ddm'])
    ref = _batches(DeviceUnpairedDataset(dict(opt), 4), 13)
    ds = DeviceUnpairedDataset(dict(opt, resident_u8=True), 4)
    assert all(t.dtype == torch.uint8 and t.device == dev and t.dim() == 3 and t.shape[2] == 3 for k in ('fake_LR', 'real_LR', 'HR') for t in ds.img[k])
    assert all(t.dtype == torch.float32 for t in ds.img['fake_w'])
    assert ds.resident_bytes == 3 * (6 * 40 * 56 + 6 * 10 * 14 + 4 * 10 * 14)
    got = _batches(ds, 13)
    assert len(got) == len(ref) == 3
    for g, r in zip(got, ref):
        assert set(g) == set(r) == {'LR_fake', 'LR_real', 'HR', 'HR_unpair', 'fake_w'}
        for k in r:
            assert g[k].shape == r[k].shape and torch.equal(g[k], r[k]), k


def test_paired_dataset_gives_the_batches_of_the_fp32_store_with_and_without_lr_files(tmp_path, margins):
    dev = _gpu()
    from dasr_amd.data import DevicePairedDataset
    dirs = _folders(tmp_path)
    opt = dict(BASE, mode='LRHR', dataroot_HR=dirs['HR'], dataroot_LR=dirs['fake_LR'])
    ref = _batches(DevicePairedDataset(dict(opt), 4), 17)
    ds = DevicePairedDataset(dict(opt, resident_u8=True), 4)
    assert all(t.dtype == torch.uint8 and t.device == dev for k in ('LR', 'HR') for t in ds.img[k])
    got = _batches(ds, 17)
    assert len(got) == len(ref) == 3
    for g, r in zip(got, ref):
        assert torch.equal(g['LR'], r['LR']) and torch.equal(g['HR'], r['HR']) and tuple(g['LR'].shape) == (2, 3, 8, 8)
    # no LR folder: the fp32 store makes the LR images on the host at construction (imresize_matlab), the byte store per batch on the device
    opt = dict(BASE, mode='LRHR', dataroot_HR=dirs['HR'], dataroot_LR=None)
    ref = _batches(DevicePairedDataset(dict(opt), 4), 19)
    ds = DevicePairedDataset(dict(opt, resident_u8=True), 4)
    assert ds.img['LR'] is None and all(t.dtype == torch.uint8 for t in ds.img['HR'])
    got = _batches(ds, 19)
    assert len(got) == len(ref) == 3
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g['HR'], r['HR']) and g['LR'].shape == r['LR'].shape
        err = float((g['LR'].double() - r['LR'].double()).abs().max())
        margins('paired resident_u8 without LR files, batch %d: LR vs the fp32 store (host imresize_matlab) max abs %.3e (bound 2^-23 = %.3e)' % (i, err, ULP))
        assert err <= ULP


@pytest.mark.parametrize('resident', [False, True])
def test_subset_file_selects_the_listed_files(tmp_path, resident):
    _gpu()
    from dasr_amd import train
    from dasr_amd.data import DevicePairedDataset, load_image
    dirs = _folders(tmp_path)
    listed = ['img_04.png', 'img_01.png']
    sub = tmp_path / 'subset.txt'
    sub.write_text('\n'.join(listed) + '\n')
    opt = dict(BASE, mode='LRHR', dataroot_HR=dirs['HR'], dataroot_LR=None, subset_file=str(sub), use_shuffle=False, resident_u8=resident)
    ds = train.create_dataset(dict(opt), {'scale': 4, 'model': 'sr'})
    assert isinstance(ds, DevicePairedDataset) and len(ds.img['HR']) == 2 and len(ds) == 1
    for t, name in zip(ds.img['HR'], sorted(listed)):
        want = load_image(os.path.join(dirs['HR'], name))
        stored = t.cpu().permute(2, 0, 1).float().div(255.0) if resident else t.cpu()
        assert torch.equal(stored, want), name
    b = _batches(ds, 3, 1)[0]
    assert tuple(b['HR'].shape) == (2, 3, 32, 32) and tuple(b['LR'].shape) == (2, 3, 8, 8)
    with pytest.raises(NotImplementedError, match='subset only supports generating LR on-the-fly'):
        train.create_dataset(dict(opt, dataroot_LR=dirs['fake_LR']), {'scale': 4, 'model': 'sr'})


def test_training_driver_logs_the_same_losses_with_and_without_resident_u8(tmp_path):
    """`python -m dasr_amd.train`, model sr, RRDB_net nf 32 nb 1, paired with LR files, three iterations from equal seeds: the batches are bit-equal, so are the losses.
    (nf 32 is the narrowest generator there is: RRDBNetHIP and SRResNetHIP take multiples of 32 only, an option file with nf 16 stops in the constructor.)"""
    _gpu()
    dirs = _folders(tmp_path)
    logs = []
    for name, extra in (('fp32_store', {}), ('byte_store', {'resident_u8': True})):
        ds = dict({k: v for k, v in BASE.items() if k != 'phase'}, mode='LRHR', dataroot_HR=dirs['HR'], dataroot_LR=dirs['fake_LR'], **extra)
        opt = {'name': name, 'use_tb_logger': False, 'model': 'sr', 'scale': 4, 'gpu_ids': [0], 'datasets': {'train': ds}, 'path': {'root': str(tmp_path)},
               'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 32, 'nb': 1, 'in_nc': 3, 'out_nc': 3, 'gc': 32},
               'train': {'lr_G': 2e-4, 'weight_decay_G': 0, 'beta1_G': 0.9, 'lr_scheme': 'MultiStepLR', 'lr_steps': [100], 'lr_gamma': 0.5, 'pixel_criterion': 'l1',
                         'pixel_weight': 1.0, 'manual_seed': 7, 'niter': 3},
               'logger': {'print_freq': 1, 'save_checkpoint_freq': 100}}
        path = tmp_path / (name + '.json')
        path.write_text(json.dumps(opt))
        p = subprocess.run([sys.executable, '-c', 'import sys\nsys.path.insert(0, %r)\nfrom dasr_amd import train\ntrain.main([\'-opt\', %r])\n' % (ROOT, str(path))],
                           cwd=ROOT, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        text = p.stdout.decode()
        assert p.returncode == 0, text[-4000:]
        assert ('resident_u8 [tiny]: 12 files' in text) == bool(extra)
        logs.append([l.split('> ', 1)[1].strip() for l in text.splitlines() if '<epoch:' in l and 'iter:' in l])
    assert len(logs[0]) == 3 and 'l_pix' in logs[0][0], logs[0]
    assert logs[0] == logs[1]


def test_fp32_store_batches_do_not_depend_on_when_the_host_waits():
    """the fp32 store's descriptors cross in one asynchronous copy from a pinned staging block (imgio.upload): eight batches enqueued back to back, nothing kept but
    the batch dicts and one synchronisation at the end, against the same eight with a synchronisation after each.  A staging block handed out again before its copy
    has run would show as a mismatch (not as a fault: every kernel clamps its source coordinates).  Every descriptor kind: 3-channel crops, the HR window at 4 x the
    LR origin, the domain-distance maps through the bilinear virtual resize (5 x 6 seen as 7 x 9), all flags."""
    dev = _gpu()
    from dasr_amd.data import DeviceUnpairedDataset
    g = torch.Generator().manual_seed(41)
    images = {'fake_LR': [torch.rand(3, 7, 9, generator=g) for _ in range(4)], 'real_LR': [torch.rand(3, 6, 8, generator=g) for _ in range(3)],
              'HR': [torch.rand(3, 28, 36, generator=g) for _ in range(4)], 'fake_w': [torch.rand(1, 5, 6, generator=g) for _ in range(4)]}
    ds = DeviceUnpairedDataset({'batch_size': 2, 'HR_size': 16, 'use_flip': True, 'use_rot': True, 'use_shuffle': True}, 4, images=images, device=dev)
    keys = ('LR_fake', 'LR_real', 'HR', 'HR_unpair', 'fake_w')

    def eight(wait):
        _seed(23)
        out = []
        for _ in range(4):
            for b in ds:
                out.append(b)
                if wait:
                    torch.cuda.synchronize()
        torch.cuda.synchronize()
        return out
    free, waited = eight(False), eight(True)
    assert len(free) == len(waited) == 8 and len({int(b['_keep'][0].data_ptr()) for b in free}) == 8
    assert [tuple(free[0][k].shape) for k in keys] == [(2, 3, 4, 4), (2, 3, 4, 4), (2, 3, 16, 16), (2, 3, 16, 16), (2, 1, 4, 4)]
    for i, (a, b) in enumerate(zip(free, waited)):
        for k in keys:
            assert torch.equal(a[k], b[k]), (i, k)
    assert not all(torch.equal(free[0][k], free[1][k]) for k in keys)           # (the batches differ from each other: a stale block would be seen)
