"""GPU: iterative back-projection (`"back_projection": true | N`, `python -m dasr_amd.back_projection`; reference: codes/SRN/scripts/back_projection/backprojection.m,
main_bp.m).  The residual kernel bit for bit against dasr_imresize_down and a torch subtraction, the update kernel and twenty iterations against the fp64 restatement
on the host (backproject.back_project_fp64), the option key through the evaluation driver and one validation pass, and the folder CLI."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -22
EPS = 2.0 ** -24


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tiles():
    from dasr_amd import backproject
    return backproject.RES_TILE, backproject.UPD_TILE


def _residual_cases():
    """(s, (h, w) of the LR image, C): the issue's list; the two tile shapes follow the kernel's LR tile (backproject.RES_TILE)"""
    (rt, ct), _ = _tiles()
    cases = [(4, hw, c) for hw in ((1, 1), (2, 3), (5, 7), (17, 33), (rt + 1, ct + 1), (rt - 1, ct - 1)) for c in (1, 3)]
    return cases + [(2, (6, 9), 1), (2, (6, 9), 3), (3, (4, 5), 1), (3, (4, 5), 3)]


def _update_cases():
    """the residual list, plus HR sizes that straddle the update tile (backproject.UPD_TILE) by one LR sample at s = 4 and by the smallest step the scale allows:
    one HR sample short at s = 3 (15 x 63 for a 16 x 64 tile), two beyond at s = 2 (18 x 66)"""
    _, (uy, ux) = _tiles()
    extra = [(4, (uy // 4 + 1, ux // 4 + 1), 3), (4, (uy // 4 - 1, ux // 4 - 1), 3), (3, ((uy - 1) // 3, (ux - 1) // 3), 3), (3, (uy // 3 + 1, ux // 3 + 1), 1),
             (2, (uy // 2 + 1, ux // 2 + 1), 3), (2, (uy // 2 - 1, ux // 2 - 1), 1)]
    return _residual_cases() + extra


def _case_id(c):
    return 'x%d_%dx%d_c%d' % (c[0], c[1][0], c[1][1], c[2])


def _rand(shape, seed):
    """fp32 values outside [0, 1]: standard normal times 1.5"""
    return 1.5 * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _down_device(sr, s):
    """dasr_imresize_down of a [1, C, H, W] device tensor: [1, C, H / s, W / s]"""
    from dasr_amd import _lib
    from dasr_amd.imgio import tap_table
    _, c, H, W = sr.shape
    (jh, wh), (jw, ww) = tap_table(H, s, sr.device), tap_table(W, s, sr.device)
    tmp = torch.empty((c, H // s, W), dtype=torch.float64, device=sr.device)
    out = torch.full((1, c, H // s, W // s), float('nan'), device=sr.device)
    assert _lib.lib().dasr_imresize_down(sr.data_ptr(), c, H, W, s, jh.data_ptr(), wh.data_ptr(), jw.data_ptr(), ww.data_ptr(), tmp.data_ptr(), out.data_ptr(), _stream()) == 0
    return out


# ---- 1. residual kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', _residual_cases(), ids=_case_id)
def test_residual_is_bit_equal_to_imresize_down_and_subtraction(case):
    dev = _gpu()
    from dasr_amd import backproject
    s, (h, w), c = case
    sr, lr = _rand((1, c, s * h, s * w), 7 * h + w + s), _rand((1, c, h, w), 11 * h + w + s)
    assert sr.numel() < 64 or (float(sr.min()) < 0 and float(sr.max()) > 1)
    srd, lrd = sr.to(dev), lr.to(dev)
    got = backproject.residual(srd, lrd)
    want = lrd - _down_device(srd, s)   # the subtraction in fp32, by torch, on the device
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, c, h, w)
    assert torch.equal(got.cpu(), want.cpu())
    assert torch.equal(srd.cpu(), sr) and torch.equal(lrd.cpu(), lr)   # the inputs are left alone


# ---- 2. update kernel ---------------------------------------------------------------------------------------------------------------------
def _check_update(sr, d, s, what):
    """one dasr_bp_update against sr + conv(up(d)) in fp64; elementwise bound 2^-24 max(1, |ref|) + 1e-12 (fp64 arithmetic, one rounding to fp32)"""
    from dasr_amd import backproject
    dev = torch.device('cuda')
    srd, dd = sr.to(dev), d.to(dev)
    out = backproject.update_(srd, dd)
    torch.cuda.synchronize()
    assert out is srd and torch.equal(dd.cpu(), d)
    ref = sr[0].double() + backproject.upsample_conv_fp64(d[0], s)
    err = (srd.cpu()[0].double() - ref).abs()
    bound = EPS * ref.abs().clamp(min=1.0) + 1e-12
    print('bp_update %s: worst error / bound %.3f' % (what, float((err / bound).max())))
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, (what, bad[:8].tolist(), float(err.max()))
    return srd.cpu()


@pytest.mark.parametrize('case', _update_cases(), ids=_case_id)
def test_update_matches_fp64(case):
    _gpu()
    s, (h, w), c = case
    sr, d = _rand((1, c, s * h, s * w), 13 * h + w + s), _rand((1, c, h, w), 17 * h + w + s)
    _check_update(sr, d, s, _case_id(case))


@pytest.mark.parametrize('s', [2, 3, 4])
def test_update_of_single_impulses(s):
    """d = one impulse at each corner, mid-edge and the centre of LR 5 x 7: the up-sampling mirrors at the image border, the 5 x 5 pass sees zeros beyond it and real
    neighbours beyond a tile border (HR 20 x 28 at s = 4 is two tiles high) -- an impulse at a border separates the three"""
    _gpu()
    h, w = 5, 7
    sr = _rand((1, 1, s * h, s * w), 5 + s)
    outs = []
    for y in (0, h // 2, h - 1):
        for x in (0, w // 2, w - 1):
            d = torch.zeros(1, 1, h, w)
            d[0, 0, y, x] = 1.0
            outs.append(_check_update(sr, d, s, 'x%d impulse (%d, %d)' % (s, y, x)))
    assert all(not torch.equal(outs[0], o) for o in outs[1:])


def test_entry_points_return_einval():
    dev = _gpu()
    from dasr_amd import _lib, backproject
    from dasr_amd.imgio import tap_table, up_tap_table
    import ctypes as C
    L, st = _lib.lib(), _stream()
    s, h, w = 4, 5, 7
    sr, lr = torch.zeros(1, 3, s * h, s * w, device=dev), torch.ones(1, 3, h, w, device=dev)
    d = torch.zeros(1, 3, h, w, device=dev)
    dn = [t.data_ptr() for t in tap_table(s * h, s, dev) + tap_table(s * w, s, dev)]
    up = [t.data_ptr() for t in up_tap_table(h, s, dev) + up_tap_table(w, s, dev)]
    u5 = C.cast((C.c_double * 5)(*backproject.gaussian_u5()), C.c_void_p)
    assert L.dasr_bp_residual(None, lr.data_ptr(), 3, s * h, s * w, s, *dn, d.data_ptr(), st) == EINVAL
    assert L.dasr_bp_residual(sr.data_ptr(), lr.data_ptr(), 3, s * h, s * w, s, *dn, None, st) == EINVAL
    assert L.dasr_bp_residual(sr.data_ptr(), lr.data_ptr(), 3, s * h, s * w, 5, *dn, d.data_ptr(), st) == EINVAL
    assert L.dasr_bp_residual(sr.data_ptr(), lr.data_ptr(), 3, s * h + 1, s * w, s, *dn, d.data_ptr(), st) == EINVAL   # H != s h
    assert L.dasr_bp_residual(sr.data_ptr(), lr.data_ptr(), 65536, s * h, s * w, s, *dn, d.data_ptr(), st) == EINVAL
    assert L.dasr_bp_residual(sr.data_ptr(), lr.data_ptr(), 3, 65536, s * w, s, *dn, d.data_ptr(), st) == EINVAL
    assert L.dasr_bp_update(None, lr.data_ptr(), 3, h, w, s, *up, u5, st) == EINVAL
    assert L.dasr_bp_update(sr.data_ptr(), lr.data_ptr(), 3, h, w, s, *up, None, st) == EINVAL
    assert L.dasr_bp_update(sr.data_ptr(), lr.data_ptr(), 3, h, w, 1, *up, u5, st) == EINVAL
    assert L.dasr_bp_update(sr.data_ptr(), lr.data_ptr(), 3, 16384, w, s, *up, u5, st) == EINVAL   # s h over 65535
    assert L.dasr_bp_update(sr.data_ptr(), lr.data_ptr(), 0, h, w, s, *up, u5, st) == EINVAL
    torch.cuda.synchronize()
    assert float(sr.abs().sum()) == 0 and float(d.abs().sum()) == 0   # nothing was launched


# ---- 3. twenty iterations -----------------------------------------------------------------------------------------------------------------
def _sr_lr(s, h, w, seed):
    """an LR image, and an SR image that is not consistent with it: the HR image it came from plus noise"""
    from dasr_amd.data import imresize_matlab
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(3, s * h, s * w, generator=g)
    lr = imresize_matlab(hr, 1.0 / s)
    return (hr + 0.05 * torch.randn(hr.shape, generator=g))[None].contiguous(), lr[None].contiguous()


@pytest.mark.parametrize('s,hw', [(4, (12, 16)), (4, (17, 33)), (2, (6, 9))], ids=['x4_12x16', 'x4_17x33', 'x2_6x9'])
def test_twenty_iterations_match_fp64(s, hw):
    """bound: iters * 3 * 2^-24 * max(1, max|ref|) -- per iteration sr rounds once (2^-24 below 2), the down image and d once each (2^-25), and the latter pass through
    an up-sampling whose absolute weights sum to about 1.57; it assumes that the iteration does not amplify earlier errors"""
    dev = _gpu()
    from dasr_amd import backproject
    sr, lr = _sr_lr(s, hw[0], hw[1], 31 * hw[0] + s)
    srd, lrd = sr.to(dev), lr.to(dev)
    out = backproject.back_project(srd, lrd, 20)
    again = backproject.back_project(srd, lrd, 20)
    zero = backproject.back_project(srd, lrd, 0)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == srd.shape and out.is_cuda and out.data_ptr() != srd.data_ptr()
    assert torch.equal(srd.cpu(), sr) and torch.equal(lrd.cpu(), lr)              # the inputs are unmodified
    assert torch.equal(out.cpu(), again.cpu())                                    # same inputs, same bits
    assert torch.equal(zero.cpu(), sr) and zero.data_ptr() != srd.data_ptr()      # iters = 0: a bit-equal copy
    ref = backproject.back_project_fp64(sr, lr, 20)
    err = float((out.cpu().double() - ref).abs().max())
    bound = 20 * 3 * EPS * max(1.0, float(ref.abs().max()))
    print('back_project x%d %dx%d: max error %.3e = %.2f x 2^-24, bound %.3e' % (s, hw[0], hw[1], err, err / EPS, bound))
    assert err <= bound, (err, bound)
    res = lambda t: float((lrd - _down_device(t, s)).abs().max())
    r0, r20 = res(srd), res(out)
    print('  max|lr - down(sr)|: %.3e -> %.3e' % (r0, r20))
    assert r20 < r0


def test_back_project_refuses_what_it_cannot_pair():
    dev = _gpu()
    from dasr_amd import backproject
    z = lambda *shape: torch.zeros(shape, device=dev)
    for sr, lr in ((z(2, 3, 8, 8), z(2, 3, 2, 2)), (z(1, 3, 8, 8), z(1, 1, 2, 2)), (z(1, 3, 8, 12), z(1, 3, 2, 4)), (z(1, 3, 10, 10), z(1, 3, 2, 2)), (z(1, 3, 2, 2), z(1, 3, 2, 2))):
        with pytest.raises(ValueError) as e:
            backproject.back_project(sr, lr, 2)
        assert str(tuple(sr.shape)) in str(e.value) and str(tuple(lr.shape)) in str(e.value)
    with pytest.raises(ValueError):
        backproject.back_project(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 2, 2), 2)   # host tensors: there is no fallback


# ---- 4. pipeline --------------------------------------------------------------------------------------------------------------------------
def _json_opt(tmp_path, name, extra=None):
    opt = {
        'name': name, 'use_tb_logger': False, 'model': 'sr', 'scale': 4, 'gpu_ids': [0], 'chop': False, 'val_lpips': False,
        'datasets': {'test_1': {'name': 'synset', 'mode': 'synthetic', 'n_images': 2, 'LR_size': 24}},
        'path': {'root': str(tmp_path), 'pretrain_model_G': None},
        'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 32, 'nb': 1, 'in_nc': 3, 'out_nc': 3, 'gc': 32},
    }
    opt.update(extra or {})
    p = tmp_path / (name + '.json')
    p.write_text(json.dumps(opt))
    return str(p)


def _log_text(root):
    return ''.join(open(os.path.join(root, f)).read() for f in sorted(os.listdir(root)) if f.endswith('.log'))


def test_evaluation_cli_with_back_projection(tmp_path):
    _gpu()
    from PIL import Image
    from dasr_amd import options, test as dtest, util
    from dasr_amd.backproject import back_project
    from dasr_amd.lpips import lpips_metric
    from dasr_amd.models import create_model
    from dasr_amd.train import create_dataset
    from oracle import fixtures, nets
    g_path = tmp_path / 'G.pth'   # weights of O(1) gain: the SR images are far from black and far from consistent with the LR images
    torch.save(fixtures.seeded_state_dict(nets.RRDBNet(3, 3, 32, 1, 4).state_dict(), 8, 1.0), str(g_path))
    path = {'root': str(tmp_path), 'pretrain_model_G': str(g_path)}
    full = {'back_projection': 3, 'self_ensemble': True, 'device_metrics': True, 'val_lpips': True, 'allow_random_perceptual': True}
    runs = {}
    for name, extra in (('bp_off', {}), ('bp_on', {'back_projection': 3}), ('bp_on_dev', {'back_projection': 3, 'device_metrics': True}), ('bp_full', full)):
        p = _json_opt(tmp_path, name, dict(extra, path=dict(path)))
        opt = options.dict_to_nonedict(options.parse(p, is_train=False))
        loaders = [('synset', list(create_dataset(dict(opt['datasets']['test_1'], phase='test'), opt)))]
        s = dtest.main(['-opt', p], loaders)['synset']
        root = tmp_path / 'results' / name
        runs[name] = (s, sorted((root / 'synset' / 'imgs').glob('*.png')), _log_text(str(root)))
        assert len(runs[name][1]) == 2
    note = 'back_projection: every SR image is back-projected onto its LR image, 3 iterations'
    assert 'back_projection:' not in runs['bp_off'][2]   # the key absent: neither the option dump nor a note mentions it
    assert all(runs[k][2].count(note) == 1 for k in ('bp_on', 'bp_on_dev', 'bp_full'))
    px = lambda p: np.array(Image.open(str(p)))[:, :, ::-1]
    # the expected images from a model WITHOUT the key: test() / test_x8(), then back_project by hand
    opt = options.dict_to_nonedict(options.parse(_json_opt(tmp_path, 'bp_direct', {'val_lpips': True, 'allow_random_perceptual': True, 'path': dict(path)}), is_train=False))
    m = create_model(opt)
    lpips = []
    for i, data in enumerate(create_dataset(dict(opt['datasets']['test_1'], phase='test'), opt)):
        m.feed_data(data, False)
        m.test()
        plain = m.fake_H.detach().clone()
        want = util.tensor2img(back_project(plain, m.var_L, 3)[0].cpu())
        assert np.array_equal(px(runs['bp_off'][1][i]), util.tensor2img(plain[0].cpu()))
        assert not np.array_equal(px(runs['bp_off'][1][i]), want)                  # the key has an effect
        assert np.array_equal(px(runs['bp_on'][1][i]), want)
        assert np.array_equal(px(runs['bp_on_dev'][1][i]), want)                   # the same bytes with device_metrics
        m.test_x8()
        bp_x8 = back_project(m.fake_H.detach().clone(), m.var_L, 3)
        assert np.array_equal(px(runs['bp_full'][1][i]), util.tensor2img(bp_x8[0].cpu()))   # with self_ensemble the input is the test_x8 image
        lpips.append((float(lpips_metric(m.cri_fea_lpips, bp_x8, m.real_H)), float(m.LPIPS)))
    assert abs(runs['bp_on'][0]['psnr'] - runs['bp_on_dev'][0]['psnr']) < 1e-3
    # under val_lpips the logged LPIPS is that of the back-projected image, not of the generator's
    got = runs['bp_full'][0]['lpips']
    assert abs(got - sum(a for a, _ in lpips) / 2) < 1e-6, (got, lpips)
    assert all(abs(a - b) > 1e-4 for a, b in lpips), lpips   # (the two images are told apart by the metric)
    assert m.lpips_label + ': ' in runs['bp_full'][2]


def test_models_apply_the_key_and_validate_uses_it(tmp_path):
    _gpu()
    import logging
    from PIL import Image
    from dasr_amd import options, train, util
    from dasr_amd.backproject import back_project
    from dasr_amd.models import create_model
    from oracle import fixtures
    # SRModel through one validation pass
    opt = options.dict_to_nonedict(options.parse(_json_opt(tmp_path, 'bp_val', {'back_projection': True}), is_train=False))
    opt['path']['val_images'] = str(tmp_path / 'val_images')
    m = create_model(opt)
    val_set = list(train.create_dataset(dict(opt['datasets']['test_1'], phase='val'), opt))
    train.validate(m, val_set, opt, 5, logging.getLogger('bp_val_test'))
    pngs = sorted((tmp_path / 'val_images').rglob('*_5.png'))
    assert len(pngs) == 2
    opt_off = options.dict_to_nonedict(dict(opt, back_projection=None))
    m_off = create_model(opt_off)
    m_off.netG.load_state_dict(m.netG.state_dict())
    for data, png in zip(val_set, pngs):
        m_off.feed_data(data, False)
        m_off.test()
        want = back_project(m_off.fake_H, m_off.var_L, 20)
        assert np.array_equal(np.array(Image.open(str(png)))[:, :, ::-1], util.tensor2img(want[0].cpu()))
    # DASR_Model: test() applies the key, test(tsamples=True) (a batch of crops) does not
    dopt = fixtures.make_opt('dasr_wavelet_nf64_nb23_n1_32')
    dopt['network_G'].update(nb=1)
    dopt['train']['feature_weight'] = 0
    dopt.update(gpu_ids=[0], model='DASR', back_projection=2)
    dm = create_model(options.dict_to_nonedict(dopt))
    g = torch.Generator().manual_seed(12)
    dm.feed_data({'LR': torch.rand(1, 3, 20, 28, generator=g), 'HR': torch.rand(1, 3, 80, 112, generator=g)}, False)
    dm.test()
    got = dm.fake_H.clone()
    plain = dm._generate(dm.var_L)
    assert torch.equal(got, back_project(plain, dm.var_L, 2)) and not torch.equal(got, plain)
    dm.test_x8()
    assert tuple(dm.fake_H.shape) == (1, 3, 80, 112)
    dm.feed_data({'LR': torch.rand(2, 3, 16, 16, generator=g), 'HR': torch.rand(1, 3, 64, 64, generator=g)}, False)
    dm.test(tsamples=True)
    assert tuple(dm.fake_H.shape) == (2, 3, 64, 64)


# ---- 5. CLI -------------------------------------------------------------------------------------------------------------------------------
def test_folder_cli(tmp_path):
    """a written byte may differ from round(255 clip(back_project_fp64)) by 1, and only where the fp64 value x 255 lies within 255 x (the bound of twenty iterations) of a
    half-integer; every other byte is equal"""
    _gpu()
    from PIL import Image
    from dasr_amd import back_projection as cli
    from dasr_amd.backproject import back_project_fp64
    lr_dir, sr_dir, out_dir = tmp_path / 'LR', tmp_path / 'results', tmp_path / 'results_20bp'
    lr_dir.mkdir()
    sr_dir.mkdir()
    to_u8 = lambda t: (t.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0).numpy()
    names = ['a.png', 'b.png', 'c.png']
    for k, name in enumerate(names):
        sr, lr = _sr_lr(4, 12, 16, 50 + k)
        Image.fromarray(to_u8(sr[0])).save(str(sr_dir / name))
        Image.fromarray(to_u8(lr[0])).save(str(lr_dir / name))
    written = cli.main(['--lr_dir', str(lr_dir), '--sr_dir', str(sr_dir), '--out_dir', str(out_dir), '--num_workers', '2'])
    assert written == [str(out_dir / n) for n in names] and all(os.path.isfile(p) for p in written)
    load = lambda p: torch.from_numpy(np.array(Image.open(str(p)))).permute(2, 0, 1).double() / 255.0   # (im2double)
    for name in names:
        ref = back_project_fp64(load(sr_dir / name), load(lr_dir / name), 20)
        got = np.array(Image.open(str(out_dir / name))).astype(np.int64)
        assert got.shape == (48, 64, 3)
        v = (ref.clamp(0, 1) * 255.0).permute(1, 2, 0).numpy()
        want = np.round(v).astype(np.int64)
        tol = 255.0 * 20 * 3 * EPS * max(1.0, float(ref.abs().max()))
        near_half = np.abs(v - np.floor(v) - 0.5) <= tol
        diff = np.abs(got - want)
        print('%s: %d of %d bytes differ, %d samples within %.1e of a half-integer' % (name, int((diff != 0).sum()), diff.size, int(near_half.sum()), tol))
        assert int(diff.max()) <= 1 and not bool((diff != 0)[~near_half].any())
        assert not np.array_equal(got, np.array(Image.open(str(sr_dir / name))).astype(np.int64))   # the images were moved
