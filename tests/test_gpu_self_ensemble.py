"""GPU: the x8 self-ensemble (`"self_ensemble": true`; reference: codes/SRN/models/SR_model.py:102-140 test_x8): the two geometry kernels of csrc/imgio.hip bit for bit
against torch on the CPU, BaseModel.test_x8 against the oracle net run on the eight torch-transformed inputs, and the two drivers with the option key."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -22
# the issue's shapes: one element, widths / heights that are no multiple of 4, an exact tile, partial tiles on both axes, more than one tile on each axis;
# (7, 4) and (132, 68): the 16-byte paths with a partial tile (one axis / both axes vectorised)
KSHAPES = [(1, 1), (5, 3), (64, 64), (65, 130), (96, 33), (7, 4), (132, 68)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', KSHAPES, ids=lambda s: '%dx%d' % s)
def test_dihedral8_is_an_exact_copy_of_flip_and_transpose(hw):
    dev = _gpu()
    from dasr_amd import _lib
    H, W = hw
    x = torch.randn(3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    xd = x.to(dev)
    a = torch.full((4, 3, H, W), float('nan'), device=dev)
    b = torch.full((4, 3, W, H), float('nan'), device=dev)
    assert _lib.lib().dasr_dihedral8(xd.data_ptr(), 3, H, W, a.data_ptr(), b.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    a, b = a.cpu(), b.cpu()
    for i in range(8):
        want = x
        if i & 1:
            want = want.flip(-1)
        if (i >> 1) & 1:
            want = want.flip(-2)
        if i >> 2:
            want = want.transpose(-1, -2)
        got = a[i] if i < 4 else b[i - 4]
        assert torch.equal(got, want.contiguous()), i
    assert torch.equal(xd.cpu(), x)   # the source is left alone


def _seeded_sr(shape, seed):
    """negative and positive values, magnitudes from 1e-3 to 1e2"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(shape, generator=g) * 5.0 - 3.0)
    return (mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)).float()


@pytest.mark.parametrize('hw', KSHAPES, ids=lambda s: '%dx%d' % s)
def test_dihedral8_mean_is_the_sequential_fp32_sum(hw):
    dev = _gpu()
    from dasr_amd import _lib
    H, W = hw
    sr_a, sr_b = _seeded_sr((4, 3, H, W), 11 * H + W), _seeded_sr((4, 3, W, H), 13 * H + W)
    assert float(sr_a.min()) < 0 < float(sr_a.max()) and 0.999e-3 <= float(sr_a.abs().min()) and float(sr_a.abs().max()) <= 1e2
    ad, bd = sr_a.to(dev), sr_b.to(dev)
    out = torch.full((3, H, W), float('nan'), device=dev)
    assert _lib.lib().dasr_dihedral8_mean(ad.data_ptr(), bd.data_ptr(), 3, H, W, out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    # s_i on the CPU with torch: member i's transform undone
    s = []
    for i in range(8):
        y = sr_a[i] if i < 4 else sr_b[i - 4].transpose(-1, -2)
        if (i >> 1) & 1:
            y = y.flip(-2)
        if i & 1:
            y = y.flip(-1)
        s.append(y.contiguous())
    want = 0.125 * (((((((s[0] + s[1]) + s[2]) + s[3]) + s[4]) + s[5]) + s[6]) + s[7])
    assert want.dtype == torch.float32 and torch.equal(got, want)
    # first-order bound of a sequential sum of 8 terms (7 adds, each within 2^-24 relative of its partial sum; the scaling by a power of two is exact)
    s64 = torch.stack(s).double()
    err, bound = (got.double() - s64.mean(0)).abs(), 7 * 2.0 ** -24 * s64.abs().mean(0)
    print('dihedral8_mean %dx%d: worst error / bound %.3f' % (H, W, float((err / bound).max())))
    assert bool((err <= bound).all())


def test_entry_points_return_einval():
    dev = _gpu()
    from dasr_amd import _lib
    L = _lib.lib()
    H, W = 5, 3
    x = torch.zeros(3, H, W, device=dev)
    a, b, o = torch.zeros(4, 3, H, W, device=dev), torch.zeros(4, 3, W, H, device=dev), torch.zeros(3, H, W, device=dev)
    st = _stream()
    assert L.dasr_dihedral8(None, 3, H, W, a.data_ptr(), b.data_ptr(), st) == EINVAL
    assert L.dasr_dihedral8(x.data_ptr(), 3, 0, W, a.data_ptr(), b.data_ptr(), st) == EINVAL
    assert L.dasr_dihedral8(x.data_ptr(), 3, H, W, x.data_ptr(), b.data_ptr(), st) == EINVAL
    assert L.dasr_dihedral8_mean(None, b.data_ptr(), 3, H, W, o.data_ptr(), st) == EINVAL
    assert L.dasr_dihedral8_mean(a.data_ptr(), b.data_ptr(), 3, 0, W, o.data_ptr(), st) == EINVAL
    assert L.dasr_dihedral8_mean(a.data_ptr(), b.data_ptr(), 3, H, W, a.data_ptr(), st) == EINVAL
    torch.cuda.synchronize()
    assert float(a.abs().sum()) == 0 and float(o.abs().sum()) == 0   # nothing was launched


# ---- model --------------------------------------------------------------------------------------------------------------------------------
def _oracle_x8(net_fn, x):
    """the generator on the eight torch-transformed inputs, every transform undone, the mean in fp64"""
    outs = []
    for i in range(8):
        y = x
        if i & 1:
            y = y.flip(-1)
        if (i >> 1) & 1:
            y = y.flip(-2)
        if i >> 2:
            y = y.transpose(-1, -2)
        with torch.no_grad():
            y = net_fn(y.contiguous()).double()
        if i >> 2:
            y = y.transpose(-1, -2)
        if (i >> 1) & 1:
            y = y.flip(-2)
        if i & 1:
            y = y.flip(-1)
        outs.append(y)
    return torch.stack(outs).mean(0)


def _sr_model(chop, sd_seed=3, **extra):
    from oracle import fixtures, nets
    from dasr_amd import options
    from dasr_amd.models import create_model
    opt = fixtures.make_opt('sr_nf64_nb1_b1_24x40')
    opt['gpu_ids'] = [0]
    opt['chop'] = chop
    opt.update(extra)
    m = create_model(options.dict_to_nonedict(opt))
    net = nets.RRDBNet(3, 3, 64, 1, 4)
    sd = fixtures.seeded_state_dict(net.state_dict(), sd_seed, 0.1)
    net.load_state_dict(sd)
    m.netG.load_state_dict(sd)
    return m, net


@pytest.mark.parametrize('hw', [(52, 44), (53, 47), (48, 48)], ids=['52x44', '53x47_odd', '48x48_square'])
@pytest.mark.parametrize('chop', [False, True])
def test_test_x8_matches_oracle(chop, hw):
    """(48 x 48: both batches of 4 run on the same plan -- the first result must survive the second forward)"""
    _gpu()
    from oracle import util_ref
    m, net = _sr_model(chop)
    H, W = hw
    g = torch.Generator().manual_seed(8)
    x = torch.rand(1, 3, H, W, generator=g)
    m.feed_data({'LR': x, 'HR': torch.rand(1, 3, 4 * H, 4 * W, generator=g)}, False)
    built = []
    make = m.netG._make_plan
    m.netG._make_plan = lambda *a, **k: (built.append(a), make(*a, **k))[1]
    m.test_x8()
    got = m.fake_H.cpu()
    fn = (lambda t: util_ref.forward_chop(t, 4, net, shave=20, min_size=320000)) if chop else net
    want = _oracle_x8(fn, x)
    assert tuple(got.shape) == (1, 3, 4 * H, 4 * W) and got.dtype == torch.float32 and m.fake_H.is_cuda
    r = rel(got, want)
    print('test_x8 %dx%d chop %s: rel %.2e' % (H, W, chop, r))
    assert r < 1e-3, r
    # a second image of the same size: the (4, h, w) and (4, w, h) plans are both still cached (RRDBNetHIP.INFER_CACHE = 2), nothing is rebuilt
    n_first = len(built)
    assert n_first == (1 if H == W else 2), built
    m.test_x8()
    assert len(built) == n_first, built
    assert torch.equal(m.fake_H.cpu(), got)   # same inputs, same bits
    # the ensemble of a network that is not equivariant is not the network
    m.test()
    plain = m.fake_H.cpu()
    assert rel(got, plain) > 1e-6
    vis = m.get_current_visuals()
    assert tuple(vis['SR'].shape) == (3, 4 * H, 4 * W)


def test_test_x8_with_sr_resnet_matches_eight_forwards():
    """the oracle has no SRResNet: against the eight-forward composition on the project's own generator (torch transforms on the device)"""
    _gpu()
    from oracle import fixtures
    from dasr_amd import options
    from dasr_amd.models import create_model
    opt = fixtures.make_opt('sr_nf64_nb1_b1_24x40')
    opt['gpu_ids'] = [0]
    opt['network_G'].update(which_model_G='sr_resnet', upsample_mode=None, nb=2)
    m = create_model(options.dict_to_nonedict(opt))
    m.netG.load_state_dict(fixtures.seeded_state_dict(m.netG.state_dict(), 5, 0.1))
    x = torch.rand(1, 3, 40, 28, generator=torch.Generator().manual_seed(9))
    m.feed_data({'LR': x}, False)
    m.test_x8()
    got = m.fake_H.cpu()
    want = _oracle_x8(lambda t: m.netG.forward(t.cuda()).clone().cpu(), x)
    assert tuple(got.shape) == (1, 3, 160, 112)
    assert rel(got, want) < 1e-3, rel(got, want)
    m.test()
    assert rel(got, m.fake_H.cpu()) > 1e-6


def test_test_x8_of_the_dasr_trainer_sets_lpips():
    _gpu()
    from oracle import fixtures
    from dasr_amd import options
    from dasr_amd.models import create_model
    from dasr_amd.lpips import lpips_metric
    opt = fixtures.make_opt('dasr_wavelet_nf64_nb23_n1_32')
    opt['network_G'].update(nb=1)
    opt['train']['feature_weight'] = 0   # (no VGG19 for this test: only the generator and the validation metric are used)
    opt.update(gpu_ids=[0], val_lpips=True, allow_random_perceptual=True, model='DASR')
    m = create_model(options.dict_to_nonedict(opt))
    g = torch.Generator().manual_seed(10)
    x, hr = torch.rand(1, 3, 36, 28, generator=g), torch.rand(1, 3, 144, 112, generator=g)
    m.feed_data({'LR': x, 'HR': hr}, False)
    m.LPIPS = None
    m.test_x8()
    assert tuple(m.fake_H.shape) == (1, 3, 144, 112)
    got = float(m.LPIPS)
    assert np.isfinite(got)
    assert got == float(lpips_metric(m.cri_fea_lpips, m.fake_H, hr.cuda()))
    assert 'LPIPS' in m.get_current_visuals()
    # test(tsamples=True) is untouched: a batch of crops, no LPIPS
    m.feed_data({'LR': torch.rand(2, 3, 16, 16, generator=g), 'HR': torch.rand(1, 3, 64, 64, generator=g)}, False)
    m.test(tsamples=True)
    assert tuple(m.fake_H.shape) == (2, 3, 64, 64)


# ---- drivers ------------------------------------------------------------------------------------------------------------------------------
def _json_opt(tmp_path, name, is_train, extra=None):
    opt = {
        'name': name, 'use_tb_logger': False, 'model': 'sr', 'scale': 4, 'gpu_ids': [0], 'chop': False, 'val_lpips': False,
        'datasets': {},
        'path': {'root': str(tmp_path), 'pretrain_model_G': None},
        'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 32, 'nb': 1, 'in_nc': 3, 'out_nc': 3, 'gc': 32},
    }
    if is_train:
        opt['datasets'] = {'train': {'name': 'syn', 'mode': 'synthetic', 'batch_size': 4, 'HR_size': 64, 'n_batches': 8},
                           'val': {'name': 'synval', 'mode': 'synthetic', 'n_images': 2, 'LR_size': 24}}
        opt['train'] = {'lr_G': 2e-4, 'weight_decay_G': 0, 'beta1_G': 0.9, 'lr_scheme': 'MultiStepLR', 'lr_steps': [100], 'lr_gamma': 0.5,
                        'pixel_criterion': 'l1', 'pixel_weight': 1.0, 'manual_seed': 0, 'niter': 4, 'val_freq': 2}
        opt['logger'] = {'print_freq': 2, 'save_checkpoint_freq': 4}
    else:
        opt['datasets'] = {'test_1': {'name': 'synset', 'mode': 'synthetic', 'n_images': 2, 'LR_size': 24}}
    opt.update(extra or {})
    p = tmp_path / (name + '.json')
    p.write_text(json.dumps(opt))
    return str(p)


def _log_text(root):
    return ''.join(open(os.path.join(root, f)).read() for f in sorted(os.listdir(root)) if f.endswith('.log'))


def test_evaluation_cli_with_self_ensemble(tmp_path):
    _gpu()
    from PIL import Image
    from dasr_amd import options, test as dtest, util
    from dasr_amd.models import create_model
    from dasr_amd.train import create_dataset
    from oracle import fixtures, nets
    g_path = tmp_path / 'G.pth'   # weights of O(1) gain: the SR images are far from black, the ensemble moves whole grey levels
    torch.save(fixtures.seeded_state_dict(nets.RRDBNet(3, 3, 32, 1, 4).state_dict(), 8, 1.0), str(g_path))
    path = {'root': str(tmp_path), 'pretrain_model_G': str(g_path)}
    runs = {}
    for name, extra in (('se_off', {}), ('se_on', {'self_ensemble': True}), ('se_on_dev', {'self_ensemble': True, 'device_metrics': True})):
        s = dtest.main(['-opt', _json_opt(tmp_path, name, False, dict(extra, path=dict(path)))])['synset']
        assert all(np.isfinite(s[k]) for k in ('psnr', 'ssim', 'psnr_y', 'ssim_y')), (name, s)
        root = tmp_path / 'results' / name
        runs[name] = (s, sorted((root / 'synset' / 'imgs').glob('*.png')), _log_text(str(root)))
    assert len(runs['se_off'][1]) == len(runs['se_on'][1]) == len(runs['se_on_dev'][1]) == 2
    assert 'x8 self-ensemble inference is on' in runs['se_on'][2] and 'x8 self-ensemble inference is on' in runs['se_on_dev'][2]
    assert 'self-ensemble inference is on' not in runs['se_off'][2]
    # the key has an effect, and the device-metrics run saves the same bytes as the host run
    px = lambda p: np.array(Image.open(str(p)))
    assert any(not np.array_equal(px(a), px(b)) for a, b in zip(runs['se_off'][1], runs['se_on'][1]))
    assert all(np.array_equal(px(a), px(b)) for a, b in zip(runs['se_on'][1], runs['se_on_dev'][1]))
    assert abs(runs['se_on'][0]['psnr'] - runs['se_on_dev'][0]['psnr']) < 1e-3
    # the saved SR image of the ensemble run = tensor2img of test_x8()'s fake_H for the same image
    opt = options.dict_to_nonedict(options.parse(_json_opt(tmp_path, 'se_direct', False, {'self_ensemble': True, 'path': dict(path)}), is_train=False))
    ds = dict(opt['datasets']['test_1'], phase='test')
    m = create_model(opt)
    for data, png in zip(create_dataset(ds, opt), runs['se_on'][1]):
        assert os.path.splitext(os.path.basename(data['LR_path'][0]))[0] == png.stem
        m.feed_data(data, False)
        m.test_x8()
        want = util.tensor2img(m.fake_H.detach()[0].float().cpu())
        assert np.array_equal(px(png)[:, :, ::-1], want)


def test_training_driver_validates_with_self_ensemble(tmp_path):
    _gpu()
    from dasr_amd import train
    train.main(['-opt', _json_opt(tmp_path, 'se_train', True, {'self_ensemble': True})])
    root = tmp_path / 'experiments' / 'se_train'
    logs = [f for f in os.listdir(root) if f.startswith('val_') and f.endswith('.log')]
    assert logs and 'psnr:' in (root / logs[0]).read_text()
    assert len(list((root / 'val_images').rglob('*.png'))) == 4   # 2 images x 2 validation passes
    tr = [f for f in os.listdir(root) if f.startswith('train_') and f.endswith('.log')]
    assert 'x8 self-ensemble inference is on' in (root / tr[0]).read_text()
