"""GPU tests of the SRResNet generator (which_model_G: sr_resnet): the fused residual-block kernel (dasr_resblock) against the two-launch
composition and fp64 torch, the SRModel step against an fp32 torch restatement run by the oracle trainers and against the
reference fixtures (scripts/gen_golden_srresnet.py), the two-stream sub-batch schedule, inference / checkpoints and the CLIs.

Tolerances are the north_star's: activations 1e-3, gradients 1e-2 relative (normwise per tensor)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-3
GRAD_TOL = 1e-2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


# ---- fp32 torch restatement of the public SRResNet architecture (CNA, ReLU, PixelShuffle x 2), in the reference's state_dict layout ----------
class _Shortcut(nn.Module):
    def __init__(self, sub):
        super().__init__()
        self.sub = sub

    def forward(self, x):
        return x + self.sub(x)


class _ResBlock(nn.Module):
    def __init__(self, nf):
        super().__init__()
        self.res = nn.Sequential(nn.Conv2d(nf, nf, 3, 1, 1), nn.ReLU(), nn.Conv2d(nf, nf, 3, 1, 1))

    def forward(self, x):
        return x + self.res(x)


class TorchSRResNet(nn.Module):
    def __init__(self, nf, nb, in_nc=3, out_nc=3):
        super().__init__()
        conv = lambda a, b: nn.Conv2d(a, b, 3, 1, 1)
        self.model = nn.Sequential(conv(in_nc, nf), _Shortcut(nn.Sequential(*[_ResBlock(nf) for _ in range(nb)], conv(nf, nf))),
                                   conv(nf, 4 * nf), nn.PixelShuffle(2), nn.ReLU(), conv(nf, 4 * nf), nn.PixelShuffle(2), nn.ReLU(),
                                   conv(nf, nf), nn.ReLU(), conv(nf, out_nc))

    def forward(self, x):
        return self.model(x)


def _fixture(golden_dir, name):
    f = np.load(os.path.join(golden_dir, name + '.npz'))
    return f, json.loads(str(f['case_json']))


def _opt(c):
    from oracle import fixtures
    opt = fixtures.make_opt(c)
    opt['network_G'].update(which_model_G='sr_resnet', upsample_mode=None)
    return opt


# ---- kernel ---------------------------------------------------------------------------------------------------------------------------
KSHAPES = [(1, 16, 16), (2, 32, 32), (1, 24, 40), (16, 32, 32), (1, 128, 128)]


@pytest.mark.parametrize('train', [True, False], ids=['train', 'infer'])
@pytest.mark.parametrize('shape', KSHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_resblock_kernel_bit_identical_to_two_conv_launches(shape, train, margins):
    dev = _gpu()
    from oracle import fixtures
    from dasr_amd import _lib
    from dasr_amd.engine import BTensor, OpList, conv_op, _stream, NULL_T
    from dasr_amd.srresnet import SRResNetHIP
    N, h, w = shape
    net = SRResNetHIP(nf=64, nb=1, device=dev, fused_blocks=False)
    sd = fixtures.seeded_state_dict(TorchSRResNet(64, 1).state_dict(), 7, 1.0)   # scale 1: h and the residual are O(1), the ReLU cuts half of h
    net.load_state_dict(sd)
    g = torch.Generator(device='cpu').manual_seed(N * 1000 + h + w)
    x = torch.randn(N, 64, h, w, generator=g)
    B = lambda f32: BTensor(N, 64, h, w, f32, dev)
    x32, x16 = B(True), B(False)
    x32.t.copy_(x.view(N, 4, 16, h, w).permute(0, 1, 3, 4, 2))
    x16.t.copy_(x32.t)
    P, pk, pack = net.params, net.pk, net.pack
    # two-launch composition
    h_a, y32_a, y16_a = B(False), B(True), B(False)
    ol = OpList()
    ol.add(conv_op(pack, pk[(0, 0)], x16.view(), False, 64, h, w, h, w, N, bias=P.ptr('model.1.sub.0.res.0.bias'), act=1, slope=0.0, out_bf16=h_a.view()))
    ol.add(conv_op(pack, pk[(0, 2)], h_a.view(), False, 64, h, w, h, w, N, bias=P.ptr('model.1.sub.0.res.2.bias'), res1=x32.view(), beta1=1.0,
                   out_f32=y32_a.view(), out_bf16=y16_a.view()))
    ol.run()
    # fused launch, through ctypes
    h_b, y32_b, y16_b = B(False), B(True), B(False)
    h_b.t.fill_(7.0)
    prm = _lib.ResblockParams()
    prm.x16, prm.x32 = x16.view(), x32.view()
    prm.w0, prm.b0 = pack.ptr(pk[(0, 0)]), P.ptr('model.1.sub.0.res.0.bias')
    prm.w1, prm.b1 = pack.ptr(pk[(0, 2)]), P.ptr('model.1.sub.0.res.2.bias')
    prm.y32, prm.y16, prm.h = y32_b.view(), y16_b.view(), (h_b.view() if train else NULL_T)
    prm.N, prm.H, prm.W, prm.res_scale, prm.slope = N, h, w, 1.0, 0.0
    _lib.check(_lib.lib().dasr_resblock(C.byref(prm), _stream()), 'dasr_resblock')
    torch.cuda.synchronize()
    assert torch.equal(y32_a.t.view(torch.int32), y32_b.t.view(torch.int32))
    assert torch.equal(y16_a.t.view(torch.int16), y16_b.t.view(torch.int16))
    if train:
        assert torch.equal(h_a.t.view(torch.int16), h_b.t.view(torch.int16))
    else:
        assert bool((h_b.t == 7.0).all())   # inference: h is not stored
    # against fp64 torch on the same bf16 operands: the only roundings left are h's bf16 and the fp32 accumulation
    bf = lambda t: t.to(torch.bfloat16).double()
    w0, w2 = bf(sd['model.1.sub.0.res.0.weight']), bf(sd['model.1.sub.0.res.2.weight'])
    b0, b2 = sd['model.1.sub.0.res.0.bias'].double(), sd['model.1.sub.0.res.2.bias'].double()
    hr = F.relu(F.conv2d(bf(x), w0, b0, padding=1))
    yr = x.double() + F.conv2d(hr, w2, b2, padding=1)
    e_h = rel(h_b.nchw().cpu(), hr) if train else 0.0
    e_y = rel(y32_b.nchw().cpu() - x.double(), yr - x.double())
    margins('dasr_resblock %dx%dx%d %s: h rel err %.2e, residual rel err %.2e vs fp64 (tol 1e-2)' % (N, h, w, 'train' if train else 'infer', e_h, e_y))
    assert e_h < 1e-2 and e_y < 1e-2


# ---- SRModel step ---------------------------------------------------------------------------------------------------------------------
TAPS = (0, 1, 15)


def _oracle_sr(c, steps=2, dasr=False):
    from oracle import fixtures, trainers
    netG = TorchSRResNet(c['nf'], c['nb'])
    sd0 = fixtures.seeded_state_dict(netG.state_dict(), 1, 0.1)
    netG.load_state_dict(sd0)
    t = trainers.SRTrainer(fixtures.make_opt(c), netG=netG)
    batch = fixtures.make_batch(c)
    taps = {}
    def hook(name):
        def f(m, i, o):   # (must return None: a returned tensor would replace the module output)
            taps.setdefault(name, o.detach().clone())
        return f

    hs = [netG.model[0].register_forward_hook(hook('fea_conv')), netG.model[1].register_forward_hook(hook('trunk_out'))]
    hs += [netG.model[1].sub[i].register_forward_hook(hook('trunk_%d' % i)) for i in TAPS if i < c['nb']]
    out = {'sd0': sd0, 'batch': batch, 'logs': []}
    for step in range(1, steps + 1):
        t.update_learning_rate()
        t.feed_data(batch)
        t.optimize_parameters(step)
        out['logs'].append(t.log['l_pix'])
        if step == 1:
            for hh in hs:
                hh.remove()
            out['taps'], out['sr'] = taps, t.fake_H.detach().clone()
            out['grads'] = [p.grad.detach().clone() for p in netG.parameters()]
    out['sdN'] = {k: v.detach().clone() for k, v in netG.state_dict().items()}
    return out


def _hip_sr(c, want, fused, steps=2):
    from dasr_amd import options
    from dasr_amd.models import create_model
    opt = _opt(c)
    opt['gpu_ids'] = [0]
    m = create_model(options.dict_to_nonedict(opt))
    m.netG.fused_blocks = None if fused == 'f16' else fused
    assert m.netG.rdb_f16 == (fused == 'f16')
    m.netG.load_state_dict(want['sd0'])
    m.netG.debug_taps = tuple(i for i in TAPS if i < c['nb'])
    res = {'logs': []}
    for step in range(1, steps + 1):
        m.update_learning_rate()
        m.feed_data(want['batch'])
        m.optimize_parameters(step)
        res['logs'].append(m.get_current_log()['l_pix'])
        if step == 1:
            plans = m._out_plans
            assert all(p.fused == (fused is True) for p in plans)
            cat = lambda f: torch.cat([f(p).cpu() for p in plans], 0)
            res['taps'] = {'fea_conv': cat(lambda p: p.fea.nchw()), 'trunk_out': cat(lambda p: p.t0.nchw())}
            for i in m.netG.debug_taps:
                res['taps']['trunk_%d' % i] = cat(lambda p: p.taps[i].nchw())
            res['sr'] = m.fake_H.cpu().clone()
            res['grads'] = m.netG.params.grad_dict()
    res['sdN'] = m.netG.state_dict()
    return res


@pytest.mark.parametrize('fused', [True, False, 'f16'], ids=['fused', 'per_layer', 'f16_trunk'])
@pytest.mark.parametrize('name', ['srresnet_nf64_nb2_b2_32', 'srresnet_nf64_nb16_b2_32', 'srresnet_nf64_nb2_b1_24x40'])
def test_srresnet_sr_step_matches_oracle_and_reference_fixture(name, fused, golden_dir, margins, monkeypatch):
    _gpu()
    if fused == 'f16':   # f16 storage of the trunk's shadows (DASR_RDB_PREC=2): two launches per block, gradient scale calibrated on step 1
        monkeypatch.setenv('DASR_RDB_PREC', '2')
    torch.set_num_threads(8)
    gold, c = _fixture(golden_dir, name)
    want = _oracle_sr(c)
    # the restatement itself against the reference's numbers
    np.testing.assert_allclose(want['logs'], gold['logs'][:, 0], rtol=1e-5)
    np.testing.assert_allclose([float(g.double().norm()) for g in want['grads']], gold['gradG_norm'], rtol=1e-4)
    got = _hip_sr(c, want, fused)
    errs = {k: rel(got['taps'][k], want['taps'][k]) for k in got['taps']}
    errs['sr'] = rel(got['sr'], want['sr'])
    margins('%s %s activations: %s (tol %.0e)' % (name, {True: 'fused', False: 'per-layer', 'f16': 'f16-trunk'}[fused], ' '.join('%s %.2e' % kv for kv in errs.items()), ACT_TOL))
    for k, e in errs.items():
        assert e < ACT_TOL, (k, e)
        if k != 'sr':
            np.testing.assert_allclose(float(got['taps'][k].double().norm()), float(gold['tap_norm/' + k]), rtol=ACT_TOL)
    worst, wk = 0.0, None
    for (k, gv), gw in zip(got['grads'].items(), want['grads']):
        r = rel(gv, gw)
        if r > worst:
            worst, wk = r, k
    margins('%s %s gradients: worst normwise rel err %.2e at %s (tol %.0e)' % (name, {True: 'fused', False: 'per-layer', 'f16': 'f16-trunk'}[fused], worst, wk, GRAD_TOL))
    assert worst < GRAD_TOL, (wk, worst)
    np.testing.assert_allclose([float(g.double().norm()) for g in got['grads'].values()], gold['gradG_norm'], rtol=GRAD_TOL)
    np.testing.assert_allclose(got['logs'], gold['logs'][:, 0], rtol=1e-4)
    dmax = 0.0
    for k, v in got['sdN'].items():
        d = (v - want['sdN'][k]).abs()
        dmax = max(dmax, float(d.max()))
        assert float(d.max()) <= 3.2e-4, k
        assert float((d > 2e-5).float().mean()) < 0.02, k
    margins('%s %s weights after 2 Adam steps: max |dw| %.2e (bound 3.2e-4)' % (name, {True: 'fused', False: 'per-layer', 'f16': 'f16-trunk'}[fused], dmax))


def test_srresnet_sr_step_two_sub_batch_replicas(margins):
    """batch 8: the trainer's two-stream schedule (two replica plans, private gradient buffer + add_flat), two steps, against the restatement"""
    _gpu()
    c = dict(kind='sr', nf=64, nb=2, n=8, lr=32)
    want = _oracle_sr(c)
    got = _hip_sr(c, want, True)
    assert rel(got['sr'], want['sr']) < ACT_TOL
    worst = max(rel(gv, gw) for gv, gw in zip(got['grads'].values(), want['grads']))
    margins('srresnet_nf64_nb2_b8_32 (two replicas): sr %.2e, worst gradient %.2e' % (rel(got['sr'], want['sr']), worst))
    assert worst < GRAD_TOL
    np.testing.assert_allclose(got['logs'], want['logs'], rtol=1e-4)


def test_srresnet_fused_and_per_layer_steps_agree(golden_dir):
    """the two forms are the same arithmetic in the forward (bit-identical blocks) and share the backward: the same step"""
    _gpu()
    gold, c = _fixture(golden_dir, 'srresnet_nf64_nb2_b2_32')
    want = _oracle_sr(c, steps=1)
    a, b = _hip_sr(c, want, True, steps=1), _hip_sr(c, want, False, steps=1)
    assert torch.equal(a['sr'], b['sr'])
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), k
    assert a['logs'] == b['logs']


# ---- inference, checkpoints ---------------------------------------------------------------------------------------------------------------
def test_forward_chop_and_checkpoint_reload(tmp_path):
    dev = _gpu()
    from oracle import fixtures
    from dasr_amd import options
    from dasr_amd.models import create_model
    from dasr_amd.util import forward_chop
    c = dict(kind='sr', nf=64, nb=2, n=1, lr=(52, 44))
    opt = _opt(c)
    opt['gpu_ids'] = [0]
    opt['path']['models'] = str(tmp_path)
    m = create_model(options.dict_to_nonedict(opt))
    sd0 = fixtures.seeded_state_dict(TorchSRResNet(64, 2).state_dict(), 1, 0.1)
    m.netG.load_state_dict(sd0)
    x = torch.rand(1, 3, 52, 44, generator=torch.Generator().manual_seed(3)).to(dev)
    y = m.netG.forward(x).clone()
    ref = TorchSRResNet(64, 2)
    ref.load_state_dict(sd0)
    with torch.no_grad():
        assert rel(y.cpu(), ref(x.cpu())) < ACT_TOL
    yc = forward_chop(x, 4, lambda t: m.netG.forward(t).clone(), min_size=1000)   # quadrants of 36 x 32 (shave 10)
    assert rel(yc, y) < ACT_TOL
    m.save(1)
    sd = torch.load(os.path.join(str(tmp_path), '1_G.pth'))
    ref2 = TorchSRResNet(64, 2)
    ref2.load_state_dict(sd)   # strict: reference key names and shapes
    opt_t = _opt(c)
    opt_t.update(gpu_ids=[0], is_train=False)
    opt_t['path']['pretrain_model_G'] = os.path.join(str(tmp_path), '1_G.pth')
    m2 = create_model(options.dict_to_nonedict(opt_t))
    assert torch.equal(m2.netG.forward(x).clone(), y)


# ---- CLIs ---------------------------------------------------------------------------------------------------------------------------
def _json_opt(tmp_path, name, is_train, extra=None):
    """a train_SRResNet.json / test_SRResNet.json-shaped option file on synthetic data"""
    opt = {
        'name': name, 'use_tb_logger': False, 'model': 'sr', 'scale': 4, 'gpu_ids': [0], 'chop': False, 'val_lpips': False, 'datasets': {},
        'path': {'root': str(tmp_path), 'pretrain_model_G': None},
        'network_G': {'which_model_G': 'sr_resnet', 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': 16, 'in_nc': 3, 'out_nc': 3},
    }
    if is_train:
        opt['datasets'] = {'train': {'name': 'syn', 'mode': 'synthetic', 'batch_size': 16, 'HR_size': 128, 'n_batches': 8},
                           'val': {'name': 'synval', 'mode': 'synthetic', 'n_images': 2, 'LR_size': 24}}
        opt['train'] = {'lr_G': 2e-4, 'lr_scheme': 'MultiStepLR', 'lr_steps': [200000, 400000, 600000, 800000], 'lr_gamma': 0.5,
                        'pixel_criterion': 'l1', 'pixel_weight': 1.0, 'val_freq': 2, 'manual_seed': 0, 'niter': 4}
        opt['logger'] = {'print_freq': 2, 'save_checkpoint_freq': 4}
    else:
        opt['datasets'] = {'test_1': {'name': 'synset', 'mode': 'synthetic', 'n_images': 2, 'LR_size': 64}}
    opt.update(extra or {})
    p = tmp_path / (name + '.json')
    p.write_text(json.dumps(opt))
    return str(p)


def test_train_and_test_cli_with_sr_resnet(tmp_path):
    _gpu()
    from dasr_amd import train, test as dtest
    train.main(['-opt', _json_opt(tmp_path, 'srresnet_train', True)])
    root = tmp_path / 'experiments' / 'srresnet_train'
    logs = [f for f in os.listdir(root) if f.startswith('val_') and f.endswith('.log')]
    assert logs and 'psnr:' in (root / logs[0]).read_text()
    g_path = root / 'models' / 'latest_G.pth'
    sd = torch.load(str(g_path))
    TorchSRResNet(64, 16).load_state_dict(sd)   # reference key names
    s = dtest.main(['-opt', _json_opt(tmp_path, 'srresnet_test', False, {'path': {'root': str(tmp_path), 'pretrain_model_G': str(g_path)}})])['synset']
    assert all(np.isfinite(s[k]) for k in ('psnr', 'ssim')) and 5 < s['psnr'] < 60
    s2 = dtest.main(['-opt', _json_opt(tmp_path, 'srresnet_test_chop', False, {'chop': True, 'val_lpips': True, 'allow_random_perceptual': True,
                                                                                'path': {'root': str(tmp_path), 'pretrain_model_G': str(g_path)}})])['synset']
    assert abs(s2['psnr'] - s['psnr']) < 1.0 and np.isfinite(s2['lpips'])


# ---- data parallelism ---------------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, c, out, streams, env):
    """one rank (world 1: the full-batch reference) of the SRModel step with sr_resnet; gloo on CUDA tensors stands in for RCCL (two ranks share
    this device), everything else is the production path (shard, 1/world in the reductions, bucketed exchange, replicated Adam)"""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), DASR_STREAMS=str(streams))
    os.environ.update(env)
    import torch
    from oracle import fixtures
    from dasr_amd import options
    from dasr_amd.dist import DataParallelGroup, shard_minibatch
    from dasr_amd.models import create_model
    torch.cuda.set_device(0)
    dp = DataParallelGroup(backend='gloo') if world > 1 else None
    opt = _opt(c)
    opt['gpu_ids'] = [0]
    m = create_model(options.dict_to_nonedict(opt))
    m.netG.load_state_dict(fixtures.seeded_state_dict(m.netG.state_dict(), 1, 0.1))
    batch = fixtures.make_batch(c)
    if dp:
        m.dp = dp
        dp.broadcast_params(m.netG.params.flat)
        m.netG.repack()
        batch = shard_minibatch(batch, rank, world)
    for step in (1, 2):
        m.update_learning_rate()
        m.feed_data(batch)
        m.optimize_parameters(step)
        if step == 1:
            torch.cuda.synchronize()
            grads = m.netG.params.grad_dict()
    torch.cuda.synchronize()
    torch.save({'G': m.netG.state_dict(), 'grads': grads, 'log': dict(m.get_current_log())}, out % (world, rank))
    if dp:
        dp.barrier()


DP_B16 = dict(kind='sr', nf=64, nb=2, n=16, lr=32)   # 8 crops per rank: two sub-batch replicas of 4 under DASR_STREAMS=2


@pytest.mark.parametrize('streams,prec', [(1, '1'), (2, '1'), (2, '2')], ids=['1stream', '2streams', '2streams-f16trunk'])
def test_two_rank_step_equals_full_batch_step(streams, prec, tmp_path, margins):
    """two gloo ranks (at most three processes on the device) against one process over the whole batch: the step-1 gradients (every bucket of the
    plan's gradient layout, the 1/world factor) and the weights after two Adam steps"""
    _gpu()
    import torch.multiprocessing as mp
    out = str(tmp_path / 'w%d_r%d.pt')
    port = 29211 + (os.getpid() % 300)
    env = {'DASR_RDB_PREC': prec}
    mp.spawn(_dp_worker, args=(1, port, DP_B16, out, streams, env), nprocs=1, join=True)
    mp.spawn(_dp_worker, args=(2, port + 1, DP_B16, out, streams, env), nprocs=2, join=True)
    full = torch.load(out % (1, 0))
    r0, r1 = torch.load(out % (2, 0)), torch.load(out % (2, 1))
    worst = 0.0
    for k, g in full['grads'].items():
        assert torch.equal(r0['grads'][k], r1['grads'][k]), k
        e = rel(r0['grads'][k], g)
        worst = max(worst, e)
        assert e < 1e-5, (k, e)   # the same arithmetic up to the order of the final sums (shard means, then the exchange)
    dmax = 0.0
    for k, v in full['G'].items():
        assert torch.equal(r0['G'][k], r1['G'][k]), k   # replicas stay bit-identical
        d = (r0['G'][k] - v).abs()
        dmax = max(dmax, float(d.max()))
        assert float(d.max()) <= 3.2e-4, k
        assert float((d > 2e-5).float().mean()) < 0.02, k
    # each rank logs the loss of its own shard (equal halves): their mean is the full-batch loss
    np.testing.assert_allclose(0.5 * (r0['log']['l_pix'] + r1['log']['l_pix']), full['log']['l_pix'], rtol=1e-5)
    margins('sr_resnet DP 2 ranks vs full batch (%d streams, trunk prec %s): worst gradient rel err %.2e, max |dw| after 2 steps %.2e'
            % (streams, prec, worst, dmax))
