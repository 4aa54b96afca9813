"""Data-parallel step on ONE GPU box: two processes (both on cuda:0) exchange gradients through torch.distributed
(gloo on CUDA tensors stands in for RCCL, which refuses two ranks on one device).  Everything else is the production
path: per-rank shard of the batch, 1/world folded into the wgrad reduction, bucketed all-reduce, replicated Adam.
The result must equal the single-process full-batch step (shard-mean gradient == full-batch gradient)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, case, out, streams, shard=None, env=None):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      DASR_STREAMS=str(streams))
    os.environ.update(env or {})
    import torch
    from oracle import fixtures
    from dasr_amd import options
    from dasr_amd.dist import DataParallelGroup, shard_minibatch
    from dasr_amd.models import create_model
    torch.cuda.set_device(0)
    dp = DataParallelGroup(backend='gloo') if world > 1 else None
    opt = fixtures.make_opt(case)
    opt['gpu_ids'] = [0]
    m = create_model(options.dict_to_nonedict(opt))
    kind = (fixtures.CASES[case] if isinstance(case, str) else case)['kind']
    from oracle import nets
    sd = fixtures.seeded_state_dict(m.netG.state_dict(), 1, 0.1)
    m.netG.load_state_dict(sd)
    if kind == 'dasr':
        m.netD_target.load_state_dict(fixtures.seeded_state_dict(m.netD_target.state_dict(), 2, 1.0))
        if m.netD_source is not None:
            m.netD_source.load_state_dict(fixtures.seeded_state_dict(m.netD_source.state_dict(), 3, 1.0))
    if dp:
        m.dp = dp
        for net in m.networks():
            dp.broadcast_params(net.params.flat)
            net.repack()
    batch = fixtures.make_batch(case)
    if dp:
        batch = shard_minibatch(batch, rank, world)
    elif shard is not None:   # single process on ONE rank's shard (what a replica of the reference's nn.DataParallel sees)
        batch = shard_minibatch(batch, shard[0], shard[1])
    grads = None
    for step in (1, 2):
        m.update_learning_rate()
        m.feed_data(batch, True) if kind == 'dasr' else m.feed_data(batch)
        m.optimize_parameters(step)
        if step == 1:
            torch.cuda.synchronize()
            grads = {'G': m.netG.params.grad_dict()}
            if kind == 'dasr':
                grads['D'] = m.netD_target.params.grad_dict()
                if m.netD_source is not None:
                    grads['D2'] = m.netD_source.params.grad_dict()
    torch.cuda.synchronize()
    res = {'G': m.netG.state_dict(), 'log': dict(m.get_current_log()), 'grads': grads}
    if kind == 'dasr':
        res['D'] = m.netD_target.state_dict()
        if m.netD_source is not None:
            res['D2'] = m.netD_source.state_dict()
    torch.save(res, out % (world, rank if shard is None else 100 + shard[0]))
    if dp:
        dp.barrier()


B16 = dict(kind='sr', nf=64, nb=2, n=16, lr=32)   # 8 crops per rank -> two sub-batch replicas of 4 under DASR_STREAMS=2
# relativistic GAN + source-domain discriminator, 2 + 2 samples: the per-pixel batch means of the logits must be GLOBAL means (two tiny
# all-reduces per loss evaluation), or the two-rank step would differ from the full-batch step
RAGAN4 = dict(kind='dasr', nf=32, nb=1, n=4, lr=32, fs='wavelet', d_in_nc=9, gan_src=0.02, ragan=True)


@pytest.mark.parametrize('case,streams', [('sr_nf64_nb2_b2_32', 1), ('dasr_wavelet_nf32_nb2_n2_32', 1), (B16, 1), (B16, 2), (RAGAN4, 1), (B16, 20)],
                         ids=['sr_b2-1stream', 'dasr_n2-1stream', 'sr_b16-1stream', 'sr_b16-2streams', 'dasr_ragan_srcD_n4', 'sr_b16-2streams-f16'])
def test_two_rank_step_equals_full_batch_step(case, streams, tmp_path, margins):
    """streams = 2: the DP x two-sub-batch-stream combination (replica gradient buffers summed, then reduced over the ranks);
    the single-process side runs the same DASR_STREAMS so that both schedules are compared like for like"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    out = str(tmp_path / 'w%d_r%d.pt')
    port = 29611 + (os.getpid() % 300)
    env = None
    if streams == 20:   # f16 storage of the dense blocks (DASR_RDB_PREC=2): every rank calibrates its own power-of-two gradient scale -- exact, so the ranks still agree
        streams, env = 2, {'DASR_RDB_PREC': '2'}
    mp.spawn(_worker, args=(1, port, case, out, streams, None, env), nprocs=1, join=True)
    mp.spawn(_worker, args=(2, port + 1, case, out, streams, None, env), nprocs=2, join=True)
    full = torch.load(out % (1, 0))
    r0, r1 = torch.load(out % (2, 0)), torch.load(out % (2, 1))
    for net in [k for k in ('G', 'D', 'D2') if k in full]:
        for k, v in full[net].items():
            assert torch.equal(r0[net][k], r1[net][k]), (net, k)  # replicas stay bit-identical
            if isinstance(case, dict) and case.get('ragan') and k == 'model.8.bias':
                continue   # relativistic loss: the true gradient of the last bias is 0, Adam turns its rounding noise into +-lr steps
            d = (r0[net][k] - v).abs().max().item()
            assert d <= 3.2e-4, (net, k, d)                      # Adam: sign flips of ~0 gradients move a weight by 2*lr
            assert ((r0[net][k] - v).abs() > 2e-5).float().mean().item() < 0.02, (net, k)
    dmax = max((r0[n_][k] - v).abs().max().item() for n_ in full if n_ in ('G', 'D', 'D2') for k, v in full[n_].items()
               if not (isinstance(case, dict) and case.get('ragan') and k == 'model.8.bias'))
    margins('DP 2 ranks vs full batch (%s, %d streams): max |dw| after 2 Adam steps %.2e (bound 3.2e-4)' % (
        case if isinstance(case, str) else ('sr_nf64_nb2_b16_32' if case['kind'] == 'sr' else 'dasr_ragan_srcD_n4'), streams, dmax))


# configs[3]'s per-rank partition: 2 source + 2 target crops per rank, [fake ; real] halves balanced on every rank
# (dist.shard_minibatch), InstanceNorm patch discriminator + VGG features: per-sample ops only, so 4 ranks == the full batch.  Four ranks, not
# the eight of the driver's scaling run: with the pytest process that makes five processes holding the device, and a shared GPU host allows six.
W4 = dict(kind='dasr', nf=32, nb=1, n=8, lr=32, fs='wavelet', d_in_nc=9)


def test_four_rank_step_equals_full_batch_step(tmp_path, margins):
    """four processes on this one device (gloo on CUDA tensors; RCCL refuses to share a device): the rank-0 weights after two steps equal the
    single-process step on the 8 + 8 crops, all four replicas bit-identical.  Replaces nn.DataParallel (networks.py:144-146) with more than two
    ranks; no multi-GPU hardware is available to the builder, this is the by-construction check."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    out = str(tmp_path / 'w%d_r%d.pt')
    port = 29111 + (os.getpid() % 300)
    mp.spawn(_worker, args=(1, port, W4, out, 1), nprocs=1, join=True)
    mp.spawn(_worker, args=(4, port + 1, W4, out, 1), nprocs=4, join=True)
    full = torch.load(out % (1, 0))
    rs = [torch.load(out % (4, r)) for r in range(4)]
    dmax = 0.0
    for net in ('G', 'D'):
        for k, v in full[net].items():
            for r in rs[1:]:
                assert torch.equal(rs[0][net][k], r[net][k]), (net, k)
            d = (rs[0][net][k] - v).abs().max().item()
            dmax = max(dmax, d)
            assert d <= 3.2e-4, (net, k, d)
            assert ((rs[0][net][k] - v).abs() > 2e-5).float().mean().item() < 0.02, (net, k)
        for k, g in full['grads'][net].items():   # step-1 gradients: mean over the 4 shards == full batch
            e = float((rs[0]['grads'][net][k] - g).norm() / (g.norm() + 1e-30))
            assert e < 2e-5 or float(g.norm()) < 1e-9, (net, k, e)
    margins('DP 4 ranks vs full batch (dasr n=8, 2 + 2 crops per rank): max |dw| after 2 Adam steps %.2e (bound 3.2e-4)' % dmax)


# BatchNorm source discriminator under data parallelism: batch statistics are PER RANK (as in the reference's nn.DataParallel replicas,
# gan_nets.py / DESIGN 4.7), so the two-rank step is NOT the full-batch step: it is the mean of the two single-rank steps on the shards
BN2 = dict(kind='dasr', nf=32, nb=1, n=4, lr=32, fs='gau', d_in_nc=3, gan_src=0.02, pairD='discriminator_vgg_128')


def test_two_rank_batchnorm_discriminator_uses_per_rank_statistics(tmp_path, margins):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    out = str(tmp_path / 'w%d_r%d.pt')
    port = 29711 + (os.getpid() % 300)
    for sh in (0, 1):
        mp.spawn(_worker, args=(1, port + sh, BN2, out, 1, (sh, 2)), nprocs=1, join=True)
    mp.spawn(_worker, args=(2, port + 2, BN2, out, 1), nprocs=2, join=True)
    s0, s1 = torch.load(out % (1, 100)), torch.load(out % (1, 101))
    r0, r1 = torch.load(out % (2, 0)), torch.load(out % (2, 1))
    worst = 0.0
    for net in ('G', 'D', 'D2'):
        for k, g0 in s0['grads'][net].items():
            want = 0.5 * (g0 + s1['grads'][net][k])
            got = r0['grads'][net][k]
            assert torch.equal(got, r1['grads'][net][k]), (net, k)
            e = float((got - want).norm() / (want.norm() + 1e-30))
            worst = max(worst, e)
            assert e < 1e-4 or float(want.norm()) < 1e-9, (net, k, e)
        for k, v in r0[net].items():
            if 'running' in k or 'num_batches' in k:
                continue   # BatchNorm buffers are per-rank state (each replica tracks the statistics of its own shard, like nn.DataParallel's replica 0)
            assert torch.equal(v, r1[net][k]), (net, k)
    # ... and the running statistics are per-rank state: each rank tracks ITS shard (they differ between the ranks; pooled statistics would not)
    k_rm = [k for k in r0['D2'] if k.endswith('running_mean')][0]
    assert not torch.allclose(r0['D2'][k_rm], r1['D2'][k_rm], rtol=1e-4, atol=1e-7)
    margins('DP 2 ranks, BatchNorm source discriminator: gradients == mean of the per-shard steps, worst rel err %.2e (bound 1e-4)' % worst)


CHAIN16 = dict(kind='sr', nf=64, nb=1, n=16, lr=128)   # 16 x 32 tiles fill the chip: the trunk runs as chained launches (dasr_conv_chain)


def _rccl_worker(rank, port, out, streams, use_dp, native=0):
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), DASR_STREAMS=str(abs(streams)),
                      DASR_RCCL_NATIVE=str(native))
    import torch
    from oracle import fixtures
    from dasr_amd import options
    from dasr_amd.dist import DataParallelGroup
    from dasr_amd.models import create_model
    torch.cuda.set_device(0)
    B16 = CHAIN16 if streams < 0 else globals()['B16']
    opt = fixtures.make_opt(B16)
    opt['gpu_ids'] = [0]
    m = create_model(options.dict_to_nonedict(opt))
    m.netG.load_state_dict(fixtures.seeded_state_dict(m.netG.state_dict(), 1, 0.1))
    if use_dp:
        m.dp = DataParallelGroup(backend='nccl', force=True)   # a real RCCL communicator of one rank
        assert m.dp.comm_stream is not None and (m.dp.native is not None) == bool(native)
        m.dp.broadcast_params(m.netG.params.flat)
    batch = fixtures.make_batch(B16)
    for step in (1, 2):
        m.update_learning_rate()
        m.feed_data(batch)
        m.optimize_parameters(step)
    torch.cuda.synchronize()
    if streams < 0:
        assert len(m._out_plans) == 1 and m._out_plans[0].chain is not None and m._out_plans[0].chain_b is not None
    torch.save({'G': m.netG.state_dict(), 'l_pix': m.get_current_log()['l_pix']}, out % int(use_dp))
    if use_dp:
        m.dp.barrier()
        assert m.dp.max_over_ranks(1.5) == 1.5


@pytest.mark.parametrize('streams,native', [(1, 0), (2, 0), (2, 1), (-1, 0)], ids=['1stream-torch', '2streams-torch', '2streams-c_abi', 'chained_trunk-torch'])
def test_rccl_exchange_path_single_rank(streams, native, tmp_path):
    """The RCCL code path (backend 'nccl': communication stream, bucket events, all-reduce enqueued behind the boundary events of
    both replica streams) executed for real on this one-GPU box with a communicator of ONE rank (RCCL refuses two ranks on one
    device).  The exchange is the identity, so the step must reproduce the no-DP step bit for bit.
    chained_trunk: a shape whose trunk runs as persistent chained launches -- the exchange of the bucket that is complete in front of the data-gradient
    chain is held back until the chain has been enqueued (rrdbnet._Plan.run_backward_dp; test_chained_step_survives_interference_on_the_communication_stream)."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    if streams < 0 and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip('the chained launches need a whole 256-CU MI355X (RRDBNetHIP.chain_ok)')
    import torch.multiprocessing as mp
    out = str(tmp_path / 'rccl_%d.pt')
    port = 29411 + (os.getpid() % 300) + abs(streams) + (7 if streams < 0 else 0)
    mp.spawn(_rccl_worker, args=(port, out, streams, False), nprocs=1, join=True)
    mp.spawn(_rccl_worker, args=(port, out, streams, True, native), nprocs=1, join=True)
    a, b = torch.load(out % 0), torch.load(out % 1)
    assert a['l_pix'] == b['l_pix']   # (a fixed-order grid sum since round 5)
    for k, v in a['G'].items():
        assert torch.equal(v, b['G'][k]), k


def _interference_worker(rank, port, out, spin):
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), DASR_STREAMS='2', DASR_RCCL_NATIVE='0')
    import torch
    from oracle import fixtures
    from dasr_amd import _lib, options
    from dasr_amd.dist import DataParallelGroup
    from dasr_amd.models import create_model
    torch.cuda.set_device(0)
    opt = fixtures.make_opt(CHAIN16)
    opt['gpu_ids'] = [0]
    m = create_model(options.dict_to_nonedict(opt))
    m.netG.load_state_dict(fixtures.seeded_state_dict(m.netG.state_dict(), 1, 0.1))
    m.dp = DataParallelGroup(backend='nccl', force=True)
    calls = []
    if spin:
        real = m.dp.all_reduce_here

        def noisy(flat_slice):   # every collective drags a kernel along that pins 32 workgroup slots (16 CUs' worth of one of the two slots) for 20 ms
            _lib.check(_lib.bench_lib().dasr_probe_spin(32, 20000, torch.cuda.current_stream().cuda_stream), 'spin')
            calls.append(int(flat_slice.numel()))
            real(flat_slice)
        m.dp.all_reduce_here = noisy
    batch = fixtures.make_batch(CHAIN16)
    for step in (1, 2, 3):
        m.update_learning_rate()
        m.feed_data(batch)
        m.optimize_parameters(step)
    torch.cuda.synchronize()
    p = m._out_plans[0]
    assert len(m._out_plans) == 1 and p.chain is not None and p.chain_b is not None
    assert not spin or len(calls) >= 3 * 3
    torch.save({'G': m.netG.state_dict(), 'grad': m.netG.params.grad.cpu(), 'l_pix': m.get_current_log()['l_pix'], 'err': int(m.netG.chain_err.item())}, out % int(spin))


def test_chained_step_survives_interference_on_the_communication_stream(tmp_path):
    """VERDICT r04 item 3 / ADVICE r04: dasr_conv_chain needs all 512 workgroups resident, 64 per XCD; a collective's kernels on the communication
    stream hold workgroup slots.  The data-parallel schedule therefore never has a collective in flight while a chained launch runs
    (rrdbnet._Plan.run_backward_dp holds the bucket in front of the data-gradient chain back; dp.wait() in front of the optimiser covers the next forward
    chain).  Here every collective of a one-rank RCCL group is accompanied by a kernel that pins 32 workgroup slots for 20 ms on the communication
    stream -- with round 4's schedule that kernel sat on the chip when the data-gradient chain started.  Three steps: error word 0, weights / gradients /
    logged loss bit-identical to the quiet run."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip('the chained launches need a whole 256-CU MI355X (RRDBNetHIP.chain_ok)')
    import torch.multiprocessing as mp
    out = str(tmp_path / 'intf_%d.pt')
    port = 29811 + (os.getpid() % 150)
    mp.spawn(_interference_worker, args=(port, out, False), nprocs=1, join=True)
    mp.spawn(_interference_worker, args=(port + 1, out, True), nprocs=1, join=True)
    a, b = torch.load(out % 0), torch.load(out % 1)
    assert a['err'] == 0 and b['err'] == 0
    assert a['l_pix'] == b['l_pix'] and torch.equal(a['grad'], b['grad'])
    for k, v in a['G'].items():
        assert torch.equal(v, b['G'][k]), k


def _dsn_worker(rank, world, port, out, ragan=False, n_total=None, wgan=False):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch
    from dasr_amd.dist import DataParallelGroup
    from dasr_amd.dsn_model import DSNModel
    from oracle.gen_golden_dsn import dsn_state, dsn_batch
    torch.cuda.set_device(0)
    dp = DataParallelGroup(backend='gloo') if world > 1 else None
    torch.manual_seed(0)
    m = DSNModel(dict(filter='wavelet', w_per=0.01, vgg_seed=78, allow_random_perceptual=True, ragan=ragan, wgan=wgan))
    m.netG.load_state_dict(dsn_state(m.netG.state_dict(), 21, 0.5))
    m.netD.load_state_dict(dsn_state(m.netD.state_dict(), 22, 1.0))
    if dp:
        m.dp = dp
        for net in m.networks():
            dp.broadcast_params(net.params.flat)
            net.repack()
    n = n_total or (4 if (ragan or wgan) else 2)   # relativistic / gradient penalty: two samples per rank, so the GLOBAL batch means (norm) differ from the per-rank ones
    hr, bic, real = dsn_batch(dict(n=n, crop=128))  # VGG16's five pools need >= 32 px LR
    if dp:
        per = n // world
        hr, bic, real = (t[rank * per:(rank + 1) * per] for t in (hr, bic, real))
    for _ in range(2):
        m.iteration(hr.cuda(), bic.cuda(), real.cuda())
    torch.cuda.synchronize()
    torch.save({'G': m.netG.state_dict(), 'D': m.netD.state_dict()}, out % (world, rank))
    if dp:
        dp.barrier()


@pytest.mark.parametrize('mode', ['plain', 'ragan', 'wgan', 'wgan_ragan'])
def test_dsn_two_rank_iteration_equals_full_batch(mode, tmp_path):
    """ragan (round 3): D(x, y) = sigmoid(D(x) - mean_n D(y)) couples the samples; under data parallelism the per-pixel batch sums are all-reduced
    between the loss stages (dsn_model.py::iteration), so two ranks with two samples each must reproduce the four-sample step.
    wgan (round 5): the gradient penalty's ONE norm over the global batch -- the ranks' sums of squares are all-reduced between the norm and the
    tangent / reverse pass, the mixing weight is rank 0's draw."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    ragan, wgan = mode in ('ragan', 'wgan_ragan'), mode in ('wgan', 'wgan_ragan')
    out = str(tmp_path / 'dsn_w%d_r%d.pt')
    port = 29911 + (os.getpid() % 300) + 2 * ['plain', 'ragan', 'wgan', 'wgan_ragan'].index(mode)
    mp.spawn(_dsn_worker, args=(1, port, out, ragan, None, wgan), nprocs=1, join=True)
    mp.spawn(_dsn_worker, args=(2, port + 1, out, ragan, None, wgan), nprocs=2, join=True)
    full = torch.load(out % (1, 0))
    r0, r1 = torch.load(out % (2, 0)), torch.load(out % (2, 1))
    for net in ('G', 'D'):
        for k, v in full[net].items():
            assert torch.equal(r0[net][k], r1[net][k]), (net, k)
            if ragan and k == 'net.net.8.bias':
                continue  # relativistic loss: shifting every logit changes nothing, the true gradient of the last bias is 0
            if k in ('net.net.2.bias', 'net.net.5.bias'):
                continue  # bias in front of an InstanceNorm: true gradient 0, Adam turns the rounding noise into +-lr steps (no effect on D)
            d = (r0[net][k] - v).abs().max().item()
            assert d <= 4.2e-4, (net, k, d)   # two Adam steps at lr 1e-4: a flipped ~0 gradient moves a weight by <= 2*lr per step
            if v.numel() > 64:
                assert ((r0[net][k] - v).abs() > 2e-5).float().mean().item() < 0.03, (net, k)


def test_dsn_four_rank_iteration_equals_full_batch(tmp_path):
    """configs[4]'s data-parallel leg by construction: batch 4 -> ONE crop per rank (InstanceNorm discriminator on a 1-image
    rank, per-sample ops only); four processes on one device over gloo reproduce the 4-crop iteration (four, not eight: with the pytest process
    that makes five processes holding the device, and a shared GPU host allows six)"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import torch.multiprocessing as mp
    out = str(tmp_path / 'dsn_w%d_r%d.pt')
    port = 29311 + (os.getpid() % 300)
    mp.spawn(_dsn_worker, args=(1, port, out, False, 4), nprocs=1, join=True)
    mp.spawn(_dsn_worker, args=(4, port + 1, out, False, 4), nprocs=4, join=True)
    full = torch.load(out % (1, 0))
    rs = [torch.load(out % (4, r)) for r in range(4)]
    for net in ('G', 'D'):
        for k, v in full[net].items():
            for r in rs[1:]:
                assert torch.equal(rs[0][net][k], r[net][k]), (net, k)
            if k in ('net.net.2.bias', 'net.net.5.bias'):
                continue  # bias in front of an InstanceNorm: true gradient 0
            d = (rs[0][net][k] - v).abs().max().item()
            assert d <= 4.2e-4, (net, k, d)
            if v.numel() > 64:
                assert ((rs[0][net][k] - v).abs() > 2e-5).float().mean().item() < 0.03, (net, k)
