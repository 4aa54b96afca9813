"""GPU tests of post-recording patches (engine.patch): the data-parallel gradient scale reaches every recorded list of a step.

Exact arithmetic: the scale multiplies an fp32 sum in the last step of every gradient (the weight-gradient reduction, the PReLU-slope and BatchNorm
parameter reductions), and 0.5 x an fp32 number is exact unless it is subnormal.  With the learning rate at 0 (weights fixed) and the same inputs, the
gradient buffer of a step at scale 0.5 is therefore BIT FOR BIT 0.5 x the buffer at scale 1 -- if the patched scale reached every list the step runs
(SRModel: whole_step of every sub-batch replica and the shared store's phase; DSN: d_bwd, g_bwd = [.. + g.bwd]).  A list that kept its old image shows
up as entries that did not halve.  Control first: two steps at scale 1 are bit-identical (the reductions are deterministic)."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda')


def _assert_halved(name, g1, g1b, g_half):
    small = (g1 != 0) & (g1.abs() < 2.0 ** -120)
    assert not bool(small.any()), '%s: %d entries of the scale-1 gradient are too close to the subnormals to halve exactly' % (name, int(small.sum()))
    assert bool((g1 != 0).any()), name
    assert torch.equal(g1, g1b), '%s: two steps at scale 1 differ in %d of %d entries (control)' % (name, int((g1 != g1b).sum()), g1.numel())
    stale = g_half != 0.5 * g1
    assert not bool(stale.any()), '%s: %d of %d entries are not 0.5 x the scale-1 gradient (%d of them still at scale 1)' % (
        name, int(stale.sum()), g1.numel(), int((stale & (g_half == g1)).sum()))


@pytest.mark.parametrize('nb', [1, 2])
def test_sr_step_on_two_streams_takes_a_patched_gradient_scale(nb, monkeypatch):
    """8 crops of 16 x 16 with f16 dense blocks: the smallest batch that runs two sub-batch replicas (and never chains).  The flat gradient buffer covers
    the HR tail and the stream convs (per replica, through whole_step) and the dense blocks (through the shared store's phase)."""
    _gpu()
    monkeypatch.setenv('DASR_RDB_PREC', '2')
    from oracle import fixtures
    from dasr_amd import options
    from dasr_amd.models import create_model
    case = dict(kind='sr', nf=64, nb=nb, n=8, lr=16)
    opt = fixtures.make_opt(case)
    opt['gpu_ids'] = [0]
    opt['train']['lr_G'] = 0.0
    m = create_model(options.dict_to_nonedict(opt))
    m.netG.load_state_dict(fixtures.seeded_state_dict(m.netG.state_dict(), 1, 0.1))
    batch = fixtures.make_batch(case)
    w0 = m.netG.params.flat.clone()
    grads = []
    for step in (1, 2, 3):
        if step == 3:
            plans = m._out_plans
            assert len(plans) == 2 and plans[0].store is plans[1].store and all(hasattr(p, 'whole_step') for p in plans)
            assert [p.set_grad_scale(0.5) for p in plans] == [True, True] and plans[0].store.set_grad_scale(0.5)
            recorded = [(p.whole_step, p.whole_step_gen) for p in plans]
        m.update_learning_rate()
        m.feed_data(batch)
        m.optimize_parameters(step)
        torch.cuda.synchronize()
        grads.append(m.netG.params.grad.clone())
    m.get_current_log()   # (raises if a gradient overflowed)
    assert [(p.whole_step, p.whole_step_gen) for p in m._out_plans] == recorded   # the recorded step lists were refreshed, not re-recorded
    assert torch.equal(m.netG.params.flat, w0)
    _assert_halved('SR netG', *grads)


@pytest.mark.parametrize('norm', ['Instance', 'Batch'])
def test_dsn_iteration_takes_a_patched_gradient_scale(norm):
    """generator (weight gradients, PReLU slopes of both forms, the fused slope reduction) and discriminator (weight gradients; Batch: dgamma / dbeta) of one DSN iteration"""
    dev = _gpu()
    from dasr_amd.dsn_model import DSNModel
    torch.manual_seed(0)
    m = DSNModel(dict(w_per=0.0, learning_rate=0.0, n_res_blocks=2, norm_layer=norm), device=dev)
    g = torch.Generator().manual_seed(1)
    hr, bic, real = (torch.rand(2, 3, s, s, generator=g).to(dev) for s in (32, 8, 8))
    w0 = [n.params.flat.clone() for n in m.networks()]
    grads = []
    for it in (1, 2, 3):
        if it == 3:
            # what a process group that appears with two ranks does: iteration() finds the plan at the group's scale and leaves it alone
            m.dp = SimpleNamespace(active=True, grad_scale=0.5, world=1, allreduce_mean=lambda t: None)
            P = m._plan(2, 32, 32)
            P.set_grad_scale(0.5)
        m.iteration(hr, bic, real)
        torch.cuda.synchronize()
        grads.append([n.params.grad.clone() for n in m.networks()])
    assert P.scale == 0.5 and all(torch.equal(n.params.flat, w) for n, w in zip(m.networks(), w0))
    for k, name in enumerate(('DSN netG', 'DSN netD')):
        _assert_halved('%s (%s)' % (name, norm), *[gr[k] for gr in grads])
