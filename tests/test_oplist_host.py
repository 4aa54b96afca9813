"""CPU tests of post-recording patches (engine.patch / OpList): an Op object recorded once sits in several op lists, each with a ctypes image of its own
that dasr_run_ops reads; a patched argument has to reach every one of them.  The plans record on device='cpu'; no kernel runs."""
from types import SimpleNamespace

import pytest
import torch

from dasr_amd import _lib, engine, rrdbnet
from dasr_amd.engine import OpList, ParamStore, PackRegistry, conv_op


def _fresh(ol):
    """the image a list just built from its ops would have"""
    return bytes((_lib.Op * len(ol.ops))(*ol.ops))


def _assert_images_fresh(lists):
    for ol in lists:
        assert bytes(ol._image()) == _fresh(ol)


def _conv():
    P = ParamStore([('w', (32, 16, 3, 3))], 'cpu')
    pack = PackRegistry(P)
    ref = pack.add(32, 16, 9, 1, 1, [(0, 32, 16, 0, 16, 0, 0)])
    pack.finalize()
    return conv_op(pack, ref, _lib.Tensor(0x1000, 64, 16), False, 16, 4, 4, 4, 4, 1, gamma=1.0), (P, pack)


def test_a_patch_reaches_the_image_of_every_list_that_holds_the_op():
    a = OpList()
    a.add(_lib.make_op(_lib.OP_FILL, p=0x1000, n=8, value=1.0))
    a.add(_lib.make_op(_lib.OP_WGRAD_REDUCE, parts_dev=0x2000, nparts=1, grad_flat=0x3000, scale=1.0))
    conv, keep = _conv()
    a.add(conv)
    b = OpList()
    b.add(_lib.make_op(_lib.OP_FILL, p=0x4000, n=4, value=0.0))
    b.extend(a)
    c = b.slice(2)
    assert [len(x.ops) for x in (a, b, c)] == [3, 4, 2] and c.ops[0] is a.ops[1] and c.ops[1] is conv
    before = [bytes(x._image()) for x in (a, b, c)]
    engine.patch(a.ops[1], scale=0.5, inv_prescale=0.25)
    _assert_images_fresh((a, b, c))
    assert all(bytes(x._arr) != old for x, old in zip((a, b, c), before))
    assert [x._arr[i].get('scale') for x, i in ((a, 1), (b, 2), (c, 0))] == [0.5] * 3
    engine.patch(conv, gamma=8.0, alpha=0.125)
    _assert_images_fresh((a, b, c))
    assert [(x._arr[i].conv.gamma, x._arr[i].conv.alpha) for x, i in ((a, 2), (b, 3), (c, 1))] == [(8.0, 0.125)] * 3
    engine.patch(conv, tag=3)   # the time bucket of a conv op is an Op slot, not a conv parameter
    assert c._image()[1].get('tag') == 3
    with pytest.raises(TypeError):
        engine.patch(conv, gama=2.0)
    with pytest.raises(TypeError):
        engine.patch(a.ops[1], gamma=2.0)


def test_oplist_set_patches_its_own_image_in_place():
    ol = OpList()
    ol.add(_lib.make_op(_lib.OP_LPIPS_S2D, mode=1))
    img = ol._image()
    gen = engine._GEN
    ol.set(0, 'mode', 1 | (5 << 4))
    assert ol._image() is img and engine._GEN == gen and img[0].get('mode') == 81 and ol.ops[0].get('mode') == 81
    engine.patch(ol.ops[0], mode=3)   # a later rebuild starts from the op, which OpList.set patched too
    assert ol._image() is not img and ol._arr[0].get('mode') == 3


def test_sequence_changes_rebuild_the_image():
    ol = OpList()
    for v in (1.0, 2.0, 3.0):
        ol.add(_lib.make_op(_lib.OP_FILL, p=0x1000, n=1, value=v))
    assert len(ol._image()) == 3
    assert ol.pop(0).get('value') == 1.0
    assert [o.get('value') for o in ol._image()] == [2.0, 3.0]
    ol.tag(7)
    assert [o.get('tag') for o in ol._image()] == [7, 7]


def _reduces(lists):
    return [o for ol in lists for o in ol.ops if o.op == _lib.OP_WGRAD_REDUCE]


def test_srresnet_scale_patches_reach_every_replica_list():
    """two replica plans on one store: the data-parallel scale reaches every reduction of every list; the calibrated scale reaches every scaled conv and every
    reduction the store registered (the trunk's: the HR tail's reductions undo the plan's own static scale, the stream convs' none)"""
    from dasr_amd.srresnet import SRResNetHIP
    net = SRResNetHIP(nb=2, trunk_prec=2, device='cpu')
    st = net.trunk_store(8, 16, 16)
    plans = [net.plan(4, 16, 16, replica=r, store=st, n0=4 * r) for r in (0, 1)]
    lists = [p.bwd for p in plans] + [seg for p in plans for seg, _ in p.bwd_segments()]
    _assert_images_fresh(lists)
    assert st.set_gscale_from(3e-6) == 2.0 ** 18
    assert [p.set_grad_scale(0.5) for p in plans] == [True, True] and st.set_grad_scale(0.5) is False
    _assert_images_fresh(lists)
    assert all(seg is s2 for p in plans for (seg, _), (s2, _) in zip(p.bwd_segments(), p.bwd_segments()))   # the segments are kept: the sequence did not change
    assert _reduces(lists) and all(o.get('scale') == 0.5 for o in _reduces(lists))
    assert st._scaled and all(o.conv.gamma == 2.0 ** 18 for o, _ in st._scaled)
    in_lists = {id(o) for o in _reduces(lists)}
    assert len(st._reduces) == 2 * 2 * net.nb and all(id(o) in in_lists and o.get('inv_prescale') == 2.0 ** -18 for o in st._reduces)
    assert [p.set_grad_scale(0.5) for p in plans] == [False, False]


def test_rrdbnet_scale_patches_reach_the_phase_and_the_plan():
    nf, nb, N, h, w = 32, 2, 2, 8, 16
    net = rrdbnet.RRDBNetHIP(nf=nf, nb=nb, device='cpu', rdb_prec=2)
    st = rrdbnet.TrunkStore(net, N, h, w)   # (as tests/test_wgrad_host.py builds it, on a real network: the plan below reads its packs)
    plan = rrdbnet._Plan(net, N, h, w)      # owns a store of its own: the phase's ops are spliced into plan.bwd
    shared = rrdbnet._Plan(net, N // 2, h, w, replica=1, store=st, n0=1)
    lists = [st.phase, plan.store.phase, plan.bwd, shared.bwd] + [seg for p in (plan, shared) for seg, _ in p.bwd_segments()]
    _assert_images_fresh(lists)
    for s in (st, plan.store):
        assert s.calibrate_due() and s.set_gscale_from(3e-6 / 0.04) == 2.0 ** 18
    assert plan.set_grad_scale(0.5) and shared.set_grad_scale(0.5) and st.set_grad_scale(0.5)
    assert not plan.store.set_grad_scale(0.5)   # its reductions are the ones in plan.bwd
    _assert_images_fresh(lists)
    assert all(o.get('scale') == 0.5 for o in _reduces(lists))
    for s in (st, plan.store):
        assert len(s._reduces) == len(s.groups) == len(_reduces([s.phase])) and all(o.get('inv_prescale') == 2.0 ** -18 for o in s._reduces)
        assert len(s._scaled) == 1 + 3 * nb   # one plan on either store: its LR_conv data gradient + the last conv of every dense block
        assert all(o.conv.gamma == _lib.c_f32(bg * 2.0 ** 18).value and (o.conv.alpha == 2.0 ** -18) == a for o, (a, bg) in s._scaled)
    assert {id(o) for o in plan.store._reduces} <= {id(o) for o in plan.bwd.ops}
    # a taken loss-gradient conversion changes the sequence: new segments
    segs = plan.bwd_segments()
    n = len(plan.bwd.ops)
    assert plan.take_f16_loss_gradient() is not None and len(plan.bwd.ops) == n - 1 and plan.bwd_segments() is not segs
    _assert_images_fresh([plan.bwd] + [seg for seg, _ in plan.bwd_segments()])


@pytest.mark.parametrize('kind', ['vgg128', 'fsd_bn'])
def test_every_batchnorm_backward_of_a_discriminator_step_writes_dgamma(kind):
    """_StepPlan.d_step / ds_step take their BatchNorm backward ops from bwd_full only, where dgamma is always set: the one rule of
    set_reduce_scale (BatchNorm backward ops WITH a dgamma) patches what set_d_grad_scale used to patch (every BatchNorm backward op)"""
    from dasr_amd import gan_nets
    if kind == 'vgg128':
        net, (N, H, W) = gan_nets.DiscriminatorVGG128HIP(3, device='cpu'), (2, 128, 128)
    else:
        net, (N, H, W) = gan_nets.BatchNormDiscriminatorHIP(3, device='cpu', spec_layers=gan_nets.fsd_spec(3, norm='Batch')), (2, 16, 16)
    d = net.plan(N, H, W)
    step = OpList()
    step.add(_lib.make_op(_lib.OP_BCE, N=1, C=1, H=1, W=1))
    step.extend(d.bwd_full)
    bn = [o for o in step.ops if o.op == _lib.OP_BNORM_BWD]
    assert bn and all(o.get('dgamma') and o.get('dbeta') for o in bn)
    data = d.bwd_data_ops(N // 2)   # the generator's path through the discriminator: no parameter gradients, no scale
    bn_data = [o for o in data.ops if o.op == _lib.OP_BNORM_BWD]
    assert len(bn_data) == len(bn) and not any(o.get('dgamma') for o in bn_data)
    _assert_images_fresh((step, d.bwd_full, data))
    assert engine.set_reduce_scale((step, data), 0.5)
    assert all(o.get('pscale') == 0.5 for o in bn) and all(o.get('pscale') == 1.0 for o in bn_data)
    assert all(o.get('scale') == 0.5 for o in _reduces([step])) and _reduces([step])
    _assert_images_fresh((step, d.bwd_full, data))
    assert not engine.set_reduce_scale((step, data), 0.5)


def test_reduce_scale_compares_in_fp32():
    """1 / 3 is no fp32 number: the stored scale must not read as changed on every step"""
    ol = OpList()
    ol.add(_lib.make_op(_lib.OP_WGRAD_REDUCE, scale=1.0))
    assert engine.set_reduce_scale([ol], 1.0 / 3) and not engine.set_reduce_scale([ol], 1.0 / 3)
