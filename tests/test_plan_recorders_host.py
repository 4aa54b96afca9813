"""CPU tests of the four plan recorders: BTensor.view(c0, n0), gan_nets.FreqSplit, _DPlan.norm_op and engine.StorageForm with the one _VGGPlan builder
that consults it.  The expected argument values are written out as literals: they are what the trainers recorded at every site before the recorders
existed.  Everything records on device='cpu'; no kernel runs."""
import pytest
import torch

from dasr_amd import _lib, engine, gan_nets
from dasr_amd._lib import Tensor
from dasr_amd.engine import BTensor, NULL_T
from dasr_amd.gan_nets import FreqSplit

L = _lib


def _t(v):
    return (v.p, v.n_stride, v.cb_stride)


# ---- BTensor.view -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32,f16,esz', [(True, False, 4), (False, False, 2), (False, True, 2)], ids=['f32', 'bf16', 'f16'])
def test_btensor_view_of_images_and_channels_is_the_old_formula(f32, f16, esz):
    N, C_, H, W = 3, 40, 5, 7
    bt = BTensor(N, C_, H, W, f32, 'cpu', f16=f16)
    assert bt.esz == esz and bt.planes == 3
    base, cbs = bt.t.data_ptr(), H * W * 16
    for c0, n0 in ((0, 0), (0, 1), (0, 2), (16, 0), (32, 2)):
        v = bt.view(c0) if n0 == 0 else bt.view(c0, n0)
        old = bt.view(c0)   # the removed helpers: Tensor(v.p + n0 * v.n_stride * bt.esz, v.n_stride, v.cb_stride)
        assert _t(v) == (old.p + n0 * old.n_stride * esz, 3 * cbs, cbs)
        assert v.p == base + ((c0 // 16) * cbs + n0 * 3 * cbs) * esz
        assert v.p == bt.t[n0, c0 // 16].data_ptr()
    assert _t(bt.view(n0=1)) == _t(bt.view(0, 1))
    for bad in (N, -1):
        with pytest.raises(AssertionError):
            bt.view(n0=bad)


def test_btensor_view_of_a_split_tensor_is_its_hi_planes():
    bt = BTensor(2, 2 * 64, 4, 4, False, 'cpu', f16=True)   # planes [0, 4) hi, [4, 8) remainders
    v = bt.view(n0=1)
    assert v.p == bt.t[1, 0].data_ptr() and v.n_stride == 8 * 4 * 4 * 16 and v.cb_stride == 4 * 4 * 16


# ---- FreqSplit ----------------------------------------------------------------------------------------------------
X, LOW, HIGH, DST, G1, G2 = (Tensor(0x1000 * (i + 1), 64 * 16, 16) for i in range(6))
N, H, W = 2, 12, 20


def _args(op, names):
    return {n: (_t(op.get(n)) if _lib.OP_ARGS[op.op][n].startswith('t') else op.get(n)) for n in names}


def _null(op, *names):
    return all(op.get(n).p is None for n in names)


# name -> (object, wavelet?, k, in_nc, forward mode, a_h, b_h, dwt norm)
def _cases():
    return {
        'dsn_gau': (FreqSplit.dsn('gau', 5, 'cat', 'cpu'), False, 5, 3, 0, 0.5, 0.5, None),
        'dsn_gau_sum': (FreqSplit.dsn('gau', 5, 'sum', 'cpu'), False, 5, 3, 0, 0.5, 0.5, None),
        'dsn_avg_pool': (FreqSplit.dsn('avg_pool', 5, 'cat', 'cpu'), False, 5, 3, 2, 0.5, 0.5, None),
        'dsn_wavelet_cat': (FreqSplit.dsn('wavelet', 5, 'cat', 'cpu'), True, 5, 9, None, None, None, 1),
        'dsn_wavelet_sum': (FreqSplit.dsn('wavelet', 5, 'sum', 'cpu'), True, 5, 3, None, None, None, 3),
        'srn_wavelet': (FreqSplit.srn('wavelet', 9, False, 'cpu'), True, 9, 9, None, None, None, 0),
        'srn_wavelet_norm': (FreqSplit.srn('wavelet', 9, True, 'cpu'), True, 9, 9, None, None, None, 1),
        'srn_gau': (FreqSplit.srn('gau', 9, False, 'cpu'), False, 9, 3, 0, 0.5, 0.5, None),
        'srn_gau_norm': (FreqSplit.srn('gau', 9, True, 'cpu'), False, 9, 3, 0, 0.25, 0.75, None),
        'srn_avgpool': (FreqSplit.srn('avgpool', 9, False, 'cpu'), False, 9, 3, 0, 0.5, 0.5, None),     # count_include_pad=True: no valid bit
        'srn_avgpool_norm': (FreqSplit.srn('avgpool', 9, True, 'cpu'), False, 9, 3, 0, 0.25, 0.75, None),
    }


CASES = sorted(_cases())


@pytest.mark.parametrize('case', CASES)
def test_freqsplit_owns_weights_sizes_and_channel_count(case):
    fs, wavelet, k, in_nc, _, _, _, norm = _cases()[case]
    assert (fs.wavelet, fs.k, fs.in_nc) == (wavelet, k, in_nc)
    assert fs.out_size(H, W) == ((6, 10) if wavelet else (12, 20))
    assert fs.colour_size(H, W) == ((6, 10) if wavelet else (12 - k + 1, 20 - k + 1))
    assert fs.w.shape == (k, k) and fs.w.dtype == torch.float32 and fs.w.is_contiguous() and abs(float(fs.w.sum()) - 1.0) < 1e-6
    box = 'avg' in case
    assert bool(torch.all(fs.w == fs.w[0, 0])) == box   # the box average, else the gaussian (a wavelet model: the gaussian of its image views)
    if wavelet:
        assert fs.dwt_norm == norm


@pytest.mark.parametrize('case', CASES)
def test_freqsplit_split_records_what_the_plans_recorded(case):
    fs, wavelet, k, _, mode, a_h, b_h, norm = _cases()[case]
    assert fs.split(X, N, H, W) == [] and fs.split(X, N, H, W, low=NULL_T, high=NULL_T) == []
    for low, high in ((LOW, HIGH), (None, HIGH), (LOW, NULL_T)):
        ops = fs.split(X, N, H, W, low=low, high=high)
        assert len(ops) == 1
        o = ops[0]
        if wavelet:
            assert o.op == L.OP_DWT_FWD
            assert _args(o, ['x', 'N', 'C', 'H2', 'W2', 'norm']) == dict(x=_t(X), N=2, C=3, H2=6, W2=10, norm=norm)
            lo_name, hi_name = 'll', 'hc'
        else:
            assert o.op == L.OP_LOWPASS
            assert _args(o, ['x', 'w', 'k', 'N', 'C', 'H', 'W', 'mode', 'a_h', 'b_h', 'accumulate']) == dict(
                x=_t(X), w=fs.w.data_ptr(), k=k, N=2, C=3, H=12, W=20, mode=mode, a_h=a_h, b_h=b_h, accumulate=0)
            assert _null(o, 'x2')
            lo_name, hi_name = 'out_low', 'out_high'
        assert _t(o.get(lo_name)) == (_t(low) if low is LOW else (None, 0, 0))
        assert _t(o.get(hi_name)) == (_t(high) if high is HIGH else (None, 0, 0))


@pytest.mark.parametrize('case', CASES)
def test_freqsplit_tangent_and_colour(case):
    fs, wavelet, k, _, mode, a_h, _, norm = _cases()[case]
    (t,), (c,) = fs.tangent(X, N, H, W, HIGH), fs.colour(X, N, H, W, LOW)
    if wavelet:
        assert (t.op, c.op) == (L.OP_DWT_FWD, L.OP_DWT_FWD)
        assert _args(t, ['x', 'N', 'C', 'H2', 'W2', 'norm', 'hc']) == dict(x=_t(X), N=2, C=3, H2=6, W2=10, norm=norm | 4, hc=_t(HIGH)) and _null(t, 'll')
        assert _args(c, ['x', 'N', 'C', 'H2', 'W2', 'norm', 'll']) == dict(x=_t(X), N=2, C=3, H2=6, W2=10, norm=1, ll=_t(LOW)) and _null(c, 'hc')
    else:
        assert (t.op, c.op) == (L.OP_LOWPASS, L.OP_LOWPASS_VALID)
        assert _args(t, ['x', 'w', 'k', 'N', 'C', 'H', 'W', 'mode', 'a_h', 'b_h', 'out_high', 'accumulate']) == dict(
            x=_t(X), w=fs.w.data_ptr(), k=k, N=2, C=3, H=12, W=20, mode=mode, a_h=a_h, b_h=0.0, out_high=_t(HIGH), accumulate=0)
        assert _null(t, 'x2', 'out_low')
        assert _args(c, ['x', 'w', 'k', 'N', 'C', 'H', 'W', 'mode', 'out', 'accumulate']) == dict(
            x=_t(X), w=fs.w.data_ptr(), k=k, N=2, C=3, H=12, W=20, mode=0, out=_t(LOW), accumulate=0)


@pytest.mark.parametrize('case', CASES)
def test_freqsplit_adjoint_takes_the_gradients_together(case):
    fs, wavelet, k, _, mode, a_h, _, norm = _cases()[case]
    assert fs.adjoint(DST, N, H, W) == [] and fs.adjoint(DST, N, H, W, g_low=NULL_T, g_high=NULL_T) == []
    with pytest.raises(AssertionError):
        fs.adjoint(DST, N, H, W, g_low=G1, g_colour=G2)
    # the SRN generator-loss backward (low + high, high alone), the gradient penalty (high alone), the DSN generator backward (high + colour)
    for kw in (dict(g_low=G1, g_high=G2), dict(g_low=NULL_T, g_high=G2), dict(g_high=G2), dict(g_high=G2, g_colour=G1), dict(g_colour=G1)):
        ops = fs.adjoint(DST, N, H, W, **kw)
        low = kw.get('g_low') if kw.get('g_low') is G1 else None
        col = kw.get('g_colour')
        if wavelet:   # ONE op: the colour gradient rides in gll
            assert len(ops) == 1 and ops[0].op == L.OP_DWT_BWD
            gll = low or col
            assert _args(ops[0], ['gll', 'ghc', 'N', 'C', 'H2', 'W2', 'norm', 'gx', 'accumulate']) == dict(
                gll=_t(gll) if gll is not None else (None, 0, 0), ghc=_t(G2) if 'g_high' in kw else (None, 0, 0), N=2, C=3, H2=6, W2=10, norm=norm,
                gx=_t(DST), accumulate=1)
            continue
        bands = [o for o in ops if o.op == L.OP_LOWPASS]
        valid = [o for o in ops if o.op == L.OP_LOWPASS_VALID]
        assert len(bands) == (1 if (low is not None or 'g_high' in kw) else 0) and len(valid) == (1 if col is not None else 0)
        assert ops == bands + valid   # the order of the DSN generator backward: the front end's adjoint, then the colour filter's
        for o in bands:
            assert _args(o, ['x', 'x2', 'w', 'k', 'N', 'C', 'H', 'W', 'mode', 'a_h', 'b_h', 'out_low', 'accumulate']) == dict(
                x=_t(low) if low is not None else (None, 0, 0), x2=_t(G2), w=fs.w.data_ptr(), k=k, N=2, C=3, H=12, W=20, mode=1 | mode, a_h=a_h,
                b_h=0.0, out_low=_t(DST), accumulate=1)
            assert _null(o, 'out_high')
        for o in valid:
            assert _args(o, ['x', 'w', 'k', 'N', 'C', 'H', 'W', 'mode', 'out', 'accumulate']) == dict(
                x=_t(G1), w=fs.w.data_ptr(), k=k, N=2, C=3, H=12, W=20, mode=1, out=_t(DST), accumulate=1)
    ca, = fs.colour_adjoint(G1, DST, N, H, W)
    assert bytes(ca) == bytes(fs.adjoint(DST, N, H, W, g_colour=G1)[0])


def test_freqsplit_rejects_unknown_options():
    for bad in (lambda: FreqSplit.srn('avg_pool', 9, False, 'cpu'), lambda: FreqSplit.dsn('avgpool', 5, 'cat', 'cpu'),
                lambda: FreqSplit.dsn('wavelet', 5, 'both', 'cpu'), lambda: FreqSplit.srn(None, 9, False, 'cpu')):
        with pytest.raises(NotImplementedError):
            bad()


# ---- _DPlan.norm_op -----------------------------------------------------------------------------------------------
def _dplan(norm):
    cls = gan_nets.BatchNormDiscriminatorHIP if norm == 'Batch' else gan_nets.NLayerDiscriminatorHIP
    net = cls(3, device='cpu', spec_layers=gan_nets.fsd_spec(3, norm=norm))
    return net, net.plan(2, 16, 16)


@pytest.mark.parametrize('norm', ['Instance', 'Batch'])
def test_norm_op_chooses_kind_and_arguments_per_pass(norm):
    net, d = _dplan(norm)
    batch, P = norm == 'Batch', net.params
    i = 1                                     # fsd: layers 1 and 2 carry the norm (64 -> 128 channels, 5 x 5, stride 1)
    Lr = net.layers[i]
    assert Lr['norm'] == ('batch' if batch else True) and d.dims[i + 1] == (16, 16) and d.group == (1 if batch else 2)
    t, out, ga, gx = (Tensor(0x1000 * (j + 1), 128 * 256, 256) for j in range(4))
    common = dict(N=2, C=128, H=16, W=16, slope=_lib.c_f32(0.2).value, stats=d.stats[i].data_ptr())
    bn = dict(group=1, gamma=P.ptr(Lr['bn'] + 'weight'), beta=P.ptr(Lr['bn'] + 'bias')) if batch else {}
    src = {'x': _t(d.zs[i].view())} if batch else {'a': _t(d.acts[i].view())}   # BatchNorm reads the conv output, InstanceNorm the saved activation
    dg, db = 0x7000, 0x7100

    def check(o, kind, want):
        assert o.op == kind
        names = list(want)
        assert _args(o, names) == want, (_args(o, names), want)
        assert set(_lib.OP_ARGS[kind]) == set(names)   # every argument of the op is pinned

    o = d.norm_op(i, 'fwd', 2)
    check(o, L.OP_BNORM_FWD if batch else L.OP_INORM_FWD,
          dict(common, x=_t(d.zs[i].view()), y=_t(d.acts[i].view()), eps=_lib.c_f32(1e-5).value, **bn))
    o = d.norm_op(i, 'bwd', 2, ga=ga, gx=gx, dgamma=dg, dbeta=db)
    check(o, L.OP_BNORM_BWD if batch else L.OP_INORM_BWD,
          dict(common, ga=_t(ga), gx=_t(gx), **src, **(dict(bn, dgamma=dg, dbeta=db, pscale=1.0) if batch else {})))
    o = d.norm_op(i, 'bwd', 1, ga=ga, gx=gx)   # the generator's path: a prefix of the batch, no parameter gradients
    check(o, L.OP_BNORM_BWD if batch else L.OP_INORM_BWD,
          dict(common, N=1, ga=_t(ga), gx=_t(gx), **src, **(dict(bn, dgamma=None, dbeta=0, pscale=1.0) if batch else {})))
    o = d.norm_op(i, 'jvp', 2, t=t, out=out)
    check(o, L.OP_BNORM_JVP if batch else L.OP_INORM_JVP, dict(common, t=_t(t), out=_t(out), **src, **bn))
    o = d.norm_op(i, 'second', 2, t=t, ga=ga, out=out, accumulate=1, dgamma=dg)
    check(o, L.OP_BNORM_SECOND if batch else L.OP_INORM_SECOND,
          dict(common, t=_t(t), ga=_t(ga), out=_t(out), accumulate=1, **src, **(dict(bn, dgamma=dg, pscale=1.0) if batch else {})))


@pytest.mark.parametrize('norm', ['Instance', 'Batch'])
def test_discriminator_plans_record_their_norm_ops_through_the_recorder(norm):
    net, d = _dplan(norm)
    batch, P = norm == 'Batch', net.params
    kf, kb = (L.OP_BNORM_FWD, L.OP_BNORM_BWD) if batch else (L.OP_INORM_FWD, L.OP_INORM_BWD)
    fwd = [o for o in d.fwd.ops if o.op == kf]
    assert len(fwd) == 2
    for o, i in zip(fwd, (1, 2)):
        assert (o.get('N'), o.get('stats'), _t(o.get('x')), _t(o.get('y'))) == (2, d.stats[i].data_ptr(), _t(d.zs[i].view()), _t(d.acts[i].view()))
    for ol, n, wgrad in ((d.bwd_full, 2, True), (d.bwd_data_ops(1), 1, False)):
        bwd = [o for o in ol.ops if o.op == kb]
        assert len(bwd) == 2
        for o, i in zip(bwd, (2, 1)):   # the backward walks the layers from the top
            bn = net.layers[i].get('bn')
            assert (o.get('N'), o.get('stats'), _t(o.get('ga')), _t(o.get('gx'))) == (n, d.stats[i].data_ptr(), _t(d.ga[i].view()), _t(d.gz[i].view()))
            if batch:
                want = (P.ptr(bn + 'weight', P.grad), P.ptr(bn + 'bias', P.grad)) if wgrad else (None, 0)
                assert (o.get('dgamma'), o.get('dbeta'), o.get('pscale')) == want + (1.0,)


# ---- engine.StorageForm -------------------------------------------------------------------------------------------
# form -> per C in (3, 64, 512): planes of alloc, (in_f32, cin, in_wrap), out16_lo, res1_lo; then dtype, OP_CVT_F16 form, affine / pool code
FORMS = {
    'F32': ([(1, (True, 16, 0), None, 0), (4, (True, 64, 0), None, 0), (32, (True, 512, 0), None, 0)], torch.float32, 0, 1),
    'F16': ([(1, (False, 16, 0), 0, 0), (4, (False, 64, 0), 0, 0), (32, (False, 512, 0), 0, 0)], torch.float16, 0, 2),
    'SPLIT': ([(2, (False, 48, 2), 1, 1), (8, (False, 192, 8), 4, 4), (64, (False, 1536, 64), 32, 32)], torch.float16, 1, 3),
}


@pytest.mark.parametrize('name', sorted(FORMS))
def test_storage_form_answers_what_the_builders_wrote_out(name):
    form = getattr(engine, name)
    rows, dtype, cvt, code = FORMS[name]
    assert (form.cvt_form, form.code) == (cvt, code)
    for C_, (planes, inp, out_lo, res_lo) in zip((3, 64, 512), rows):
        t = form.alloc(3, C_, 4, 6, 'cpu')
        assert tuple(t.t.shape) == (3, planes, 4, 6, 16) and t.t.dtype == dtype and t.f32 == (name == 'F32') and not bool(t.t.any())
        a = form.conv_in(t, C_, 2)
        assert sorted(a) == ['cin', 'in_f32', 'in_wrap', 'inp'] and _t(a['inp']) == _t(t.view(n0=2)) and _t(form.conv_in(t, C_)['inp']) == _t(t.view())
        assert (a['in_f32'], a['cin'], a['in_wrap']) == inp
        o = form.conv_out(t, C_, 1)
        if name == 'F32':
            assert sorted(o) == ['out_f32'] and _t(o['out_f32']) == _t(t.view(n0=1))
        else:
            assert sorted(o) == ['out16_f16', 'out16_lo', 'out_bf16'] and _t(o['out_bf16']) == _t(t.view(n0=1))
            assert (o['out16_f16'], o['out16_lo']) == (1, out_lo)
        r = form.conv_res(t, C_)
        assert sorted(r) == ['res1', 'res1_lo'] and _t(r['res1']) == _t(t.view()) and r['res1_lo'] == res_lo


def test_storage_form_backward_pool_codes():
    F32, F16, SPLIT = engine.F32, engine.F16, engine.SPLIT
    assert (F32.pool_bwd(F32), F16.pool_bwd(F16), SPLIT.pool_bwd(SPLIT), SPLIT.pool_bwd(F16)) == (1, 2, 3, 5)
    for act, grad in ((F32, F16), (F16, SPLIT), (F16, F32)):   # combinations no kernel has
        with pytest.raises(KeyError):
            act.pool_bwd(grad)


@pytest.mark.parametrize('count', [1, 7, 8, 2 ** 20 - 1, 2 ** 20, 3 * 2 ** 31])
def test_grad_prescale_is_the_written_out_formula(count):
    import math
    want = float(2.0 ** max(0, int(math.floor(math.log2(max(1, count)))) - 3))
    assert engine.grad_prescale(count) == want
    assert engine.grad_prescale(0) == 1.0


# ---- _VGGPlan -----------------------------------------------------------------------------------------------------
def _reachable_tensors(*roots):
    """[(first byte, end)] of the storage of every torch tensor reachable from `roots` through dasr_amd objects, lists, tuples and dicts"""
    spans, seen, stack = [], set(), list(roots)
    while stack:
        o = stack.pop()
        if id(o) in seen:
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            st = o.untyped_storage()
            spans.append((st.data_ptr(), st.data_ptr() + st.nbytes()))
        elif isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple)):
            stack.extend(o)
        elif type(o).__module__.startswith('dasr_amd.') and hasattr(o, '__dict__'):
            stack.extend(vars(o).values())
    return spans


def _pointers(o):
    """every non-null address op `o` holds"""
    import ctypes as C
    if o.op == L.OP_CONV:
        vals = [getattr(o.conv, n) for n, typ in _lib.ConvParams._fields_ if typ in (Tensor, C.c_void_p)]
    else:
        vals = list(o.t) + list(o.p)
    return [p for p in (v.p if isinstance(v, Tensor) else v for v in vals) if p]


# (prec, bwd_prec) -> (x_flag, the no-gradient images get a launch of their own, a conversion opens the backward)
VGG_PRECS = {(5, 2): (3, True, True), (5, 5): (3, True, True), (4, None): (1, True, False), (3, None): (1, True, False),
             (2, None): (2, False, True), (1, None): (1, False, False)}


@pytest.mark.parametrize('prec,bwd_prec', sorted(VGG_PRECS, key=str))
def test_vgg_plan_is_one_builder_in_every_precision(prec, bwd_prec, monkeypatch):
    monkeypatch.delenv('DASR_VGG_NOGRAD_PREC', raising=False)
    x_flag, one_pass, cvt = VGG_PRECS[(prec, bwd_prec)]
    V = gan_nets.VGGFeatureHIP(3, device='cpu', cfg=[16, 'M', 32], prec=prec, bwd_prec=bwd_prec)   # conv+ReLU, pool, conv: the pool runs in the activation form
    assert [l[0] for l in V.layers] == ['conv', 'pool', 'conv']
    P = V.plan(2, 1, 8, 8)
    assert not [n for n in dir(P) if n.startswith('_init_')]
    assert P.x_flag == x_flag and hasattr(P, 'gscale') == cvt
    conv = [L.OP_CONV] * (2 if one_pass else 1)
    assert [o.op for o in P.fwd.ops] == conv + [L.OP_MAXPOOL] + conv
    assert [o.op for o in P.bwd.ops] == ([L.OP_CVT_F16] if cvt else []) + [L.OP_CONV, L.OP_MAXPOOL_BWD, L.OP_CONV]
    assert [o.get('tag') for o in P.fwd.ops] == ([6, 7 if prec == 5 else 6, 6, 6, 7 if prec == 5 else 6] if one_pass else [6, 6, 6])
    assert (P.feat.f32, P.g_feat.f32, P.gx.f32) == (True, True, True) and tuple(P.feat.t.shape) == (2, 2, 4, 4, 16) and P.feat is P.outs[-1]
    spans = _reachable_tensors(P, V)
    acts = _reachable_tensors(P.x, P.outs, P.g_feat, P.gx, P._keep)   # the tensors the plan itself keeps: everything but weights and biases
    for ol in (P.fwd, P.bwd):
        for o in ol.ops:
            ptrs = _pointers(o)
            assert len(ptrs) >= 2
            for p in ptrs:
                assert any(a <= p < b for a, b in spans), (o.op, hex(p))
            own = [o.conv.inp.p, o.conv.out_f32.p or o.conv.out_bf16.p] if o.op == L.OP_CONV else [t.p for t in o.t if t.p]
            for p in own:
                assert any(a <= p < b for a, b in acts), (o.op, hex(p))
    kind = L.OP_AXPBY if x_flag == 1 else L.OP_CVT_F16
    c = P.input_copy_op(X, 1, 1, 8, 8)
    assert c.op == kind and _t(c.get('out_f32' if x_flag == 1 else 'y')) == _t(P.x.view(n0=1))
    if x_flag != 1:
        assert c.get('form') == int(prec == 5)
