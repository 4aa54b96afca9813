"""CPU tests of the three plan recorders: BTensor.view(c0, n0), gan_nets.FreqSplit and _DPlan.norm_op.  The expected argument values are written out as
literals: they are what the trainers recorded at every site before the recorders existed.  Everything records on device='cpu'; no kernel runs."""
import pytest
import torch

from dasr_amd import _lib, gan_nets
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
