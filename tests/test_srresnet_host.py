"""CPU tests of the SRResNet generator (which_model_G: sr_resnet): parameter layout and init replay against the reference fixtures
(scripts/gen_golden_srresnet.py), option refusals, and the C-ABI mirror of dasr_resblock_params."""
import glob
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', '*srresnet_*.npz')))


def _case(path):
    f = np.load(path)
    return f, json.loads(str(f['case_json']))


def test_fixtures_present():
    names = {os.path.basename(p)[:-4] for p in FIXTURES}
    assert {'srresnet_nf64_nb2_b2_32', 'srresnet_nf64_nb16_b2_32', 'srresnet_nf64_nb2_b1_24x40', 'dasr_srresnet_wavelet_nf64_nb2_n2_32'} <= names


@pytest.mark.parametrize('path', FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_param_spec_matches_reference_keys(path):
    from dasr_amd.srresnet import srresnet_param_spec
    f, c = _case(path)
    spec = srresnet_param_spec(3, 3, c['nf'], c['nb'])
    assert [k for k, _ in spec] == list(f['state_keys'])
    assert len(spec) == len(f['gradG_norm'])   # one gradient tensor per parameter, in the same order


@pytest.mark.parametrize('path', FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_kaiming_init_replays_reference_define_G(path):
    """init_weights(kaiming, scale 0.1) of networks.py:142-143 under torch.manual_seed(0): same weights bit for bit (digests to 1e-12)"""
    from oracle.nets import tensor_digest
    from dasr_amd.init import kaiming_state_dict
    from dasr_amd.srresnet import srresnet_param_spec
    f, c = _case(path)
    torch.manual_seed(0)
    sd = kaiming_state_dict(srresnet_param_spec(3, 3, c['nf'], c['nb']), 0.1)
    got = np.array([tensor_digest(v) for v in sd.values()])
    for k, (v, (_, shape)) in enumerate(zip(sd.values(), srresnet_param_spec(3, 3, c['nf'], c['nb']))):
        assert tuple(v.shape) == tuple(shape)
    np.testing.assert_allclose(got, f['init_digest'], rtol=1e-12, atol=1e-12)


def _opt(**g):
    net = {'which_model_G': 'sr_resnet', 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': 2, 'in_nc': 3, 'out_nc': 3, 'scale': 4}
    net.update(g)
    from dasr_amd import options
    return options.dict_to_nonedict({'is_train': True, 'network_G': net})


@pytest.mark.parametrize('bad, what', [(dict(norm_type='batch'), "norm_type 'batch' is not implemented"), (dict(mode='NAC'), "mode 'NAC' is not implemented"),
                                       (dict(mode='CNAC'), "mode 'CNAC' is not implemented"), (dict(scale=2), 'scale 2 is not implemented'),
                                       (dict(scale=3), 'scale 3 is not implemented')])
def test_define_G_refuses_unsupported_variants(bad, what):
    from dasr_amd.models import _define_G
    with pytest.raises(NotImplementedError, match=what):
        _define_G(_opt(**bad), 'cpu')


def test_define_G_refuses_split_bf16_hr_tail(monkeypatch):
    from dasr_amd.models import _define_G
    monkeypatch.setenv('DASR_HR_PREC', '3')
    with pytest.raises(NotImplementedError, match='DASR_HR_PREC=3 is not implemented'):
        _define_G(_opt(), 'cpu')


def test_resblock_struct_matches_header_layout():
    import ctypes
    from dasr_amd import _lib
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "dasr_hip.h"
int main(){printf("%zu %zu %zu %zu\n", sizeof(dasr_resblock_params), offsetof(dasr_resblock_params, h), offsetof(dasr_resblock_params, N),
 offsetof(dasr_resblock_params, slope)); printf("%d\n", (int)DASR_OP_RESBLOCK); return 0;}'''
    d = tempfile.mkdtemp()
    open(os.path.join(d, 't.c'), 'w').write(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
    vals = [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).split()]
    R = _lib.ResblockParams
    assert vals[:4] == [ctypes.sizeof(R), R.h.offset, R.N.offset, R.slope.offset]
    assert vals[4] == _lib.OP_RESBLOCK


@pytest.mark.parametrize('trunk_prec', [1, 2])
@pytest.mark.parametrize('fused', [None, True, False])
def test_plans_record_on_the_host(trunk_prec, fused):
    """SRResNetHIP and its plans reuse RRDBNetHIP's builders without calling its constructor: recording every plan kind (training, sub-batch
    replicas, inference) on CPU tensors exercises every attribute those builders read.  No kernel runs."""
    from dasr_amd.srresnet import SRResNetHIP
    if fused and trunk_prec == 2:
        with pytest.raises(ValueError, match='f16-storage trunk'):
            SRResNetHIP(nb=2, device='cpu', fused_blocks=True, trunk_prec=2)
        return
    net = SRResNetHIP(nb=2, device='cpu', fused_blocks=fused, trunk_prec=trunk_prec)
    p = net.plan(2, 24, 40)
    st = net.trunk_store(8, 32, 32)
    reps = [net.plan(4, 32, 32, replica=r, store=st, n0=4 * r) for r in (0, 1)]
    assert all(q.store is st for q in reps) and st.calibrate_due() == (trunk_prec == 2)
    inf = net._make_plan(1, 24, 40, inference=True)
    assert p.fused == bool(fused) and inf.fused == (fused is not False and trunk_prec == 1)
    assert p.take_f16_loss_gradient() is not None
    # gradient buckets: contiguous, descending, covering the whole flat buffer
    spans = [s for _, s in p.bwd_segments()]
    assert spans[0][1] == net.params.total and spans[-1][0] == 0
    assert all(a[0] == b[1] for a, b in zip(spans, spans[1:]))
    if trunk_prec == 2:   # a new scale reaches every scaled op and reduction of every plan of the shape
        st.set_gscale_from(3e-6)
        assert st.gscale == 2.0 ** 18 and st._scaled and all(o.conv.gamma == st.gscale for o, _ in st._scaled) and all(o.get('inv_prescale') == 2.0 ** -18 for o in st._reduces)


@pytest.mark.parametrize('model', ['DASR', 'DASR_FS_ESRGAN_patchGAN'])
def test_define_G_refuses_sr_resnet_as_dasr_generator(model):
    """outside the gradient tolerance on the DASR step: refused, not run with a looser bound"""
    from dasr_amd import options
    from dasr_amd.models import _define_G
    opt = _opt()
    opt['model'] = model
    with pytest.raises(NotImplementedError, match='sr_resnet as the generator of model %s is not implemented' % model):
        _define_G(options.dict_to_nonedict(opt), 'cpu')
