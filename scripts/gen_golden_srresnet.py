"""Reference fixtures of the SRResNet generator (`which_model_G: sr_resnet`, codes/SRN/models/modules/architecture.py:18-48) behind the
reference's SRModel and DASR_Model -> tests/golden/{srresnet,dasr_srresnet}_*.npz.

TEST INFRASTRUCTURE: runs the reference code (oracle.ref_import), so it only works where the reference tree is importable:
    python scripts/gen_golden_srresnet.py [CASE ...]
Each fixture carries its own case description (`case_json`), the taps / gradients / logs / final-weight digests that oracle.gen_golden.collect
records over two steps from seeded weights, and `init_digest`: the reference's define_G under torch.manual_seed(0) (init_weights kaiming,
scale 0.1) before any seeded weights are loaded.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import fixtures, nets, ref_import  # noqa: E402
from oracle.gen_golden import OUT, collect  # noqa: E402

CASES = {
    'srresnet_nf64_nb2_b2_32': dict(kind='sr', nf=64, nb=2, n=2, lr=32),
    'srresnet_nf64_nb16_b2_32': dict(kind='sr', nf=64, nb=16, n=2, lr=32),          # full depth (train_SRResNet.json)
    'srresnet_nf64_nb2_b1_24x40': dict(kind='sr', nf=64, nb=2, n=1, lr=(24, 40)),   # non-square, partial tiles
    'dasr_srresnet_wavelet_nf64_nb2_n2_32': dict(kind='dasr', nf=64, nb=2, n=2, lr=32, fs='wavelet', d_in_nc=9),
}


def make_opt(c):
    """fixtures.make_opt with the generator switched to sr_resnet (networks.py:88-91 reads in_nc, out_nc, nf, nb, scale, norm_type, mode)"""
    opt = fixtures.make_opt(c)
    opt['network_G'].update(which_model_G='sr_resnet', upsample_mode=None)
    return opt


def run(case):
    option, SRModel, DASR_Model, arch, networks = ref_import.import_srn()
    c = CASES[case]
    opt = option.dict_to_nonedict(make_opt(c))
    torch.manual_seed(0)
    init = np.array([nets.tensor_digest(v) for v in networks.define_G(opt).state_dict().values()])
    torch.manual_seed(0)
    m = (SRModel if c['kind'] == 'sr' else DASR_Model)(opt)
    m.netG.load_state_dict(fixtures.seeded_state_dict(m.netG.state_dict(), 1, 0.1))
    netD = None
    if c['kind'] == 'dasr':
        netD = m.netD_target
        netD.load_state_dict(fixtures.seeded_state_dict(netD.state_dict(), 2, 1.0))
        feed = lambda b: m.feed_data(b, True)
    else:
        feed = lambda b: m.feed_data(b)
    fx = collect(c, m.netG, netD, m.update_learning_rate, feed, m.optimize_parameters, m.get_current_log)
    fx['init_digest'] = init
    fx['case_json'] = np.array(json.dumps(c))
    return fx


def main():
    if not ref_import.available():
        sys.exit('reference tree missing; fixtures can only be generated where it is importable')
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    for case in [a for a in sys.argv[1:] if a in CASES] or CASES:
        fx = run(case)
        np.savez_compressed(os.path.join(OUT, case + '.npz'), **fx)
        print(case, 'logs', fx['logs'][0])


if __name__ == '__main__':
    main()
