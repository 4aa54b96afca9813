"""A/B of the SRResNet trunk forms: fused residual blocks (dasr_resblock, one launch per block) against two dasr_conv launches per block.

Times, in ONE process and alternating the two forms round by round (device-synchronised wall clock around K steps after W warm-up steps):
  (a) the SRModel step at the shipped training shape, batch 16 of 32 x 32 LR (train_SRResNet.json, HR_size 128)
  (b) the SRModel step at batch 16 of 128 x 128 LR (the shape bench.py uses for RRDBNet)
  (c) the inference forward of one 256 x 256 LR image
and prints one JSON line per (shape, form, round) plus a summary table (median over rounds).  Kernel statistics come from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/srresnet_ab.py --steps 3 --warmup 1 --rounds 1`.

    python scripts/srresnet_ab.py [--shapes a,b,c] [--steps K] [--warmup W] [--rounds R] [--out profiles/srresnet_ab.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = {'a': ('train', 16, 32), 'b': ('train', 16, 128), 'c': ('infer', 1, 256)}


def _model(fused):
    from dasr_amd import options
    from dasr_amd.models import create_model
    opt = {'is_train': True, 'gpu_ids': [0], 'scale': 4, 'chop': False, 'val_lpips': False, 'model': 'sr',
           'path': {'pretrain_model_G': None, 'models': '/tmp', 'training_state': '/tmp'},
           'network_G': {'which_model_G': 'sr_resnet', 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': 16, 'in_nc': 3, 'out_nc': 3, 'scale': 4},
           'train': {'lr_G': 1e-4, 'weight_decay_G': 0, 'lr_scheme': 'MultiStepLR', 'lr_steps': [200000], 'lr_gamma': 0.5, 'pixel_criterion': 'l1',
                     'pixel_weight': 1.0, 'manual_seed': 0}}
    m = create_model(options.dict_to_nonedict(opt))
    m.netG.fused_blocks = fused
    return m


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='a,b,c')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--forms', default='both', choices=('both', 'fused', 'layer'), help='one form only: per-form kernel traces')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    g = torch.Generator().manual_seed(0)
    forms = {'both': (True, False), 'fused': (True,), 'layer': (False,)}[a.forms]
    models = {f: _model(f) for f in forms}
    res = {}
    for sk in a.shapes.split(','):
        kind, N, s = SHAPES[sk]
        x = torch.rand(N, 3, s, s, generator=g).cuda()
        hr = torch.rand(N, 3, 4 * s, 4 * s, generator=g).cuda()
        fns = {}
        for f, m in models.items():
            if kind == 'train':
                m.feed_data({'LR': x, 'HR': hr})
                ctr = [0]

                def step(m=m, ctr=ctr):
                    ctr[0] += 1
                    m.update_learning_rate()
                    m.optimize_parameters(ctr[0])
                fns[f] = step
            else:
                fns[f] = (lambda m=m: m.netG.forward(x))
        for r in range(a.rounds):
            for f in forms:
                ms = _time(fns[f], a.steps, a.warmup if r == 0 else 1)
                res.setdefault((sk, f), []).append(ms)
                print(json.dumps({'shape': sk, 'kind': kind, 'N': N, 'lr': s, 'fused': f, 'round': r, 'ms': round(ms, 4)}), flush=True)
        del x, hr
    if len(forms) == 1:
        return
    lines = ['SRResNet nf 64 nb 16, fused residual blocks (dasr_resblock) vs two dasr_conv launches per block; median over %d alternating rounds of %d '
             'timed steps (%d warm-up), device-synchronised wall clock' % (a.rounds, a.steps, a.warmup),
             '%-6s %-6s %4s %5s %12s %12s %8s' % ('shape', 'kind', 'N', 'LR', 'fused ms', 'per-layer ms', 'ratio')]
    for sk in a.shapes.split(','):
        kind, N, s = SHAPES[sk]
        fu, pl = statistics.median(res[(sk, True)]), statistics.median(res[(sk, False)])
        lines.append('%-6s %-6s %4d %5d %12.3f %12.3f %8.3f' % (sk, kind, N, s, fu, pl, fu / pl))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
