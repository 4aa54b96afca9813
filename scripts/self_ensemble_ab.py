"""A/B of x8 self-ensemble inference (`"self_ensemble": true`, BaseModel.test_x8) on RRDB_net nf 64 nb 23, in ONE process, same weights and image:

  test      plain test(): one forward (the quadrant inference under `chop`)
  test_x8   dasr_dihedral8, the generator twice at batch 4, dasr_dihedral8_mean
  host_x8   the reference's procedure (codes/SRN/models/SR_model.py:102-140) restated on this project's generator: every transform a device -> numpy -> device round
            trip, eight batch-1 forwards, torch.cat(...).mean(dim=0)

at LR 128 x 128 without `chop` and LR 339 x 510 (a DIV2K validation image at x4) with it.  Wall clock between two device synchronisations; every variant is warmed up at
every shape, then the variants ALTERNATE for --reps rounds; median, min and max are printed.  The forward-plan cache of the generator (RRDBNetHIP.INFER_CACHE = 2 plans) is
raised to 8 for this process: alternating three variants needs five plan keys per image size, and a plan rebuilt inside a timed call would be timed with it (a driver
runs ONE variant over a folder: its two keys fit the cache of 2).  The table goes to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/self_ensemble_ab.py [--reps 5] [--nb 23] [--out profiles/self_ensemble.txt]

Kernel rates: `--kernels MANIFEST.json` only launches the two geometry kernels (--kernel-reps times per shape) and writes what it launched, with the algorithmic bytes
of every launch (1 read + 8 writes of the LR image; 8 reads + 1 write of the SR image), to MANIFEST.json.  Run it under the profiler in a run of its own,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o se -- python scripts/self_ensemble_ab.py --kernels DIR/manifest.json

then `--rates DIR/manifest.json --trace DIR/.../se_kernel_trace.csv` divides the bytes by the kernel times of the trace (launch order = manifest order) and sets the rates
against the 6.3 TB/s a streaming kernel achieves from HBM on this device.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s, streaming kernels on MI355X


def make_model(nb, chop):
    from dasr_amd import options
    from dasr_amd.models import create_model
    opt = {'is_train': False, 'gpu_ids': [0], 'scale': 4, 'chop': chop, 'val_lpips': False, 'model': 'sr',
           'path': {'pretrain_model_G': None},
           'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': nb, 'in_nc': 3, 'out_nc': 3, 'gc': 32, 'scale': 4}}
    m = create_model(options.dict_to_nonedict(opt))
    from dasr_amd.init import kaiming_state_dict
    from dasr_amd.rrdbnet import rrdbnet_param_spec
    torch.manual_seed(0)
    m.netG.load_state_dict(kaiming_state_dict(rrdbnet_param_spec(3, 3, 64, nb, 'upconv'), 0.1))
    m.netG.INFER_CACHE = 8   # (see the module docstring)
    return m


def host_x8(m):
    """SR_model.py:102-140 on m._generate: the transforms through numpy on the host, eight batch-1 forwards, torch.cat(...).mean(dim=0)"""
    def _transform(v, op):
        v2np = v.data.cpu().numpy()
        if op == 'v':
            tfnp = v2np[:, :, :, ::-1].copy()
        elif op == 'h':
            tfnp = v2np[:, :, ::-1, :].copy()
        else:
            tfnp = v2np.transpose((0, 1, 3, 2)).copy()
        return torch.Tensor(tfnp).to(m.device)
    lr_list = [m.var_L]
    for tf in 'v', 'h', 't':
        lr_list.extend([_transform(t, tf) for t in lr_list])
    sr_list = [m._generate(aug) for aug in lr_list]
    for i in range(len(sr_list)):
        if i > 3:
            sr_list[i] = _transform(sr_list[i], 't')
        if i % 4 > 1:
            sr_list[i] = _transform(sr_list[i], 'h')
        if (i % 4) % 2 == 1:
            sr_list[i] = _transform(sr_list[i], 'v')
    m.fake_H = torch.cat(sr_list, dim=0).mean(dim=0, keepdim=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def ab(args):
    lines = ['# scripts/self_ensemble_ab.py --reps %d --nb %d: RRDB_net nf 64 nb %d, %s, torch %s' % (args.reps, args.nb, args.nb, torch.cuda.get_device_name(0), torch.__version__),
             '# wall clock between two device synchronisations, ms; variants warmed up at every shape, then alternated for %d rounds; spread = (max - min) / median' % args.reps]
    for (H, W), chop in (((128, 128), False), ((339, 510), True)):
        m = make_model(args.nb, chop)
        x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(1))
        m.feed_data({'LR': x}, False)
        variants = [('test', m.test), ('test_x8', m.test_x8), ('host_x8', lambda: host_x8(m))]
        outs = {}
        for name, fn in variants:   # warm-up: plans, code objects
            fn()
            fn()
            outs[name] = m.fake_H.detach().double().cpu()
        ts = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                ts[name].append(timed(fn))
        lines.append('LR %d x %d, chop %s (SR %d x %d)' % (H, W, chop, 4 * H, 4 * W))
        for name, _ in variants:
            t = ts[name]
            med = statistics.median(t)
            lines.append('  %-8s median %9.2f  min %9.2f  max %9.2f  spread %5.1f %%   x %.2f of test' % (
                name, med * 1e3, min(t) * 1e3, max(t) * 1e3, 100 * (max(t) - min(t)) / med, med / statistics.median(ts['test'])))
        r = lambda a, b: float((a - b).norm() / b.norm())
        lines.append('  test_x8 vs host_x8: rel %.2e (sequential fp32 sum against torch.mean; same eight SR images up to the batch size they were computed at); '
                     'test_x8 vs test: rel %.2e; host_x8 / test_x8 time: %.2f' % (r(outs['test_x8'], outs['host_x8']), r(outs['test_x8'], outs['test']),
                                                                                statistics.median(ts['host_x8']) / statistics.median(ts['test_x8'])))
        del m
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


def kernels(args):
    """the two geometry kernels alone, for the profiler"""
    from dasr_amd import util
    manifest = []
    dev = torch.device('cuda')
    for H, W in ((128, 128), (339, 510), (1356, 2040)):   # dihedral8 on the two LR sizes of the A/B, and on an image large enough to leave launch latency behind
        x = torch.rand(3, H, W, device=dev)
        for _ in range(args.kernel_reps):
            util.dihedral8(x)
        manifest.append({'kernel': 'dihedral8_kernel', 'H': H, 'W': W, 'reps': args.kernel_reps, 'bytes': 9 * 3 * H * W * 4})
        torch.cuda.synchronize()
    for H, W in ((512, 512), (1356, 2040)):               # dihedral8_mean on the two SR sizes of the A/B
        a, b = torch.rand(4, 3, H, W, device=dev), torch.rand(4, 3, W, H, device=dev)
        for _ in range(args.kernel_reps):
            util.dihedral8_mean(a, b)
        manifest.append({'kernel': 'dihedral8_mean_kernel', 'H': H, 'W': W, 'reps': args.kernel_reps, 'bytes': 9 * 3 * H * W * 4})
        torch.cuda.synchronize()
    with open(args.kernels, 'w') as f:
        json.dump(manifest, f)
    print('launched', json.dumps(manifest))


def rates(args):
    manifest = json.load(open(args.rates))
    rows = list(csv.DictReader(open(args.trace)))
    rows = [r for r in rows if 'dihedral8' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    lines = ['# kernel time: rocprofv3 --kernel-trace (run of its own); bytes: algorithmic, from the shapes (1 read + 8 writes / 8 reads + 1 write of the image); the bound is',
             '# HBM bandwidth (no arithmetic but 7 adds per output sample): share = rate / 6.3 TB/s achievable.  The first launch of every shape is left out (cold caches, code load).']
    k = 0
    for e in manifest:
        grp = rows[k:k + e['reps']]
        k += e['reps']
        assert len(grp) == e['reps'] and all(e['kernel'] in r['Kernel_Name'] for r in grp), 'the trace does not follow the manifest'
        us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in grp][1:]
        med = statistics.median(us)
        rate = e['bytes'] / (med * 1e-6)
        lines.append('%-22s %4d x %-4d  %8.2f MB  median %8.2f us (min %.2f, max %.2f, n %d)  %6.2f TB/s  %5.1f %% of 6.3 TB/s' % (
            e['kernel'], e['H'], e['W'], e['bytes'] / 1e6, med, min(us), max(us), len(us), rate / 1e12, 100 * rate / HBM_ACHIEVABLE))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--nb', type=int, default=23)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels', default=None, metavar='MANIFEST.json')
    ap.add_argument('--kernel-reps', type=int, default=21)
    ap.add_argument('--rates', default=None, metavar='MANIFEST.json')
    ap.add_argument('--trace', default=None, metavar='kernel_trace.csv')
    args = ap.parse_args()
    if args.rates:
        return rates(args)
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: a timing taken anywhere else says nothing about it')
    if args.kernels:
        return kernels(args)
    ab(args)


if __name__ == '__main__':
    main()
