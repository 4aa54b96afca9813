"""A/B of the SRN trainers' training input stage: the fp32 store of data.DeviceUnpairedDataset / DevicePairedDataset against `"resident_u8": true`, in the SAME
process, on folders of seeded PNGs the script writes itself.

  unpaired   LRHR_wavelet_unpair_fake_weights_EQ, batch 8, HR_size 128 (the shipped shape), model DASR (RRDB_net nf 64 nb 23, wavelet)
  paired     LRHR with LR files, batch 8, HR_size 192, model sr (RRDB_net nf 64 nb 23)
  paired-fly LRHR without dataroot_LR (the LR images are made from the HR images), same shape and model

Per configuration, for either store: the construction time (decode + upload + -- fp32 store without LR files -- imresize_matlab of every whole image on the host),
the bytes resident in device memory, the time per assembled batch (--batches batches between two device synchronisations, --repeats times, the two stores alternating,
the fastest repeat) and the time per whole training iteration (batch + feed_data + optimize_parameters, one model per configuration shared by both stores, same protocol).
Every configuration runs in a fresh child process under its own time limit; after a child that fails nothing more is started.

The table goes to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/srn_data_ab.py [--files 16] [--out profiles/srn_device_data.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = ('unpaired', 'paired', 'paired-fly')


def write_png(path, h, w, seed):
    """a photograph-like 8-bit image (smooth field + noise): PNG decode time depends on the content"""
    import torch
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, h // 16 + 2, w // 16 + 2, generator=g), size=(h, w), mode='bilinear', align_corners=False)[0]
    img = (base + 0.03 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(path)


def make_folders(tmp, files, H, W):
    import numpy as np
    dirs = {k: os.path.join(tmp, k) for k in ('HR', 'LR', 'real_LR', 'ddm')}
    for d in dirs.values():
        os.makedirs(d)
    for i in range(files):
        write_png(os.path.join(dirs['HR'], 'img_%04d.png' % i), H, W, 1000 + i)
        write_png(os.path.join(dirs['LR'], 'img_%04d.png' % i), H // 4, W // 4, 2000 + i)
        write_png(os.path.join(dirs['real_LR'], 'img_%04d.png' % i), H // 4, W // 4, 3000 + i)
        np.save(os.path.join(dirs['ddm'], 'img_%04d.npy' % i), np.random.RandomState(i).rand(1, H // 32, W // 32).astype(np.float32))
    return dirs


def child(config, dirs, a):
    import random
    import numpy as np
    import torch
    import bench
    from dasr_amd import options
    from dasr_amd.data import DevicePairedDataset, DeviceUnpairedDataset
    from dasr_amd.models import create_model
    ds_opt = {'name': config, 'phase': 'train', 'batch_size': 8, 'use_flip': True, 'use_rot': True, 'use_shuffle': True, 'n_workers': 16, 'dataroot_HR': dirs['HR']}
    if config == 'unpaired':
        ds_opt.update(mode='LRHR_wavelet_unpair_fake_weights_EQ', HR_size=128, dataroot_fake_LR=dirs['LR'], dataroot_real_LR=dirs['real_LR'],
                      dataroot_fake_weights=dirs['ddm'])
        cls, opt = DeviceUnpairedDataset, bench.make_dasr_opt(64, 23, 'wavelet')
    else:
        ds_opt.update(mode='LRHR', HR_size=192, dataroot_LR=dirs['LR'] if config == 'paired' else None)
        cls, opt = DevicePairedDataset, bench.make_opt(64, 23)
    sets, built = {}, {}
    for name, key in (('fp32', False), ('u8', True)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sets[name] = cls(dict(ds_opt, resident_u8=key), 4)
        torch.cuda.synchronize()
        built[name] = {'seconds': time.perf_counter() - t0, 'bytes': sum(t.numel() * t.element_size() for v in sets[name].img.values() if v is not None for t in v)}
    model = create_model(options.dict_to_nonedict(opt))
    step = [0]

    def batches(ds, n):
        k = 0
        while True:
            for b in ds:
                yield b
                k += 1
                if k == n:
                    return

    def assemble(ds, n):
        for _ in batches(ds, n):
            pass

    def train(ds, n):
        for b in batches(ds, n):
            step[0] += 1
            model.update_learning_rate()
            model.feed_data(b, True)
            model.optimize_parameters(step[0])

    res = {}
    for what, fn, n in (('batch_ms', assemble, a.batches), ('iteration_ms', train, a.iterations)):
        times = {'fp32': [], 'u8': []}
        for rep in range(a.repeats + 1):          # (the first round is the warm-up: code objects, plans, the allocator)
            for name in ('fp32', 'u8'):
                random.seed(rep)
                np.random.seed(rep)
                torch.manual_seed(rep)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(sets[name], n)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(1e3 * (time.perf_counter() - t0) / n)
        res[what] = times
    print('AB_RESULT ' + json.dumps({'config': config, 'built': built, 'times': res, 'files': len(sets['u8'].img['HR']), 'device': torch.cuda.get_device_name(0),
                                     'torch': torch.__version__}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--dirs', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--files', type=int, default=16, help='HR files (and as many LR, real-LR and domain-distance files)')
    ap.add_argument('--height', type=int, default=1356)
    ap.add_argument('--width', type=int, default=2040)
    ap.add_argument('--batches', type=int, default=200, help='assembled batches per timed window')
    ap.add_argument('--iterations', type=int, default=30, help='training iterations per timed window')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--limit', type=int, default=300, help='time limit of one configuration, seconds')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'srn_device_data.txt'))
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, json.loads(a.dirs), a)
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        dirs = make_folders(tmp, a.files, a.height - a.height % 32, a.width - a.width % 32)
        t_png = time.perf_counter() - t0
        for config in CONFIGS:
            cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--child', config, '--dirs', json.dumps(dirs), '--batches', str(a.batches),
                   '--iterations', str(a.iterations), '--repeats', str(a.repeats)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            text = p.stdout.decode(errors='replace')
            rows = [l for l in text.splitlines() if l.startswith('AB_RESULT ')]
            if p.returncode != 0 or not rows:
                sys.stderr.write(text[-4000:])
                raise SystemExit('srn_data_ab.py: configuration %s ended with status %d; nothing more is started on the device' % (config, p.returncode))
            results.append(json.loads(rows[-1][len('AB_RESULT '):]))
            sys.stderr.write('%s done\n' % config)
    H, W = a.height - a.height % 32, a.width - a.width % 32
    lines = ['SRN training input stage by store (scripts/srn_data_ab.py): fp32 store against "resident_u8": true, same process, stores alternating',
             'device: %s; host: %d CPUs available to the process, torch %s' % (results[0]['device'], len(os.sched_getaffinity(0)), results[0]['torch']),
             'data: %d HR PNGs of %d x %d, as many LR / real-LR PNGs of %d x %d and domain-distance maps, written in %.1f s; batch 8, flips and rotation on' % (
                 a.files, W, H, W // 4, H // 4, t_png),
             'ms: wall clock between two device synchronisations over %d batches / %d iterations, fastest of %d repeats [slowest] after one warm-up round' % (
                 a.batches, a.iterations, a.repeats), '',
             '| configuration | store | construction s | resident MB | ms per assembled batch | ms per training iteration |', '|---|---|---|---|---|---|']
    for r in results:
        for name in ('fp32', 'u8'):
            b, i = r['times']['batch_ms'][name], r['times']['iteration_ms'][name]
            lines.append('| %s | %s | %.2f | %.1f | %.3f [%.3f] | %.2f [%.2f] |' % (r['config'], name, r['built'][name]['seconds'], r['built'][name]['bytes'] / 1e6,
                                                                                  min(b), max(b), min(i), max(i)))
    lines.append('')
    for r in results:
        b, i = r['times']['batch_ms'], r['times']['iteration_ms']
        lines.append('%s: batch fp32 / u8 = %.2fx, iteration fp32 - u8 = %+.2f ms, resident bytes fp32 / u8 = %.2fx, construction fp32 / u8 = %.2fx' % (
            r['config'], min(b['fp32']) / min(b['u8']), min(i['fp32']) - min(i['u8']), r['built']['fp32']['bytes'] / r['built']['u8']['bytes'],
            r['built']['fp32']['seconds'] / r['built']['u8']['seconds']))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
