"""A/B of the DSN trainer's data path: whole training iterations of `python -m dasr_amd.dsn_train` on image folders with

  A   the host loader (dsn_data.TrainDeresnetDataset in DataLoader worker processes: PIL decode of two whole files per item, crop, flips, rotation, imresize as two
      dense matmuls, three tensors over PCIe), at --num_workers 6 (the default) and 16 (the CPUs a GPU job may use)
  B   --device_data (dsn_data.DeviceTrainDeresnet: every file decoded once, bytes resident in device memory, a batch = one descriptor upload + three launches)
  C   --dataset synthetic (random crops made on the host, no files): the floor -- the iteration with next to no data work

on a temporary folder of seeded PNGs, 2040 x 1356 for the clean set and 1020 x 678 for the source set (DIV2K-sized images and their x1/2 versions), with
--filter wavelet --batch_size 8 --crop_size 256 --flips --rotations --allow_random_perceptual.  The epoch length is the number of source files; 16 distinct source
images are written and copied to --source_files names so that an epoch is long enough to time.

Every configuration runs dsn_train.main in a fresh child process under its own time limit.  The child stamps the wall clock at the end of every epoch after ONE device
synchronisation (a hook in front of DSNModel.end_epoch), so an epoch's time holds everything a user waits for: iterations, the loader's start-up (worker processes are
started again every epoch), the epoch's logging.  The first --warmup epochs (plan construction, code objects, the allocator) are dropped; reported is the time per
iteration over all timed epochs and the fastest and slowest single epoch.  The configurations run in the order A6 A16 B C, --repeats times over, so that drift of the
machine shows as a spread between the repeats rather than as a difference between configurations.  B also reports its one-off construction time (decode of every file
on --num_workers threads + upload), which no epoch contains.

The table goes to stdout and to --out.  Nothing here is asserted by a test; the gap B - C is the exposed cost of assembling batches.

    python scripts/dsn_data_ab.py [--repeats 2] [--out profiles/dsn_device_data.txt]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COMMON = ['--filter', 'wavelet', '--batch_size', '8', '--crop_size', '256', '--flips', '--rotations', '--allow_random_perceptual', '--no_saving',
          '--val_interval', '100000', '--val_img_interval', '100000', '--save_model_interval', '100000']


def write_png(path, h, w, seed):
    """a photograph-like 8-bit image (smooth field + noise): PNG decode time depends on the content"""
    import torch
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, h // 16 + 2, w // 16 + 2, generator=g), size=(h, w), mode='bilinear', align_corners=False)[0]
    img = (base + 0.03 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(path)


def make_folders(tmp, n_clean, n_source):
    import yaml
    dirs = {k: os.path.join(tmp, k) for k in ('source', 'target', 'valid_hr', 'valid_lr')}
    for d in dirs.values():
        os.makedirs(d)
    for i in range(n_clean):
        write_png(os.path.join(dirs['target'], 'clean_%03d.png' % i), 1356, 2040, 1000 + i)
    distinct = min(16, n_source)
    for i in range(distinct):
        write_png(os.path.join(dirs['source'], 'source_%04d.png' % i), 678, 1020, 2000 + i)
    for i in range(distinct, n_source):
        shutil.copyfile(os.path.join(dirs['source'], 'source_%04d.png' % (i % distinct)), os.path.join(dirs['source'], 'source_%04d.png' % i))
    write_png(os.path.join(dirs['valid_hr'], 'val.png'), 256, 256, 1)      # (the validation pass never runs here; the folders must list a pair)
    write_png(os.path.join(dirs['valid_lr'], 'val.png'), 64, 64, 2)
    paths = os.path.join(tmp, 'paths.yml')
    with open(paths, 'w') as f:
        yaml.safe_dump({'aim2019': {'tdsr': dirs}}, f)
    return paths


def child(argv, epochs):
    """run dsn_train.main(argv + --num_epochs epochs) with the epoch stamps; prints one JSON line"""
    import torch
    from dasr_amd import dsn_data, dsn_model, dsn_train
    stamps, built = [], {}
    end_epoch, make = dsn_model.DSNModel.end_epoch, dsn_data.make_device_datasets

    def stamped_end_epoch(self):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return end_epoch(self)

    def timed_make(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = make(*a, **k)
        torch.cuda.synchronize()
        built.update(seconds=time.perf_counter() - t0, files=len(out[0].noisy) + len(out[0].clean),
                     bytes=sum(t.numel() for t in out[0].noisy + out[0].clean))
        return out
    dsn_model.DSNModel.end_epoch = stamped_end_epoch
    dsn_data.make_device_datasets = timed_make
    t0 = time.perf_counter()
    m = dsn_train.main(argv + ['--num_epochs', str(epochs), '--num_decay_epochs', str(max(1, epochs // 2))])
    print('AB_RESULT ' + json.dumps({'epoch_seconds': [b - a for a, b in zip([t0] + stamps[:-1], stamps)], 'iterations': m.iteration_count, 'built': built,
                                     'device': torch.cuda.get_device_name(0), 'torch': torch.__version__}))


def run_child(argv, epochs, limit):
    cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--child', json.dumps(argv), '--epochs', str(epochs)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = p.stdout.decode(errors='replace')
    rows = [l for l in text.splitlines() if l.startswith('AB_RESULT ')]
    if p.returncode != 0 or not rows:
        sys.stderr.write(text[-4000:])
        raise SystemExit('dsn_data_ab.py: a configuration ended with status %d; nothing more is started on the device' % p.returncode)
    return json.loads(rows[-1][len('AB_RESULT '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--epochs', type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--clean_files', type=int, default=8)
    ap.add_argument('--source_files', type=int, default=256, help='epoch length in items: 256 files are 32 iterations of batch 8')
    ap.add_argument('--warmup', type=int, default=2, help='epochs dropped in front of the timed ones')
    ap.add_argument('--host_epochs', type=int, default=3, help='timed epochs of the host-loader configurations (seconds each)')
    ap.add_argument('--device_epochs', type=int, default=20, help='timed epochs of --device_data and synthetic (a fraction of a second each)')
    ap.add_argument('--limit', type=int, default=420, help='time limit of one configuration, seconds')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dsn_device_data.txt'))
    a = ap.parse_args()
    if a.child is not None:
        return child(json.loads(a.child), a.epochs)
    iters = (a.source_files + 7) // 8
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        paths = make_folders(tmp, a.clean_files, a.source_files)
        t_png = time.perf_counter() - t0
        folder = ['--dataset', 'aim2019', '--artifacts', 'tdsr', '--paths', paths]
        configs = [('A  host loader, --num_workers 6', folder + ['--num_workers', '6'], a.host_epochs),
                   ('A  host loader, --num_workers 16', folder + ['--num_workers', '16'], a.host_epochs),
                   ('B  --device_data (16 decode threads)', folder + ['--num_workers', '16', '--device_data'], a.device_epochs),
                   ('C  --dataset synthetic (floor)', ['--dataset', 'synthetic', '--iters_per_epoch', str(iters)], a.device_epochs)]
        for rep in range(a.repeats):
            for name, argv, timed in configs:
                r = run_child(COMMON + argv, a.warmup + timed, a.limit)
                ep = r['epoch_seconds'][a.warmup:]
                per_epoch_iters = r['iterations'] // (a.warmup + timed)
                results.setdefault(name, []).append(dict(r, ms=1e3 * sum(ep) / (per_epoch_iters * len(ep)), lo=1e3 * min(ep) / per_epoch_iters,
                                                         hi=1e3 * max(ep) / per_epoch_iters, n=per_epoch_iters * len(ep)))
                sys.stderr.write('%s, repeat %d: %.2f ms per iteration\n' % (name, rep + 1, results[name][-1]['ms']))
    first = next(iter(results.values()))[0]
    lines = ['DSN training iterations by data path (scripts/dsn_data_ab.py): dsn_train.main ' + ' '.join(COMMON[:9]),
             'device: %s; host: %d CPUs available to the process, torch %s' % (first['device'], len(os.sched_getaffinity(0)), first['torch']),
             'data: %d clean PNGs of 2040 x 1356, %d source PNGs of 1020 x 678 (16 distinct), written in %.1f s; %d iterations per epoch' % (
                 a.clean_files, a.source_files, t_png, iters),
             'wall clock per epoch between two device synchronisations, %d warm-up epochs dropped; ms per iteration: all timed epochs together [fastest epoch, slowest epoch]' % a.warmup,
             '', '| configuration | ' + ' | '.join('repeat %d' % (k + 1) for k in range(a.repeats)) + ' | timed iterations per repeat |', '|---|' + '---|' * (a.repeats + 1)]
    for name, rs in results.items():
        lines.append('| %s | %s | %d |' % (name, ' | '.join('%.2f [%.2f, %.2f]' % (r['ms'], r['lo'], r['hi']) for r in rs), rs[0]['n']))
    best = {name: min(r['ms'] for r in rs) for name, rs in results.items()}
    names = list(results)
    lines += ['', 'fastest repeat of each: A(6) %.2f, A(16) %.2f, B %.2f, C %.2f ms per iteration' % tuple(best[n] for n in names),
              'A(16) / B = %.1fx; B - C = %+.2f ms per iteration (the exposed cost of assembling a batch on the device; negative: B is the faster of the two)' % (
                  best[names[1]] / best[names[2]], best[names[2]] - best[names[3]]), '']
    for r in results[names[2]]:
        b = r['built']
        lines.append('B, one-off construction (decode of %d files on 16 threads + upload of %.1f MB, train set): %.2f s' % (b['files'], b['bytes'] / 1e6, b['seconds']))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
