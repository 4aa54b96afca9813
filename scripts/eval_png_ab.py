"""A/B of the option key `"device_png": true` (SR images encoded by csrc/png.hip through png.FileWriter) against the default path (png.save_host on the main thread: PIL, compress_level 6,
on the main thread) in the drivers that write SR images, in ONE process, the two variants alternating:

  1. `python -m dasr_amd.test` (test.main) on a folder of --pairs LR/HR PNG pairs, RRDB_net nf 64 nb 23, `chop`, `device_metrics: true`, at every --sizes entry
     (LR h x w, SR 4h x 4w): wall ms per image of the pass over the dataset (test.evaluate: the loader's decode and upload, inference, scores, save, and the wait for
     the writer at the end), the split into inference / scores / save (each closed by a device synchronisation, which an ordinary run does not do) and the bytes per file;
  2. one train.validate pass over the first size, both ways;
  3. `python -m dasr_amd.back_projection` over the same folder (the HR files as the SR images), with and without --device_png;
  4. the bytes and the time of one 512 x 512 file by content (flat, a ramp, png.photo, uniform noise): PIL level 6 in memory against png.encode_batch(fmt='bgr').  The
     device files carry no LZ77 matches, so content that repeats is where they are larger.

Run 0 of every variant is the warm-up (code objects, the plans of this size) and is left out.  The table goes to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/eval_png_ab.py [--pairs 8] [--sizes 339x510,128x128,64x64] [--reps 3] [--out profiles/eval_png.txt]
"""
import argparse
import contextlib
import io
import json
import logging
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STAGES = ('run_inference', 'sr_and_scores', 'write')   # (write: png.FileWriter.write, the one place both paths save an image)


def write_pairs(lr_dir, hr_dir, n, h, w):
    """photograph-like HR images (a smooth field plus noise) and their 4 x 4 box averages as LR images"""
    from PIL import Image
    for i in range(n):
        g = torch.Generator().manual_seed(100 + i)
        base = torch.nn.functional.interpolate(torch.rand(1, 3, h // 4 + 2, w // 4 + 2, generator=g), size=(4 * h, 4 * w), mode='bilinear', align_corners=False)
        hr = (base + 0.02 * torch.randn(1, 3, 4 * h, 4 * w, generator=g)).clamp(0, 1)
        for folder, img in ((hr_dir, hr), (lr_dir, torch.nn.functional.avg_pool2d(hr, 4))):
            Image.fromarray((img[0].permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(os.path.join(folder, 'img_%02d.png' % i), compress_level=1)


def write_generator(path, sigma=0.005):
    """weights with which RRDB_net nf 64 nb 23 writes image-like SR images (a seeded generator writes nearly flat ones, which PIL encodes at a speed and to a size no
    photograph has): an identity tap for the three colour channels in conv_first, both up-convs, HRconv and conv_last, so the SR image is the nearest-neighbour x4 image of
    the LR image, plus seeded normal weights of deviation `sigma` everywhere, so every block contributes a little texture.  The kernels and their cost are those of any
    other weights."""
    from dasr_amd.rrdbnet import rrdbnet_param_spec
    g = torch.Generator().manual_seed(23)
    sd = {k: sigma * torch.randn(shape, generator=g) if k.endswith('weight') else torch.zeros(shape) for k, shape in rrdbnet_param_spec(3, 3, 64, 23)}
    for idx in (0, 3, 6, 8, 10):
        for c in range(3):
            sd['model.%d.weight' % idx][c, c, 1, 1] += 1.0
    torch.save(sd, path)
    return path


def opt_file(tmp, name, lr_dir, hr_dir, device_png):
    opt = {'name': name, 'use_tb_logger': False, 'model': 'sr', 'scale': 4, 'gpu_ids': [0], 'chop': True, 'val_lpips': False, 'device_metrics': True,
           'datasets': {'test_1': {'name': 'set', 'mode': 'LRHR', 'dataroot_HR': hr_dir, 'dataroot_LR': lr_dir}},
           'path': {'root': tmp, 'pretrain_model_G': os.path.join(tmp, 'G.pth')},
           'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': 23, 'in_nc': 3, 'out_nc': 3, 'gc': 32}}
    if device_png:
        opt['device_png'] = True
    path = os.path.join(tmp, name + '.json')
    with open(path, 'w') as f:
        json.dump(opt, f)
    return path


class Clock:
    """the named functions of a driver module replaced by versions that synchronise the device and add their seconds to self.t; self.wall: the seconds of `outer`"""

    def __init__(self, module, outer):
        self.module, self.outer, self.t, self.wall, self.saved = module, outer, {}, 0.0, {}

    def _wrap(self, owner, name, is_outer):
        fn = getattr(owner, name)

        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if is_outer:
                self.wall += dt
            else:
                self.t[name] = self.t.get(name, 0.0) + dt
            return r
        self.saved[(owner, name)] = fn
        setattr(owner, name, timed)

    def __enter__(self):
        from dasr_amd import png
        for name in STAGES:
            self._wrap(png.FileWriter if name == 'write' else self.module, name, False)
        self._wrap(self.module, self.outer, True)
        return self

    def __exit__(self, *exc):
        for (owner, name), fn in self.saved.items():
            setattr(owner, name, fn)
        return False


def quiet(fn):
    """fn() with the drivers' console output swallowed and their log handlers dropped afterwards"""
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        try:
            return fn()
        finally:
            for name in ('base', 'val'):
                lg = logging.getLogger(name)
                for h in list(lg.handlers):
                    h.close()
                    lg.removeHandler(h)


def progress(text):
    sys.stderr.write('[eval_png_ab] %s\n' % text)
    sys.stderr.flush()


def folder_bytes(folder):
    sizes = [os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(folder) for f in fs if f.endswith('.png')]
    return len(sizes), sum(sizes) / max(len(sizes), 1)


def row(label, n, clocks, files):
    """one table row from the Clock objects of the measured runs of a variant"""
    wall = statistics.median(c.wall for c in clocks) / n * 1e3
    parts = [statistics.median(c.t.get(s, 0.0) for c in clocks) / n * 1e3 for s in STAGES]
    return '| %s | %.1f | %.1f | %.2f | %.1f | %.1f | %d x %.0f |' % ((label, wall) + tuple(parts) + (wall - sum(parts),) + files), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--sizes', default='339x510,128x128,64x64')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--num_workers', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_png.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_png_ab.py needs the GPU: a CPU run says nothing about the device path')
    from dasr_amd import back_projection, options, test as dtest, train
    from dasr_amd.models import create_model
    sizes = [tuple(int(v) for v in s.split('x')) for s in a.sizes.split(',')]
    lines = ['SR images written by the device PNG encoder (`"device_png": true`, `--device_png`; png.FileWriter, %d host threads in the option-file drivers) against '
             "the default path (png.save_host: PIL's Image.save, compress_level 6, main thread)" % train.DEVICE_PNG_THREADS,
             'device: %s; host: %d CPUs available to the process, torch %s, numpy %s' % (torch.cuda.get_device_name(0), len(os.sched_getaffinity(0)), torch.__version__,
                                                                                       np.__version__),
             '%d pairs per folder (a smooth field plus noise of deviation 0.02), RRDB_net nf 64 nb 23 with the weights of write_generator (the SR image is the '
             'nearest-neighbour x4 image of the LR image plus a little texture), chop, device_metrics; one process, the variants alternating, run 0 of each is the warm-up, median of %d runs; '
             'ms per image; the stages are closed by device synchronisations' % (a.pairs, a.reps), '']
    head = ['| variant | wall | inference | scores | save (device_png: filter .. pack, two read-backs, hand-off to the pool) | rest (decode + upload of the pair, logging, '
            'the wait for the writer) | files x mean bytes |', '|---|---|---|---|---|---|---|']
    with tempfile.TemporaryDirectory() as tmp:
        write_generator(os.path.join(tmp, 'G.pth'))
        folders = {}
        for h, w in sizes:
            lr_dir, hr_dir = os.path.join(tmp, 'LR_%dx%d' % (h, w)), os.path.join(tmp, 'HR_%dx%d' % (h, w))
            os.makedirs(lr_dir)
            os.makedirs(hr_dir)
            write_pairs(lr_dir, hr_dir, a.pairs, h, w)
            progress('wrote %d pairs at LR %d x %d' % (a.pairs, h, w))
            folders[(h, w)] = (lr_dir, hr_dir)
        # 1. the evaluation CLI
        for h, w in sizes:
            lr_dir, hr_dir = folders[(h, w)]
            runs = {False: [], True: []}
            for rep in range(a.reps + 1):
                for key in (False, True):
                    name = 'eval_%dx%d_%s_%d' % (h, w, 'dev' if key else 'host', rep)
                    with Clock(dtest, 'evaluate') as c:
                        quiet(lambda: dtest.main(['-opt', opt_file(tmp, name, lr_dir, hr_dir, key)]))
                    c.files = folder_bytes(os.path.join(tmp, 'results', name))
                    progress('%s: %.2f s' % (name, c.wall))
                    if rep:
                        runs[key].append(c)
            lines += ['## python -m dasr_amd.test, LR %d x %d, SR %d x %d' % (h, w, 4 * h, 4 * w), ''] + head
            r_host, w_host = row('default (PIL level 6)', a.pairs, runs[False], runs[False][0].files)
            r_dev, w_dev = row('device_png', a.pairs, runs[True], runs[True][0].files)
            ratio = runs[True][0].files[1] / runs[False][0].files[1]
            lines += [r_host, r_dev, '', 'wall: %.2fx (%s); the device files carry no LZ77 matches: %.2fx the bytes of PIL level 6 (%s)' % (
                w_host / w_dev, 'device_png is faster' if w_dev < w_host else 'device_png does NOT pay at this size', ratio, 'larger' if ratio > 1 else 'not larger'), '']
        # 2. one validation pass
        h, w = sizes[0]
        lr_dir, hr_dir = folders[(h, w)]
        opt = options.dict_to_nonedict(options.parse(opt_file(tmp, 'val', lr_dir, hr_dir, False), is_train=False))
        model = quiet(lambda: create_model(opt))
        val_set = train.create_dataset(dict(opt['datasets']['test_1'], phase='val'), opt)
        runs = {False: [], True: []}
        for rep in range(a.reps + 1):
            for key in (False, True):
                opt['device_png'] = True if key else None
                opt['path']['val_images'] = os.path.join(tmp, 'val_images_%s_%d' % ('dev' if key else 'host', rep))
                with Clock(train, 'validate') as c:
                    quiet(lambda: train.validate(model, val_set, opt, rep, logging.getLogger('eval_png_ab')))
                c.files = folder_bytes(opt['path']['val_images'])
                progress('validate %s %d: %.2f s' % ('dev' if key else 'host', rep, c.wall))
                if rep:
                    runs[key].append(c)
        lines += ['## one train.validate pass, LR %d x %d, %d images (PSNR only)' % (h, w, a.pairs), ''] + head
        r_host, w_host = row('default (PIL level 6)', a.pairs, runs[False], runs[False][0].files)
        r_dev, w_dev = row('device_png', a.pairs, runs[True], runs[True][0].files)
        lines += [r_host, r_dev, '', 'a validation pass holds the training loop for %.2f s instead of %.2f s (%.2fx)' % (w_dev * a.pairs / 1e3, w_host * a.pairs / 1e3, w_host / w_dev), '']
        del model
        # 3. the back-projection CLI
        lines += ['## python -m dasr_amd.back_projection --iters 20 --num_workers %d (decode threads; with the flag also the threads of the writer)' % a.num_workers, '',
                  '| LR size | default, ms per file | --device_png, ms per file | ratio | mean bytes default | mean bytes --device_png |', '|---|---|---|---|---|---|']
        for h, w in sizes:
            lr_dir, hr_dir = folders[(h, w)]
            ts, files = {False: [], True: []}, {}
            for rep in range(a.reps + 1):
                for key in (False, True):
                    out_dir = os.path.join(tmp, 'bp_%dx%d_%s_%d' % (h, w, 'dev' if key else 'host', rep))
                    argv = ['--lr_dir', lr_dir, '--sr_dir', hr_dir, '--out_dir', out_dir, '--num_workers', str(a.num_workers)] + (['--device_png'] if key else [])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    quiet(lambda: back_projection.main(argv))
                    torch.cuda.synchronize()
                    if rep:
                        ts[key].append(time.perf_counter() - t0)
                    files[key] = folder_bytes(out_dir)[1]
                    progress('back_projection %d x %d %s %d: %.2f s' % (h, w, 'dev' if key else 'host', rep, time.perf_counter() - t0))
            t_host, t_dev = (statistics.median(ts[k]) / a.pairs * 1e3 for k in (False, True))
            lines.append('| %d x %d | %.1f | %.1f | %.2fx | %.0f | %.0f |' % (h, w, t_host, t_dev, t_host / t_dev, files[False], files[True]))
        lines.append('')
        # 4. one file by content
        from PIL import Image
        from dasr_amd import png
        rng = np.random.default_rng(7)
        contents = {'flat (128)': np.full((512, 512, 3), 128, np.uint8),
                    'ramp (x * 255 // 511 in every row and channel)': np.ascontiguousarray(np.broadcast_to((np.arange(512) * 255 // 511).astype(np.uint8)[None, :, None], (512, 512, 3))),
                    'png.photo(512, 512, 1)': png.photo(512, 512, 1), 'uniform random bytes': rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)}
        lines += ['## one 512 x 512 file by content (BGR tensor on the device; PIL: Image.fromarray(...).save(buffer), level 6, one thread; median of 5)', '',
                  '| content | PIL bytes | PIL ms | device bytes | device ms (encode_batch: tables, five launches, two read-backs, container) | bytes ratio |', '|---|---|---|---|---|---|']
        for label, img in contents.items():
            t_dev = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).cuda()
            tp, td = [], []
            for _ in range(6):
                t0 = time.perf_counter()
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, 'PNG')
                tp.append(time.perf_counter() - t0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                data = png.encode_batch([t_dev], fmt='bgr')[0]
                td.append(time.perf_counter() - t0)
            with Image.open(io.BytesIO(data)) as im:
                assert np.array_equal(np.array(im), img), label
            nb = len(buf.getvalue())
            lines.append('| %s | %d | %.2f | %d | %.2f | %.2fx |' % (label, nb, statistics.median(tp[1:]) * 1e3, len(data), statistics.median(td[1:]) * 1e3, len(data) / nb))
        lines.append('')
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
