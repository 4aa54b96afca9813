"""Measurement of the dataset preparation (`python -m dasr_amd.prepare_data`, dasr_amd/bicubic.py) in ONE process, on a folder of --files synthetic 2040 x 1356 PNG files
(a DIV2K image's size; smooth colour fields plus noise of a few grey levels, so that the PNG codec has something to compress), with --sub_dir, --lr_dir and --bic_dir at
scale 4: 40 sub-images of 480 x 480 per file, each with its 120 x 120 LR and 480 x 480 Bic image.

  run        prepare_data.run on --workers host threads: wall clock of the whole folder, and per file the time of decode (as the consumer waits for it), upload, the two
             launches (each synchronised, which an ordinary run does not do), read-back, and what the consumer waits for the encoders
  codec      decode of one file and PNG encoding of one file's 120 products on ONE thread: what the worker threads share out
  host       the same LR and Bic bytes from the restatements (bicubic.down_windows_fp64, upsample_fp64, quantise) on 16 torch threads for --host-windows windows, scaled
             to a file's 40: the only way to make them without these kernels
  kernels    the two launches of one file inside a profiling session of the library (the dispatch's own begin / end timestamps), --reps times: median time, algorithmic
             bytes (down: every window's bytes read once, LR bytes and LR doubles written; up: LR doubles read, Bic bytes written) over that time against the 6.3 TB/s a
             streaming kernel achieves from HBM on this device, and the fp64 operations and LDS reads the kernels issue per file, counted from the shapes
  reverse    backproject.reverse_filter, 20 iterations at LR 339 x 510 -> SR 1356 x 2040, next to back_project, and the largest error of 20 iterations against
             reverse_filter_fp64 in units of 2^-24 on the six cases of tests/test_gpu_prepare_data.py

The table goes to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/prepare_data_ab.py [--files 4] [--workers 6] [--reps 20] [--host-windows 4] [--out profiles/prepare_data.txt]
"""
import argparse
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s, streaming kernels on MI355X
H, W, CROP, STEP, THRES, S = 1356, 2040, 480, 240, 48, 4


def synthetic(seed):
    """uint8 [H, W, 3]: a 12 x 17 random colour field enlarged bilinearly, plus uniform noise of +-4 grey levels"""
    g = torch.Generator().manual_seed(seed)
    field = torch.nn.functional.interpolate(torch.rand(1, 3, 12, 17, generator=g), size=(H, W), mode='bilinear', align_corners=True)[0]
    img = field * 255.0 + (torch.rand(3, H, W, generator=g) * 8.0 - 4.0)
    return img.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def profiled(fn, capacity=256):
    """[(kernel tag, microseconds)] of every launch of the library inside fn()"""
    from dasr_amd import _lib
    L = _lib.lib()
    torch.cuda.synchronize()
    _lib.check(L.dasr_prof_begin(capacity), 'prof_begin')
    fn()
    torch.cuda.synchronize()
    us, fl, by = (C.c_float * capacity)(), (C.c_double * capacity)(), (C.c_double * capacity)()
    op, tg = (C.c_int32 * capacity)(), (C.c_char_p * capacity)()
    n = L.dasr_prof_end(capacity, us, fl, by, op, tg)
    if n < 0:
        raise RuntimeError('dasr_prof_end: %d' % n)
    return [(tg[i].decode(), us[i]) for i in range(n)]


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=4)
    ap.add_argument('--workers', type=int, default=6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-windows', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: a timing taken anywhere else says nothing about it')
    from PIL import Image
    from dasr_amd import backproject, bicubic, imgio, png, prepare_data
    from dasr_amd.data import imresize_matlab
    dev = torch.device('cuda')
    torch.set_num_threads(16)
    lines = ['# scripts/prepare_data_ab.py --files %d --workers %d --reps %d --host-windows %d: %s, torch %s, %d torch threads' % (
        args.files, args.workers, args.reps, args.host_windows, torch.cuda.get_device_name(0), torch.__version__, torch.get_num_threads())]
    root = tempfile.mkdtemp(prefix='prepare_data_ab_')
    try:
        hr = os.path.join(root, 'HR')
        os.makedirs(hr)
        for k in range(args.files):
            Image.fromarray(synthetic(k)).save(os.path.join(hr, '%04d.png' % (k + 1)))
        size = statistics.mean(os.path.getsize(os.path.join(hr, f)) for f in os.listdir(hr))
        lines.append('# %d synthetic %d x %d PNG files of %.1f MB; crop_sz %d, step %d, thres_sz %d, scale %d: 40 sub-images per file' % (args.files, W, H, size / 1e6, CROP, STEP, THRES, S))
        argv = ['--input_dir', hr, '--crop_sz', str(CROP), '--step', str(STEP), '--thres_sz', str(THRES), '--scale', str(S), '--num_workers', str(args.workers), '--overwrite',
                '--sub_dir', os.path.join(root, 'sub'), '--lr_dir', os.path.join(root, 'lr'), '--bic_dir', os.path.join(root, 'bic')]
        # run: once untimed (tables, code objects, the allocator), once without the per-stage synchronisations, once with them
        prepare_data.run(prepare_data.parse_args(argv))
        t0 = time.perf_counter()
        written = prepare_data.run(prepare_data.parse_args(argv))
        t_run = time.perf_counter() - t0
        times = []
        t0 = time.perf_counter()
        prepare_data.run(prepare_data.parse_args(argv), times)
        t_staged = time.perf_counter() - t0
        nfiles = sum(len(v) for v in written.values())
        lines.append('run     %d files -> %d PNG files on %d threads: %.2f s wall clock, %.0f ms per input file (%.2f s with every stage synchronised)' % (
            args.files, nfiles, args.workers, t_run, 1e3 * t_run / args.files, t_staged))
        lines.append('        per file, ms:   decode wait   upload     down       up  read-back   submit  encode wait')
        for t in times:
            lines.append('        %-12s %11.1f %8.2f %8.3f %8.3f %10.2f %8.1f %12.1f' % (
                os.path.basename(t['file']), *(1e3 * t.get(k, 0.0) for k in ('decode', 'upload', 'down', 'up', 'readback', 'submit', 'encode_wait'))))
        dev_ms = statistics.median(1e3 * (t['upload'] + t['down'] + t['up'] + t['readback']) for t in times)
        # codec on one thread
        path = os.path.join(hr, '0001.png')
        t0 = time.perf_counter()
        img = imgio.decode_u8(path)
        t_dec = time.perf_counter() - t0
        products = [os.path.join(root, d, f) for d in ('sub', 'lr', 'bic') for f in sorted(os.listdir(os.path.join(root, d))) if f.startswith('0001_')]
        arrays = [np.array(Image.open(p)) for p in products]
        t0 = time.perf_counter()
        for a, p in zip(arrays, products):
            png.save_host(a, p, 'rgb', prepare_data.PNG_COMPRESSION)
        t_enc = time.perf_counter() - t0
        lines.append('codec   one thread: decode of one file %.0f ms, PNG encoding of its %d products at zlib level %d %.0f ms; upload + launches + read-back %.1f ms per file (median), %.2f %% of'
                     ' decode + encode' % (1e3 * t_dec, len(products), prepare_data.PNG_COMPRESSION, 1e3 * t_enc, dev_ms, 100 * dev_ms / (1e3 * (t_dec + t_enc))))
        # host restatement
        origins = prepare_data.window_grid(H, W, CROP, STEP, THRES)
        t0 = time.perf_counter()
        ref_u8, ref_f64 = bicubic.down_windows_fp64(img, origins[:args.host_windows], CROP, S)
        ref_bic = bicubic.quantise(bicubic.upsample_fp64(ref_f64, S))
        t_host = (time.perf_counter() - t0) * len(origins) / args.host_windows
        dimg = torch.from_numpy(img).to(dev)

        def launches():
            lr_u8, lr_f64 = bicubic.down_windows_u8(dimg, origins, CROP, S)
            return lr_u8, bicubic.upsample(lr_f64, S, out='u8')
        lr_u8, bic_u8 = launches()
        t_dev = wall(launches, args.reps)
        k = args.host_windows
        diff = (int((lr_u8[:k].cpu() != ref_u8).sum()), int((bic_u8[:k].cpu() != ref_bic.permute(0, 2, 3, 1)).sum()))
        lines.append('host    down_windows_fp64 + upsample_fp64 + quantise, 16 threads, scaled to 40 windows from %d: %.2f s per file; the two launches: %.3f ms wall clock'
                     ' (median of %d); bytes that differ in the %d windows: LR %d, Bic %d' % (k, t_host, 1e3 * statistics.median(t_dev), args.reps, k, diff[0], diff[1]))
        lines.append('        (kernel ratio %.0f: NOT the speed-up of the preparation, whose wall clock is decode and encode on the host threads -- see `run` and `codec`)' % (
            t_host / statistics.median(t_dev)))
        # kernels
        n, hl = len(origins), CROP // S
        recs = []
        for _ in range(args.reps):
            recs += profiled(launches)
        traffic = {'windows_down_u8_kernel': n * (CROP * CROP * 3 + hl * hl * 3 + 3 * hl * hl * 8), 'imresize_up_kernel': n * (3 * hl * hl * 8 + CROP * CROP * 3)}
        taps = 4 * S + 2
        rt, ct = bicubic.DOWN_TILE
        wgs = n * -(-hl // rt) * -(-hl // ct)
        row_out = rt * 3 * (S * ct + 3 * S + 4)
        uy, ux = bicubic.UP_TILE
        up_wgs, up_out = n * 3 * -(-CROP // uy) * -(-CROP // ux), uy * ((ux - 1 + S - 1) // S + 8) + uy * ux   # row-pass and column-pass outputs of a tile
        # fp64 operations (a product and a sum per tap) and LDS reads per lane (row pass of the window kernel: weight, row offset, byte, table entry; every other pass:
        # weight, index, sample)
        work = {'windows_down_u8_kernel': (wgs * (row_out + 3 * rt * ct) * taps * 2, wgs * (row_out * 4 + 3 * rt * ct * 3) * taps),
                'imresize_up_kernel': (up_wgs * up_out * 6 * 2, up_wgs * up_out * 6 * 3)}
        for tag, nbytes in traffic.items():
            us = [u for t, u in recs if t == tag][1:]   # (the first launch left out: cold caches)
            med = statistics.median(us)
            rate = nbytes / (med * 1e-6)
            flops, lds = work[tag]
            lines.append('kernel  %-22s %6.2f MB  median %8.2f us (min %.2f, max %.2f, n %d)  %6.3f TB/s  %5.1f %% of 6.3 TB/s;  %.0f MFLOP fp64 (%.2f TFLOP/s), %.1f M LDS reads'
                         ' per lane (%.1f G/s)' % (tag, nbytes / 1e6, med, min(us), max(us), len(us), rate / 1e12, 100 * rate / HBM_ACHIEVABLE, flops / 1e6,
                                                   flops / (med * 1e-6) / 1e12, lds / 1e6, lds / (med * 1e-6) / 1e9))
        # reverse filter
        g = torch.Generator().manual_seed(1)
        hrt = torch.rand(3, H, W, generator=g)
        lr = imresize_matlab(hrt, 1.0 / S)[None].contiguous()
        sr = (hrt + 0.05 * torch.randn(hrt.shape, generator=g))[None].contiguous()
        srd, lrd = sr.to(dev), lr.to(dev)
        for fn in (backproject.reverse_filter, backproject.back_project):
            for _ in range(3):
                fn(srd, lrd, 20)
            ts = wall(lambda: fn(srd, lrd, 20), args.reps)
            lines.append('reverse %-15s 20 iterations, LR %d x %d -> SR %d x %d: median %.3f ms (min %.3f, max %.3f)' % (
                fn.__name__, H // S, W // S, H, W, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)))
        up = [u for t, u in profiled(lambda: backproject.reverse_filter(srd, lrd, 20)) if t == 'imresize_up_kernel'][1:]
        nbytes = 3 * (2 * H * W + (H // S) * (W // S)) * 4
        lines.append('        imresize_up_kernel (fp32, accumulate) %.2f MB  median %.2f us  %.3f TB/s  %.1f %% of 6.3 TB/s' % (
            nbytes / 1e6, statistics.median(up), nbytes / (statistics.median(up) * 1e-6) / 1e12, 100 * nbytes / (statistics.median(up) * 1e-6) / HBM_ACHIEVABLE))
        worst = 0.0
        for s in (2, 3, 4):
            for h, w in ((9, 13), (1, 1)):
                g = torch.Generator().manual_seed(77 * h + s)
                a = torch.rand(3, s * h, s * w, generator=g)
                b = imresize_matlab(a, 1.0 / s)
                a, b = (a + 0.05 * torch.randn(a.shape, generator=g))[None].contiguous(), b[None].contiguous()
                err = float((backproject.reverse_filter(a.to(dev), b.to(dev), 20).cpu().double() - backproject.reverse_filter_fp64(a, b, 20)).abs().max()) / 2.0 ** -24
                lines.append('        reverse_filter x%d LR %d x %d, 20 iterations: max |device - reverse_filter_fp64| = %.2f x 2^-24' % (s, h, w, err))
                worst = max(worst, err)
        lines.append('        largest: %.2f x 2^-24 (the test bounds it at about 8 x that)' % worst)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
