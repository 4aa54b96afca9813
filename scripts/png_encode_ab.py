"""Measurement of the device PNG encoder (dasr_amd/png.py, csrc/png.hip, `--device_png`) in ONE process, on synthetic 2040 x 1356 inputs with 40 sub-images each, as
scripts/prepare_data_ab.py makes them: the 120 products of a file are its 40 sub-images (480 x 480), their LR images (120 x 120) and their Bic images (480 x 480).

  pil        (a) the parent commit's path: the 120 products of one file through PIL at zlib level 3 into files, on 1 and on 16 threads (the raw bytes already on the host)
  device     (b) the same products through png.write_batch on a 16-thread pool, from the tensors on the device to closed files: wall clock, and its parts with the stream
             synchronised in between (tables + upload, the five launches, the two read-backs, container + Adler + CRC + write on the pool)
  crc        zlib.crc32 over the packed bytes of one file's products on one thread: the host's share per byte
  kernels    every launch inside a profiling session of the library (the dispatch's own begin / end timestamps), --reps times: median time, algorithmic bytes over that time
             against the 6.3 TB/s a streaming kernel achieves from HBM on this device
  bytes      what both paths write for the same products
  cli        prepare_data.run (--sub_dir --lr_dir --bic_dir) and add_corruptions.run (noise 8, JPEG 30) on --files files and 16 threads with and without --device_png,
             alternating, wall clock per input file
  fibonacci  the code stage on Fibonacci counts over 24 symbols (an unrestricted tree 23 deep): coded bits over the unrestricted optimum

The table goes to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/png_encode_ab.py [--files 4] [--reps 10] [--out profiles/png_encode.txt]
"""
import argparse
import ctypes as C
import heapq
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s, streaming kernels on MI355X
H, W, CROP, STEP, THRES, S = 1356, 2040, 480, 240, 48, 4
THREADS = 16


def synthetic(seed):
    """uint8 [H, W, 3]: a 12 x 17 random colour field enlarged bilinearly, plus uniform noise of +-4 grey levels (the inputs of scripts/prepare_data_ab.py)"""
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


def med_ms(ts):
    return '%.1f ms (min %.1f, max %.1f, n %d)' % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=4)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: a timing taken anywhere else says nothing about it')
    from PIL import Image
    from dasr_amd import add_corruptions, bicubic, png, prepare_data
    dev = torch.device('cuda')
    lines = ['# scripts/png_encode_ab.py --files %d --reps %d: %s, torch %s' % (args.files, args.reps, torch.cuda.get_device_name(0), torch.__version__)]
    root = tempfile.mkdtemp(prefix='png_encode_ab_')
    try:
        hr = os.path.join(root, 'HR')
        os.makedirs(hr)
        imgs = [synthetic(k) for k in range(args.files)]
        for k, a in enumerate(imgs):
            Image.fromarray(a).save(os.path.join(hr, '%04d.png' % (k + 1)))
        origins = prepare_data.window_grid(H, W, CROP, STEP, THRES)
        dimg = torch.from_numpy(imgs[0]).to(dev)
        lr_u8, lr_f64 = bicubic.down_windows_u8(dimg, origins, (CROP, CROP), S, want_f64=True)
        bic_u8 = bicubic.upsample(lr_f64, S, out='u8')
        tensors = [dimg[y:y + CROP, x:x + CROP] for y, x in origins] + [lr_u8[k] for k in range(len(origins))] + [bic_u8[k] for k in range(len(origins))]
        arrays = [np.ascontiguousarray(t.cpu().numpy()) for t in tensors]
        raw = sum(a.size for a in arrays)
        out = os.path.join(root, 'out')
        os.makedirs(out)
        paths = [os.path.join(out, '%03d.png' % k) for k in range(len(tensors))]
        lines.append('# one %d x %d file: %d products (%d sub-images %d x %d, their LR and Bic images), %.1f MB of pixels, %d strips of at most %d filtered bytes' % (
            W, H, len(tensors), len(origins), CROP, CROP, raw / 1e6, png.Plan(tensors).n_strips, png.STRIP_TARGET))
        # (a) PIL
        t_pil = {}
        for threads in (1, THREADS):
            ts = []
            with ThreadPoolExecutor(max_workers=threads) as pool:
                for _ in range(max(2, args.reps // 3) + 1):
                    t0 = time.perf_counter()
                    list(pool.map(lambda arr, path: png.save_host(arr, path, 'rgb', prepare_data.PNG_COMPRESSION), arrays, paths))
                    ts.append(time.perf_counter() - t0)
            t_pil[threads] = ts[1:]
            lines.append('pil     %2d thread(s), zlib level %d, %d products into files: %s' % (threads, prepare_data.PNG_COMPRESSION, len(arrays), med_ms(ts[1:])))
        pil_bytes = sum(os.path.getsize(p) for p in paths)
        for a, p in zip(arrays, paths):
            assert np.array_equal(np.array(Image.open(p)), a)
        # (b) the device
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            def device():
                for f in png.write_batch(tensors, paths, pool):
                    f.result()
            device()
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                device()
                ts.append(time.perf_counter() - t0)
            lines.append('device  png.write_batch, %d-thread pool, %d products from device tensors into files: %s' % (THREADS, len(tensors), med_ms(ts)))
            t_dev = ts
            dev_bytes = sum(os.path.getsize(p) for p in paths)
            for a, p in zip(arrays, paths):
                assert np.array_equal(np.array(Image.open(p)), a)
            parts = []
            for _ in range(args.reps):
                t = {}
                t0 = time.perf_counter()
                futures = png.write_batch(tensors, paths, pool, times=t)
                t1 = time.perf_counter()
                for f in futures:
                    f.result()
                t['pool'] = time.perf_counter() - t1
                t['all'] = time.perf_counter() - t0
                parts.append(t)
            keys = ('plan', 'kernels', 'readback_meta', 'readback_bytes', 'pool', 'all')
            lines.append('        parts, stream synchronised in between, median ms: ' + ', '.join('%s %.2f' % (k, 1e3 * statistics.median(t[k] for t in parts)) for k in keys))
            lines.append('        (plan: tables on the host and their one upload; pool: container, Adler-32, CRC and write of %d files on %d threads)' % (len(tensors), THREADS))
        # crc on one thread
        plan, m, packed = png._encode_device(tensors)
        buf = packed.tobytes()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            zlib.crc32(buf)
            ts.append(time.perf_counter() - t0)
        lines.append('crc     zlib.crc32 of the %.1f MB of packed strips on one thread: %.2f ms, %.2f GB/s' % (len(buf) / 1e6, 1e3 * min(ts), len(buf) / min(ts) / 1e9))
        lines.append('bytes   PIL level %d: %.2f MB; device: %.2f MB (%.1f %% of PIL); pixels %.1f MB' % (prepare_data.PNG_COMPRESSION, pil_bytes / 1e6, dev_bytes / 1e6,
                                                                                                     100.0 * dev_bytes / pil_bytes, raw / 1e6))
        verdict = statistics.median(t_dev) < statistics.median(t_pil[THREADS])
        lines.append('verdict (b) %.1f ms against (a) at %d threads %.1f ms: the device path is %s (%.2f x)' % (
            1e3 * statistics.median(t_dev), THREADS, 1e3 * statistics.median(t_pil[THREADS]), 'FASTER' if verdict else 'NOT faster',
            statistics.median(t_pil[THREADS]) / statistics.median(t_dev)))
        # kernels
        recs = []
        for _ in range(args.reps):
            recs += profiled(lambda: png._encode_device(tensors))
        filt_bytes = int(plan.strips['n'].sum())
        coded = int(m[1])
        ns = plan.n_strips
        traffic = {'png_filter_kernel': raw + filt_bytes + ns * (257 + 2) * 4, 'png_codes_kernel': ns * (257 * 4 + 257 * 3 + 64 * 4),
                   'png_emit_kernel': filt_bytes + ns * (257 * 3 + 64 * 4) + coded, 'png_scan_kernel': ns * (4 + 8 + 32), 'png_gather_kernel': 2 * coded + ns * 12}
        total_us = 0.0
        for tag, nbytes in traffic.items():
            us = [u for t, u in recs if t == tag][1:]   # (the first launch left out: cold caches)
            med = statistics.median(us)
            total_us += med
            rate = nbytes / (med * 1e-6)
            lines.append('kernel  %-18s %8.3f MB  median %8.2f us (min %.2f, max %.2f, n %d)  %6.3f TB/s  %5.1f %% of 6.3 TB/s' % (
                tag, nbytes / 1e6, med, min(us), max(us), len(us), rate / 1e12, 100 * rate / HBM_ACHIEVABLE))
        lines.append('        the five launches together: %.1f us per file of 120 products' % total_us)
        # cli, alternating
        argv = ['--input_dir', hr, '--crop_sz', str(CROP), '--step', str(STEP), '--thres_sz', str(THRES), '--scale', str(S), '--num_workers', str(THREADS), '--overwrite',
                '--sub_dir', os.path.join(root, 'sub'), '--lr_dir', os.path.join(root, 'lr'), '--bic_dir', os.path.join(root, 'bic')]
        t_cli = {False: [], True: []}
        for rep in range(3):
            for flag in (False, True):
                t0 = time.perf_counter()
                written = prepare_data.run(prepare_data.parse_args(argv + (['--device_png'] if flag else [])))
                if rep:   # (the first pair warms tables, code objects and the allocator)
                    t_cli[flag].append(time.perf_counter() - t0)
        for flag in (False, True):
            lines.append('cli     prepare_data on %d files -> %d PNG files, %d threads, %s: %.0f ms per input file (runs: %s)' % (
                args.files, sum(len(v) for v in written.values()), THREADS, '--device_png' if flag else 'PIL (default)', 1e3 * statistics.median(t_cli[flag]) / args.files,
                ', '.join('%.2f s' % t for t in t_cli[flag])))
        argv = ['--input_dir', hr, '--output_dir', os.path.join(root, 'noisy'), '--noise_std_dev', '8', '--jpg_quality', '30', '--num_workers', str(THREADS), '--overwrite']
        t_cli = {False: [], True: []}
        for rep in range(3):
            for flag in (False, True):
                t0 = time.perf_counter()
                written = add_corruptions.run(add_corruptions.parse_args(argv + (['--device_png'] if flag else [])))
                if rep:
                    t_cli[flag].append(time.perf_counter() - t0)
        for flag in (False, True):
            lines.append('cli     add_corruptions on %d files -> %d PNG files, %d threads, %s: %.0f ms per input file (runs: %s)' % (
                args.files, len(written), THREADS, '--device_png' if flag else 'PIL level %d (default)' % add_corruptions.PNG_COMPRESSION,
                1e3 * statistics.median(t_cli[flag]) / args.files, ', '.join('%.2f s' % t for t in t_cli[flag])))
        # fibonacci
        f = [1, 1]
        while len(f) < 24:
            f.append(f[-1] + f[-2])
        hist = [0] * (257 - 24) + f
        lens = png.codes_batch(torch.tensor([hist], dtype=torch.int32, device=dev))[0].cpu().numpy()[0]
        h = list(f)
        heapq.heapify(h)
        best = 0
        while len(h) > 1:
            a = heapq.heappop(h) + heapq.heappop(h)
            best += a
            heapq.heappush(h, a)
        cost = sum(c * int(l) for c, l in zip(hist, lens))
        lines.append('fibonacci  24 symbols, unrestricted depth 23, limited to 15: %d bits against the unrestricted optimum %d, ratio %.6f' % (cost, best, cost / best))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
