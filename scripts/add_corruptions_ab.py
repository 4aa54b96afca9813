"""Measurement of the DSN corruption step (`python -m dasr_amd.add_corruptions`, dasr_amd/corrupt.py) in ONE process at 2040 x 1356 (a DIV2K image's size; synthetic smooth
colour fields plus noise of a few grey levels), the variants alternating after a warm-up:

  kernels    jpeg_blocks_kernel, jpeg_merge_kernel and noise_u8_kernel inside a profiling session of the library (the dispatch's own begin / end timestamps), --reps
             times: median time, the bytes each moves (blocks: image read, planes written; merge: planes read, image written; noise: image read and written) over that
             time against the 6.3 TB/s a streaming kernel achieves from HBM on this device, and the integer multiplications (blocks) / Philox rounds and fp64
             transcendentals (noise) the launch issues, counted from the shapes
  roundtrip  corrupt.jpeg_roundtrip (both launches and the two allocations, wall clock with a synchronisation) next to PIL's save + open of the same bytes on ONE
             host thread, alternating, --reps times; the bytes that differ between the two
  cli        add_corruptions.run on a folder of --files such PNG files with --workers threads: wall clock per file, and per file the time of decode (as the consumer
             waits for it), upload, kernels (synchronised, which an ordinary run does not do), read-back, submit and the wait for the encoders; decode and PNG encode
             of one file on one thread; the reference's host sequence (numpy noise, PIL JPEG round trip, PNG) on one thread

The table goes to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/add_corruptions_ab.py [--files 6] [--workers 6] [--reps 20] [--out profiles/add_corruptions.txt]
"""
import argparse
import ctypes as C
import io
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
H, W = 1356, 2040


def synthetic(seed):
    """uint8 [H, W, 3]: a 12 x 17 random colour field enlarged bilinearly, plus uniform noise of +-4 grey levels"""
    g = torch.Generator().manual_seed(seed)
    field = torch.nn.functional.interpolate(torch.rand(1, 3, 12, 17, generator=g), size=(H, W), mode='bilinear', align_corners=True)[0]
    img = field * 255.0 + (torch.rand(3, H, W, generator=g) * 8.0 - 4.0)
    return img.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def profiled(fn, capacity=64):
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


def pil_roundtrip(a, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, 'JPEG', quality=q)
    buf.seek(0)
    return np.array(Image.open(buf))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=6)
    ap.add_argument('--workers', type=int, default=6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: a timing taken anywhere else says nothing about it')
    from PIL import Image
    from dasr_amd import add_corruptions, corrupt, imgio, png
    dev = torch.device('cuda')
    lines = ['# scripts/add_corruptions_ab.py --files %d --workers %d --reps %d: %s, torch %s, PIL %s' % (
        args.files, args.workers, args.reps, torch.cuda.get_device_name(0), torch.__version__, Image.__version__)]
    img = synthetic(0)
    x = torch.from_numpy(img).to(dev)
    px = H * W
    # kernels
    for _ in range(3):
        corrupt.jpeg_roundtrip(x, 30)
        corrupt.gaussian_noise(x, 8.0, 1, 0)
    recs = []
    for _ in range(args.reps):
        recs += profiled(lambda: (corrupt.jpeg_roundtrip(x, 30), corrupt.gaussian_noise(x, 8.0, 1, 0)))
    planes = corrupt.plane_bytes(H, W)
    nblocks = -(-H // 8) * -(-W // 8) + 2 * -(-(-(-H // 2)) // 8) * -(-W // 16)
    # per 8 x 8 block: four passes of 8 rows with 12 constant multiplications each, 64 divisions; per pixel 3 (Y) + 2 x 3 (Cb, Cr) multiplications of the colour conversion
    notes = {'jpeg_blocks_kernel': (3 * px + planes, '%.1f M int32 multiplications, %.1f M int32 divisions' % ((nblocks * 4 * 8 * 12 + 9 * px) / 1e6, nblocks * 64 / 1e6)),
             'jpeg_merge_kernel': (planes + 3 * px, '%.1f M int32 multiplications' % (4 * px / 1e6)),
             'noise_u8_kernel': (6 * px, '%.1f M Philox rounds (2 wide multiplications each), %.1f M fp64 log / sqrt / cos / sin' % (10 * 3 * px / 4 / 1e6, 3 * px / 1e6))}
    total_us = {}
    for tag, (nbytes, work) in notes.items():
        us = [u for t, u in recs if tag in t][1:]   # (the first launch left out: cold caches)
        med = statistics.median(us)
        total_us[tag] = med
        rate = nbytes / (med * 1e-6)
        lines.append('kernel  %-20s %6.2f MB  median %8.2f us (min %.2f, max %.2f, n %d)  %6.3f TB/s  %5.1f %% of 6.3 TB/s;  %s' % (
            tag, nbytes / 1e6, med, min(us), max(us), len(us), rate / 1e12, 100 * rate / HBM_ACHIEVABLE, work))
    lines.append('        round trip = blocks + merge: %.2f us of device time per %d x %d image (%.2f ns per 8 x 8 block)' % (
        total_us['jpeg_blocks_kernel'] + total_us['jpeg_merge_kernel'], W, H, 1e3 * (total_us['jpeg_blocks_kernel'] + total_us['jpeg_merge_kernel']) / nblocks))
    # round trip against PIL, alternating
    t_dev, t_pil = [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = corrupt.jpeg_roundtrip(x, 30)
        torch.cuda.synchronize()
        t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = pil_roundtrip(img, 30)
        t_pil.append(time.perf_counter() - t0)
    lines.append('roundtrip  corrupt.jpeg_roundtrip %.3f ms wall clock (median of %d; min %.3f, max %.3f); PIL save + open on one thread %.1f ms (min %.1f, max %.1f); '
                 'bytes that differ: %d' % (1e3 * statistics.median(t_dev), args.reps, 1e3 * min(t_dev), 1e3 * max(t_dev), 1e3 * statistics.median(t_pil), 1e3 * min(t_pil),
                                            1e3 * max(t_pil), int((y.cpu().numpy() != ref).sum())))
    # the CLI
    root = tempfile.mkdtemp(prefix='add_corruptions_ab_')
    try:
        src, out = os.path.join(root, 'clean'), os.path.join(root, 'out')
        os.makedirs(src)
        for k in range(args.files):
            Image.fromarray(synthetic(k)).save(os.path.join(src, '%04d.png' % (k + 1)))
        size = statistics.mean(os.path.getsize(os.path.join(src, f)) for f in os.listdir(src))
        argv = ['--input_dir', src, '--output_dir', out, '--num_workers', str(args.workers), '--overwrite', '--seed', '1']
        add_corruptions.run(add_corruptions.parse_args(argv))
        t0 = time.perf_counter()
        written = add_corruptions.run(add_corruptions.parse_args(argv))
        t_run = time.perf_counter() - t0
        times = []
        t0 = time.perf_counter()
        add_corruptions.run(add_corruptions.parse_args(argv), times)
        t_staged = time.perf_counter() - t0
        lines.append('cli     %d synthetic %d x %d PNG files of %.1f MB, noise 8.0 + quality 30 -> %d PNG files on %d threads: %.2f s wall clock, %.0f ms per file (%.2f s with every '
                     'stage synchronised)' % (args.files, W, H, size / 1e6, len(written), args.workers, t_run, 1e3 * t_run / args.files, t_staged))
        lines.append('        per file, ms:   decode wait   upload  kernels  read-back   submit  encode wait')
        for t in times:
            lines.append('        %-12s %11.1f %8.2f %8.3f %10.2f %8.2f %12.1f' % (
                os.path.basename(t['file']), *(1e3 * t.get(k, 0.0) for k in ('decode', 'upload', 'kernels', 'readback', 'submit', 'encode_wait'))))
        dev_ms = statistics.median(1e3 * (t['upload'] + t['kernels'] + t['readback']) for t in times)
        # codec and the reference's host sequence on one thread
        path = os.path.join(src, '0001.png')
        t0 = time.perf_counter()
        a = imgio.decode_u8(path)
        t_dec = time.perf_counter() - t0
        res = np.array(Image.open(os.path.join(out, '0001.png')))
        t0 = time.perf_counter()
        png.save_host(res, os.path.join(root, 'enc.png'), 'rgb', add_corruptions.PNG_COMPRESSION)
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        noisy = np.clip(a + np.rint(np.random.normal(loc=0.0, scale=8.0, size=a.shape)), 0, 255).astype(np.uint8)   # utils.gaussian_noise
        t_noise = time.perf_counter() - t0
        t0 = time.perf_counter()
        pil_roundtrip(noisy, 30)
        t_jpg = time.perf_counter() - t0
        lines.append('codec   one thread: decode of one file %.0f ms, PNG encoding of its result at zlib level %d %.0f ms; upload + kernels + read-back %.2f ms per file (median), '
                     '%.2f %% of decode + encode' % (1e3 * t_dec, add_corruptions.PNG_COMPRESSION, 1e3 * t_enc, dev_ms, 100 * dev_ms / (1e3 * (t_dec + t_enc))))
        host = t_dec + t_noise + t_jpg + t_enc
        lines.append('host    the reference sequence on one thread per file: decode %.0f + numpy noise %.0f + PIL JPEG save / open %.0f + PNG encode %.0f = %.0f ms; with the two middle '
                     'stages on the device: %.0f + %.2f + %.0f = %.0f ms (%.2f x)' % (1e3 * t_dec, 1e3 * t_noise, 1e3 * t_jpg, 1e3 * t_enc, 1e3 * host, 1e3 * t_dec, dev_ms, 1e3 * t_enc,
                                                                                     1e3 * (t_dec + t_enc) + dev_ms, host / (t_dec + t_enc + 1e-3 * dev_ms)))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
