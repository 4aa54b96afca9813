"""Measurement of the iterative back-projection (`"back_projection"`, dasr_amd/backproject.py) in ONE process, at LR 339 x 510 -> SR 1356 x 2040 (a DIV2K validation image at
x4) and LR 128 x 128 -> SR 512 x 512, 20 iterations:

  device     backproject.back_project: dasr_bp_residual + dasr_bp_update per iteration; wall clock between two device synchronisations
  host       backproject.back_project_fp64, the only way to do it without these kernels (dense resampling matrices in float64 on the CPU); --host-iters iterations are
             timed and scaled to 20 (every iteration does the same work)
  test()     plain inference of RRDB_net nf 64 nb 23 at the same LR size (`chop` at 339 x 510), for scale
  kernels    every launch of 20 iterations inside a profiling session of the library (dasr_prof_begin / dasr_prof_end: the dispatch's own begin / end timestamps): launches
             per iteration, median time per kernel, algorithmic bytes (residual: read SR and LR, write d; update: read and write SR, read d) over that time against the
             6.3 TB/s a streaming kernel achieves from HBM on this device
  residual   dasr_bp_residual against what the library offered before it: dasr_imresize_down (two launches, an fp64 intermediate in device memory) and a torch
             subtraction; device events around --reps alternated repetitions, and the results compared bit for bit

The table goes to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/back_projection_ab.py [--reps 20] [--host-iters 20] [--nb 23] [--out profiles/back_projection.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s, streaming kernels on MI355X
ITERS = 20


def make_model(nb, chop):
    from dasr_amd import options
    from dasr_amd.init import kaiming_state_dict
    from dasr_amd.models import create_model
    from dasr_amd.rrdbnet import rrdbnet_param_spec
    opt = {'is_train': False, 'gpu_ids': [0], 'scale': 4, 'chop': chop, 'val_lpips': False, 'model': 'sr', 'path': {'pretrain_model_G': None},
           'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': nb, 'in_nc': 3, 'out_nc': 3, 'gc': 32, 'scale': 4}}
    m = create_model(options.dict_to_nonedict(opt))
    torch.manual_seed(0)
    m.netG.load_state_dict(kaiming_state_dict(rrdbnet_param_spec(3, 3, 64, nb, 'upconv'), 0.1))
    return m


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def fmt(ts, unit=1e3):
    med = statistics.median(ts)
    return 'median %9.3f  min %9.3f  max %9.3f  spread %5.1f %%' % (med * unit, min(ts) * unit, max(ts) * unit, 100 * (max(ts) - min(ts)) / med)


def profiled(fn, capacity=4096):
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


def down_and_subtract(sr, lr, s, tmp):
    """the residual as the library formed it before dasr_bp_residual: dasr_imresize_down, then a torch subtraction"""
    from dasr_amd import _lib
    from dasr_amd.imgio import tap_table
    _, c, H, W = sr.shape
    (jh, wh), (jw, ww) = tap_table(H, s, sr.device), tap_table(W, s, sr.device)
    out = torch.empty_like(lr)
    _lib.check(_lib.lib().dasr_imresize_down(sr.data_ptr(), c, H, W, s, jh.data_ptr(), wh.data_ptr(), jw.data_ptr(), ww.data_ptr(), tmp.data_ptr(), out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), 'dasr_imresize_down')
    return lr - out


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-iters', type=int, default=20)
    ap.add_argument('--nb', type=int, default=23)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: a timing taken anywhere else says nothing about it')
    from dasr_amd import backproject
    from dasr_amd.data import imresize_matlab
    dev, s = torch.device('cuda'), 4
    lines = ['# scripts/back_projection_ab.py --reps %d --host-iters %d --nb %d: %s, torch %s, %d host threads' % (
                 args.reps, args.host_iters, args.nb, torch.cuda.get_device_name(0), torch.__version__, torch.get_num_threads()),
             '# %d iterations, scale %d, 3 channels; wall clock between two device synchronisations unless a line says otherwise; spread = (max - min) / median' % (ITERS, s)]
    for (h, w), chop in (((339, 510), True), ((128, 128), False)):
        H, W = s * h, s * w
        g = torch.Generator().manual_seed(1)
        hr = torch.rand(3, H, W, generator=g)
        lr = imresize_matlab(hr, 1.0 / s)[None].contiguous()
        sr = (hr + 0.05 * torch.randn(hr.shape, generator=g))[None].contiguous()
        srd, lrd = sr.to(dev), lr.to(dev)
        lines.append('LR %d x %d -> SR %d x %d' % (h, w, H, W))
        # device
        for _ in range(3):
            out = backproject.back_project(srd, lrd, ITERS)
        t_dev = wall(lambda: backproject.back_project(srd, lrd, ITERS), args.reps)
        lines.append('  device  back_project, %d iterations           ms  %s' % (ITERS, fmt(t_dev)))
        # host
        t0 = time.perf_counter()
        ref = backproject.back_project_fp64(sr, lr, args.host_iters)
        t_host = (time.perf_counter() - t0) * ITERS / args.host_iters
        err = float((backproject.back_project(srd, lrd, args.host_iters).cpu().double() - ref).abs().max())
        lines.append('  host    back_project_fp64, scaled to %d from %d  s   %9.2f   (x %.0f of the device; max |device - host| after %d iterations %.2e)' % (
            ITERS, args.host_iters, t_host, t_host / statistics.median(t_dev), args.host_iters, err))
        # the generator at this size
        m = make_model(args.nb, chop)
        m.feed_data({'LR': lr}, False)
        for _ in range(3):
            m.test()
        t_test = wall(m.test, args.reps)
        lines.append('  test()  RRDB_net nb %d, chop %-5s              ms  %s   (back_project / test() = %.3f)' % (
            args.nb, chop, fmt(t_test), statistics.median(t_dev) / statistics.median(t_test)))
        del m
        torch.cuda.empty_cache()
        # kernels
        recs = profiled(lambda: backproject.back_project(srd, lrd, ITERS))
        lines.append('  launches per iteration: %.1f (%d launches of the library in %d iterations)' % (len(recs) / ITERS, len(recs), ITERS))
        traffic = {'bp_residual_kernel': 3 * (H * W + 2 * h * w) * 4, 'bp_update_kernel': 3 * (2 * H * W + h * w) * 4}
        for tag, nbytes in traffic.items():
            us = [u for t, u in recs if t == tag][1:]   # (the first launch left out: cold caches)
            med = statistics.median(us)
            rate = nbytes / (med * 1e-6)
            lines.append('  %-20s %7.2f MB  median %8.2f us (min %.2f, max %.2f, n %d)  %6.3f TB/s  %5.1f %% of 6.3 TB/s' % (
                tag, nbytes / 1e6, med, min(us), max(us), len(us), rate / 1e12, 100 * rate / HBM_ACHIEVABLE))
        lines.append('  kernel time of %d iterations %.3f ms of the %.3f ms wall clock' % (ITERS, sum(u for _, u in recs) * 1e-3, statistics.median(t_dev) * 1e3))
        # the residual: fused against imresize_down + subtraction
        tmp = torch.empty((3, h, W), dtype=torch.float64, device=dev)
        fused, parent = (lambda: backproject.residual(srd, lrd)), (lambda: down_and_subtract(srd, lrd, s, tmp))
        same = torch.equal(fused(), parent())
        for fn in (fused, parent):
            events(fn, 5)
        tf, tp = [], []
        for _ in range(5):   # alternated blocks of --reps launches between device events
            tf.append(events(fused, args.reps))
            tp.append(events(parent, args.reps))
        down = [u for t, u in profiled(parent) if 'imresize' in t]
        lines.append('  residual, device events around %d calls, us per call: dasr_bp_residual %s' % (args.reps, fmt(tf, 1e6)))
        lines.append('                                   dasr_imresize_down + torch subtraction %s' % fmt(tp, 1e6))
        lines.append('  (bit-equal: %s; the two imresize_down kernels alone: %.2f us; fused / parent = %.2f)' % (same, sum(down), statistics.median(tf) / statistics.median(tp)))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
