"""A/B of the evaluation drivers' image-quality step: the host sequence of dasr_amd/test.py against the device path (`device_metrics: true`).

For one SR / HR pair of fp32 device images at 480 x 500 (Set14 size) and 1356 x 2040 (DIV2K validation size), in ONE process:
  host    what test.evaluate does per image without the option: the two fp32 images copied to the CPU (get_current_visuals), util.tensor2img twice,
          calculate_psnr / calculate_ssim on RGB and, through bgr2ycbcr, on Y
  device  BaseModel.current_sr_u8() + BaseModel.current_metrics(crop): quantisation, squared-error sums and SSIM on csrc/metrics.hip, the uint8 SR image and one
          small result buffer copied back
Wall clock between two device synchronisations, one warm-up repetition excluded, median of --reps (the host side of the large size: --host-reps-large, one is
enough at tens of seconds).  The table (with the device, its clocks as the SMI tool reports them, the CPU count and the differences between the two paths'
numbers) goes to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/metrics_ab.py [--reps 5] [--host-reps-large 1] [--sizes 480x500,1356x2040] [--out profiles/metrics_ab.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _holder(sr, hr):
    """a trainer's state after feed_data + test(), without a network: BaseModel's device entry points only read fake_H and real_H"""
    from dasr_amd.models import BaseModel
    m = BaseModel.__new__(BaseModel)
    m.fake_H, m.real_H = sr, hr
    return m


def host_sequence(m, c):
    from dasr_amd import util
    sr_img = util.tensor2img(m.fake_H.detach()[0].float().cpu())
    gt_img = util.tensor2img(m.real_H.detach()[0].float().cpu()) / 255.
    sr_img = sr_img / 255.
    csr, cgt = sr_img[c:-c, c:-c, :], gt_img[c:-c, c:-c, :]
    out = {'psnr': util.calculate_psnr(csr * 255, cgt * 255), 'ssim': util.calculate_ssim(csr * 255, cgt * 255)}
    sr_y, gt_y = util.bgr2ycbcr(sr_img, only_y=True), util.bgr2ycbcr(gt_img, only_y=True)
    out['psnr_y'] = util.calculate_psnr(sr_y[c:-c, c:-c] * 255, gt_y[c:-c, c:-c] * 255)
    out['ssim_y'] = util.calculate_ssim(sr_y[c:-c, c:-c] * 255, gt_y[c:-c, c:-c] * 255)
    return out


def device_sequence(m, c):
    m.current_sr_u8()
    return m.current_metrics(c)


def timed(fn, reps):
    fn()   # warm-up: code objects, buffers, numpy's thread pool
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts), out


def clocks():
    try:
        p = subprocess.run(['rocm-smi', '--showclocks', '-d', '0'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=30)
        rows = [l.strip() for l in p.stdout.decode().splitlines() if 'sclk' in l or 'mclk' in l]
        return '; '.join(rows) or 'not reported'
    except (OSError, subprocess.SubprocessError):
        return 'not reported'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-reps-large', type=int, default=1)
    ap.add_argument('--sizes', default='480x500,1356x2040')
    ap.add_argument('--crop', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics_ab.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('metrics_ab.py needs the GPU: a CPU run says nothing about the device path')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    dev = torch.device('cuda')
    lines = ['image-quality step of the evaluation drivers, host sequence (dasr_amd/test.py without the option) vs device path (device_metrics: true)',
             'device: %s; clocks: %s' % (torch.cuda.get_device_name(0), clocks()),
             'host: %d CPUs available to the process, torch %s; wall clock between device synchronisations, 1 warm-up excluded, median [min, max] of the repetitions' % (
                 len(os.sched_getaffinity(0)), torch.__version__),
             '', '| image (H x W x 3) | host s (reps) | device ms (reps) | host / device | max abs difference of the four numbers |', '|---|---|---|---|---|']
    for size in a.sizes.split(','):
        h, w = (int(v) for v in size.split('x'))
        g = torch.Generator().manual_seed(h * w)
        hr = torch.rand(1, 3, h, w, generator=g)
        sr = (hr + 0.05 * torch.randn(1, 3, h, w, generator=g)).to(dev)
        m = _holder(sr, hr.to(dev))
        hreps = a.host_reps_large if h * w > 1000000 else a.reps
        hm, hlo, hhi, hv = timed(lambda: host_sequence(m, a.crop), hreps)
        dm, dlo, dhi, dv = timed(lambda: device_sequence(m, a.crop), a.reps)
        diff = max(abs(hv[k] - dv[k]) for k in hv)
        lines.append('| %d x %d | %.3f [%.3f, %.3f] (%d) | %.3f [%.3f, %.3f] (%d) | %.0fx | %.2e |' % (h, w, hm, hlo, hhi, hreps, dm * 1e3, dlo * 1e3, dhi * 1e3, a.reps,
                                                                                                      hm / dm, diff))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
