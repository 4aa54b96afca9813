"""A/B of the folder evaluator (python -m dasr_amd.dsn_evaluate) against a host restatement of codes/DSN/evaluate.py on the same synthetic folder of
DIV2K-sized PNG pairs (1356 x 2040), in ONE process, pair by pair, alternating.

  device  decode on the host (PIL), upload of the bytes, dasr_u8_to_planar + dasr_tensor2img_u8, then PSNR / PSNR_col / SSIM (dasr_img_sse,
          dasr_img_channel_sums, dasr_img_ssim_box; one read-back) and LPIPS (LPIPSAlexHIP.distance), each stage closed by a device synchronisation
  host    the same decoded arrays: PSNR and PSNR_col with numpy in double, SSIM in scikit-image's form restated with scipy.ndimage.uniform_filter in fp64
          (scikit-image itself is not installed), LPIPS on oracle.lpips with torch on the CPU
The LPIPS network is the seeded one of --allow_random_perceptual on both sides (the pretrained files cannot be fetched): the column is LPIPS(random).

Then the whole CLI over the folder (wall clock per pair, decode threads as given), and the box-SSIM entry point alone under device events: achieved bytes
per second -- the bytes of the two images over the time of its two launches -- against the 6.3 TB/s the project uses as the achievable HBM rate.

The tables go to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/evaluate_ab.py [--pairs 4] [--size 1356x2040] [--border_crop 4] [--reps 20] [--out profiles/evaluate_ab.txt]
"""
import argparse
import contextlib
import io
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

HBM_ACHIEVABLE = 6.3e12


def write_pair(res_dir, gt_dir, name, h, w, seed):
    """a photograph-like ground truth (smooth field + noise) and a result that differs from it by a little noise and a colour cast"""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, h // 16 + 2, w // 16 + 2, generator=g), size=(h, w), mode='bilinear', align_corners=False)[0]
    gt = (base + 0.03 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    res = (gt + 0.02 * torch.randn(3, h, w, generator=g) + torch.tensor([0.01, -0.005, 0.008]).view(3, 1, 1)).clamp(0, 1)
    for folder, img in ((gt_dir, gt), (res_dir, res)):
        Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(os.path.join(folder, name))


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def host_ssim(img, gt):
    """compare_ssim(img, gt, multichannel=True) on uint8 HWC arrays, restated: uniform_filter 7, sample covariance, data range 255, interior region"""
    from scipy.ndimage import uniform_filter
    cov_norm, C1, C2 = 49.0 / 48.0, (0.01 * 255) ** 2, (0.03 * 255) ** 2
    means = []
    for c in range(img.shape[2]):
        x, y = img[..., c].astype(np.float64), gt[..., c].astype(np.float64)
        ux, uy, uxx, uyy, uxy = (uniform_filter(v, size=7) for v in (x, y, x * x, y * y, x * y))
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        means.append(S[3:-3, 3:-3].mean())
    return float(np.mean(means))


def host_numbers(img, gt, crit):
    t0 = time.perf_counter()
    psnr = 10 * np.log10(255.0 ** 2 / np.mean((img.astype(np.float64) - gt.astype(np.float64)) ** 2))
    va, vb = img.mean(1).mean(0) / 255., gt.mean(1).mean(0) / 255.
    col = 10 * np.log10(1.0 / np.mean((va - vb) ** 2))
    t1 = time.perf_counter()
    ssim = host_ssim(img, gt)
    t2 = time.perf_counter()
    ti, tg = (torch.from_numpy(np.ascontiguousarray(v)).permute(2, 0, 1)[None].float() / 255. for v in (img, gt))
    with torch.no_grad():
        lp = float(crit(ti, tg))
    t3 = time.perf_counter()
    return dict(psnr=float(psnr), psnr_col=float(col), ssim=ssim, lpips=lp), dict(psnr=t1 - t0, ssim=t2 - t1, lpips=t3 - t2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=4)
    ap.add_argument('--size', default='1356x2040')
    ap.add_argument('--border_crop', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--num_workers', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'evaluate_ab.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('evaluate_ab.py needs the GPU: a CPU run says nothing about the device path')
    from dasr_amd import _lib, dsn_evaluate as E, imgio, metrics
    from dasr_amd.lpips import load_lpips, lpips_label, lpips_random_state_dict
    from oracle import lpips as olpips
    h, w = (int(v) for v in a.size.split('x'))
    b = a.border_crop
    dev = imgio.device_of(None)
    net = load_lpips({'path': {'lpips_alexnet': None, 'lpips_lin': None}, 'allow_random_perceptual': True}, dev)
    sd = lpips_random_state_dict(77)
    feats = olpips.alexnet_features()
    feats.load_state_dict({k[len('features.'):]: v for k, v in sd.items() if k.startswith('features.')})
    crit = olpips.PerceptualLossLPIPS(olpips.LPIPSAlex(feats, [sd['lin%d.model.1.weight' % i].reshape(-1) for i in range(5)]))
    lines = ['folder evaluator (dasr_amd.dsn_evaluate: csrc/metrics.hip box SSIM + channel sums, dasr_lpips_s2d_any) against a host restatement of codes/DSN/evaluate.py',
             'device: %s; host: %d CPUs available to the process, torch %s, numpy %s' % (torch.cuda.get_device_name(0), len(os.sched_getaffinity(0)), torch.__version__,
                                                                                       np.__version__),
             '%d pairs of %d x %d PNGs (RGB), --border_crop %d, LPIPS network: %s; wall clock, every device stage closed by a synchronisation; pair 0 is the warm-up '
             '(code objects, the LPIPS plan of this size) and is left out of the medians' % (a.pairs, h, w, b, lpips_label(net)), '']
    with tempfile.TemporaryDirectory() as tmp:
        res_dir, gt_dir = os.path.join(tmp, 'res'), os.path.join(tmp, 'gt')
        os.makedirs(res_dir)
        os.makedirs(gt_dir)
        for i in range(a.pairs + 1):
            write_pair(res_dir, gt_dir, 'img_%02d.png' % i, h, w, 100 + i)
        pairs = E.list_pairs(res_dir, gt_dir)
        lines += ['## per pair, ms', '',
                  '| pair | decode (both files, one thread) | device: upload + planar re-layout | device: PSNR, PSNR_col, SSIM (4 entry points, one read-back) | device: LPIPS | '
                  'host: PSNR, PSNR_col | host: SSIM (uniform_filter, fp64) | host: LPIPS (torch, CPU) |', '|---|---|---|---|---|---|---|---|']
        numbers, cols = [], []
        region = (slice(None), slice(b, h - b), slice(b, w - b))
        for i, (f, g) in enumerate(pairs):
            (img, gt), t_dec = clock(lambda: E.load_pair(f, g, b))
            planes, t_up = clock(lambda: (metrics.u8_planes(torch.from_numpy(img).to(dev)), metrics.u8_planes(torch.from_numpy(gt).to(dev))))
            (fa, ua), (fb, ub) = planes
            m, t_met = clock(lambda: metrics.pair_metrics_u8(ua, ub, border=b))
            d, t_lp = clock(lambda: float(net.distance(fa[region][None], fb[region][None])))
            hn, ht = host_numbers(img[b:h - b, b:w - b], gt[b:h - b, b:w - b], crit)
            row = [t_dec, t_up, t_met, t_lp, ht['psnr'], ht['ssim'], ht['lpips']]
            lines.append('| %d%s | %s |' % (i, ' (warm-up)' if i == 0 else '', ' | '.join('%.2f' % (v * 1e3) for v in row)))
            if i:
                cols.append(row)
            numbers.append((dict(m, lpips=d), hn))
        med = [statistics.median(c) for c in zip(*cols)]
        lines.append('| median of pairs 1.. | %s |' % ' | '.join('%.2f' % (v * 1e3) for v in med))
        dev_sum, host_sum = sum(med[1:4]), sum(med[4:7])
        lines += ['', 'per pair behind the decode: device %.2f ms, host %.2f ms (%.1fx); with the decode: device %.2f ms, host %.2f ms (%.2fx).  The decode is %.0f %% of the '
                  'device sequence%s.' % (dev_sum * 1e3, host_sum * 1e3, host_sum / dev_sum, (med[0] + dev_sum) * 1e3, (med[0] + host_sum) * 1e3,
                                          (med[0] + host_sum) / (med[0] + dev_sum), 100 * med[0] / (med[0] + dev_sum),
                                          ': it dominates the wall time of a pair' if med[0] > dev_sum else ''), '']
        lines += ['## the four numbers, device | host restatement', '', '| pair | PSNR | PSNR_col | SSIM | %s |' % lpips_label(net), '|---|---|---|---|---|']
        for i, (dn, hn) in enumerate(numbers):
            lines.append('| %d | %s |' % (i, ' | '.join('%.12g / %.12g' % (dn[k], hn[k]) for k in ('psnr', 'psnr_col', 'ssim', 'lpips'))))
        worst = {k: max(abs(dn[k] - hn[k]) / (abs(hn[k]) if k == 'lpips' else 1.0) for dn, hn in numbers) for k in ('psnr', 'psnr_col', 'ssim', 'lpips')}
        lines += ['', 'worst difference: PSNR %.2e dB, PSNR_col %.2e dB, SSIM %.2e, LPIPS %.2e relative' % (worst['psnr'], worst['psnr_col'], worst['ssim'], worst['lpips']), '']
        # the whole CLI, decode threads and all
        argv = ['--dir', res_dir, '--gt_dir', gt_dir, '--border_crop', str(b), '--allow_random_perceptual', '--num_workers', str(a.num_workers)]
        with contextlib.redirect_stdout(io.StringIO()):
            E.main(argv)   # warm-up
            out, t_cli = clock(lambda: E.main(argv))
        lines += ['## the whole CLI over the folder (%d pairs, --num_workers %d, second run)' % (len(pairs), a.num_workers), '',
                  '%.2f ms per pair wall clock (network construction and weight packing included: %.1f ms for the run); PSNR %.6f PSNR_col %.6f SSIM %.9f %s %.6f' % (
                      t_cli / len(pairs) * 1e3, t_cli * 1e3, out['psnr'], out['psnr_col'], out['ssim'], out['lpips_label'], out['lpips']), '']
        # the box-SSIM entry point alone
        L = _lib.lib()
        nbytes = L.dasr_img_ws_bytes(1, 3, h, w, b)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        res = torch.zeros(1, dtype=torch.float64, device=dev)
        call = lambda: _lib.check(L.dasr_img_ssim_box(ua.data_ptr(), ub.data_ptr(), 1, 3, h, w, b, res.data_ptr(), ws.data_ptr(), nbytes, None), 'dasr_img_ssim_box')
        for _ in range(3):
            call()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        t = statistics.median(ts)
        moved = 2 * 3 * (h - 2 * b) * (w - 2 * b)
        lines += ['## dasr_img_ssim_box alone (device events around its two launches, median [min, max] of %d)' % a.reps, '',
                  '%.1f us [%.1f, %.1f] for 2 x 3 x %d x %d bytes = %.2f MB: %.1f GB/s = %.2f %% of the %.1f TB/s achievable HBM rate (the inputs of one pair fit the '
                  'Infinity Cache and are resident there when the call repeats: the figure is the rate of the kernel, not a measurement of HBM)' % (
                      t * 1e6, min(ts) * 1e6, max(ts) * 1e6, h - 2 * b, w - 2 * b, moved / 1e6, moved / t / 1e9, 100 * moved / t / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12), '']
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
