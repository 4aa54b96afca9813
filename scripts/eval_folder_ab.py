"""A/B of the input stage of the evaluation datasets (`mode: "LRHR"` without an LR folder) and the per-image breakdown of one evaluation run over a folder.

Part 1, per image file at 480 x 500 (Set14 size) and 1356 x 2040 (DIV2K validation size), in ONE process, the PNG written to a temporary folder first:
  host    load_image (PIL decode, fp32 conversion, planar re-layout), crop to a multiple of the scale, imresize_matlab (two dense fp64 matrices), upload of the two
          fp32 images
  device  data.EvalFolderDataset.item: PIL decode, upload of the BYTES, dasr_u8_to_planar (with the crop), dasr_imresize_down (tap tables uploaded once per size)
The PNG decode is common to both and is also timed alone, so the table gives the ratio of the two sequences with it and with its median subtracted from both.  Wall clock between two device synchronisations,
one warm-up repetition excluded, median [min, max] of --reps.

Part 2: one evaluation run (model sr, RRDB_net nf 64 nb 23, seeded weights, device_metrics) over a folder with three distinct image sizes, two files of each, with the
steps of test.evaluate timed one by one: decode, input stage, the forward pass (the FIRST image of a size builds the inference plan for that size: its forward time
minus the time of the same forward repeated is reported as plan construction), metrics, PNG write.

The tables (with the device, its clocks as the SMI tool reports them and the CPU count) go to stdout and to --out.  Nothing here is asserted by a test.

    python scripts/eval_folder_ab.py [--reps 5] [--sizes 480x500,1356x2040] [--out profiles/eval_folder.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def write_png(path, h, w, seed):
    """a photograph-like 8-bit image (smooth field + noise): PNG decode time depends on the content"""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.rand(1, 3, h // 16 + 2, w // 16 + 2, generator=g), size=(h, w), mode='bilinear', align_corners=False)[0]
    img = (base + 0.03 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    Image.fromarray((img.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()).save(path)


def timed(fn, reps):
    fn()   # warm-up: code objects, buffers, tap tables, numpy's thread pool
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


def host_sequence(path, scale, dev):
    from dasr_amd.data import imresize_matlab, load_image, modcrop_size
    hr = load_image(path)
    Hc, Wc = modcrop_size(hr.shape[1], hr.shape[2], scale)
    hr = hr[:, :Hc, :Wc].contiguous()
    lr = imresize_matlab(hr, 1.0 / scale)
    return lr[None].to(dev), hr[None].to(dev)


def fmt(t):
    return '%.2f [%.2f, %.2f]' % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)


def part1(a, dev, tmp, lines):
    from dasr_amd.data import EvalFolderDataset
    lines += ['## input stage per image file: host sequence vs device sequence (scale %d, times in ms: median [min, max] of %d)' % (a.scale, a.reps), '',
              '| image (H x W x 3) | PNG decode alone | host: load_image, crop, imresize_matlab, 2 fp32 uploads | device: decode, byte upload, u8_to_planar, imresize_down | '
              'host / device | host / device without the decode | max abs LR difference | HR bit-equal |', '|---|---|---|---|---|---|---|---|']
    for k, size in enumerate(a.sizes.split(',')):
        h, w = (int(v) for v in size.split('x'))
        folder = os.path.join(tmp, 'hr_%d' % k)
        os.makedirs(folder)
        path = os.path.join(folder, 'img.png')
        write_png(path, h, w, h * w)
        ds = EvalFolderDataset({'mode': 'LRHR', 'dataroot_HR': folder, 'dataroot_LR': None, 'phase': 'test'}, a.scale, device=dev)
        dec = timed(lambda: ds.decode(path), a.reps)
        host = timed(lambda: host_sequence(path, a.scale, dev), a.reps)
        devt = timed(lambda: ds.item(0), a.reps)
        (hlr, hhr), item = host[3], devt[3]
        diff = float((hlr.double() - item['LR'].double()).abs().max())
        same = bool(torch.equal(hhr, item['HR']))
        lines.append('| %d x %d | %s | %s | %s | %.1fx | %.1fx | %.2e | %s |' % (h, w, fmt(dec), fmt(host), fmt(devt), host[0] / devt[0],
                                                                                (host[0] - dec[0]) / max(devt[0] - dec[0], 1e-9), diff, same))
    lines.append('')


def part2(a, dev, tmp, lines):
    from dasr_amd import options, util
    from dasr_amd.data import EvalFolderDataset
    from dasr_amd.models import create_model
    folder, out_dir = os.path.join(tmp, 'run_hr'), os.path.join(tmp, 'run_out')
    os.makedirs(folder)
    os.makedirs(out_dir)
    sizes = [(480, 500), (339, 510), (256, 256)]
    for i, (h, w) in enumerate(sizes * 2):      # two files of every size, each size seen first once
        write_png(os.path.join(folder, 'img_%02d.png' % i), h, w, 50 + i)
    opt = options.dict_to_nonedict({
        'name': 'eval_folder_ab', 'model': 'sr', 'scale': a.scale, 'gpu_ids': [0], 'is_train': False, 'chop': False, 'val_lpips': False, 'device_metrics': True,
        'path': {'root': tmp, 'pretrain_model_G': None, 'results_root': out_dir, 'log': out_dir},
        'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': 23, 'in_nc': 3, 'out_nc': 3, 'gc': 32, 'scale': a.scale}})
    model = create_model(opt)
    torch.manual_seed(0)     # seeded weights, drawn like the training driver's initialisation (the timings do not depend on the values)
    from dasr_amd.init import kaiming_state_dict
    from dasr_amd.rrdbnet import rrdbnet_param_spec
    model.netG.load_state_dict(kaiming_state_dict(rrdbnet_param_spec(3, 3, 64, 23, 'upconv'), 0.1))
    ds = EvalFolderDataset({'mode': 'LRHR', 'dataroot_HR': folder, 'dataroot_LR': None, 'phase': 'test'}, a.scale, device=dev)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    lines += ['## one evaluation run over a folder with three image sizes (model sr, RRDB_net nf 64 nb 23, scale %d, device_metrics; ms per image, in file order)' % a.scale, '',
              '| file | HR after the crop | decode | input stage | forward, first call | forward, repeated | plan construction (first - repeated) | metrics | PNG write |',
              '|---|---|---|---|---|---|---|---|---|']
    tot = [0.0] * 7
    for i, path in enumerate(ds.paths_HR):
        arr, t_dec = clock(lambda: ds.decode(path))

        def stage():
            hr = ds.to_device(arr, a.scale, path)
            return {'LR': ds.downsample(hr), 'HR': hr, 'LR_path': [path], 'HR_path': [path]}
        data, t_in = clock(stage)
        model.feed_data(data, False)
        _, t_f1 = clock(model.test)
        _, t_f2 = clock(model.test)
        (sr_img, m), t_met = clock(lambda: (model.current_sr_u8(), model.current_metrics(a.scale)))
        _, t_png = clock(lambda: util.save_img(sr_img, os.path.join(out_dir, 'img_%02d.png' % i)))
        row = [t_dec, t_in, t_f1, t_f2, max(t_f1 - t_f2, 0.0), t_met, t_png]
        tot = [x + y for x, y in zip(tot, row)]
        lines.append('| %s | %d x %d | %s |' % (os.path.basename(path), data['HR'].shape[2], data['HR'].shape[3], ' | '.join('%.2f' % (v * 1e3) for v in row)))
    lines.append('| sum | | %s |' % ' | '.join('%.2f' % (v * 1e3) for v in tot))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('--sizes', default='480x500,1356x2040')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_folder.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_folder_ab.py needs the GPU: a CPU run says nothing about the device path')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = ['input stage of the evaluation datasets (data.EvalFolderDataset, csrc/imgio.hip) against the host sequence, and the per-image breakdown of one evaluation run',
             'device: %s; clocks: %s' % (torch.cuda.get_device_name(0), clocks()),
             'host: %d CPUs available to the process, torch %s, numpy %s; wall clock between device synchronisations, 1 warm-up excluded in part 1, none in part 2' % (
                 len(os.sched_getaffinity(0)), torch.__version__, np.__version__), '']
    with tempfile.TemporaryDirectory() as tmp:
        part1(a, dev, tmp, lines)
        part2(a, dev, tmp, lines)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
