"""Wall clock of the two folder CLIs (dasr_amd.dsn_evaluate, dasr_amd.back_projection) end to end, and of the byte hand-off in front of the folder evaluator
(metrics.u8_planes, with and without the upload), for comparing two checkouts of the project: `--tree` names the checkout whose dasr_amd is imported (default:
this one), so the same script times a parent commit and a working tree, process by process, alternating.

Every process writes its own folders of PNG pairs first (a photograph-like ground truth, a result with a little noise and a colour cast, the LR image by PIL's
bicubic) and then runs each main(argv) --runs times in-process; one line per CLI and folder with the ms per pair of every run (the first run builds the LPIPS
network's code objects and is the warm-up).  Folders: 5 pairs of 1356 x 2040 with 6 decode threads, 40 pairs of 340 x 512 with 2.  The hand-off: 100 calls between
two device synchronisations on one 1356 x 2040 image, --runs times.

The drivers that write PNG files (`png ...` reports, on the 5-file folders only; `--only png` selects them): prepare_data --sub_dir --lr_dir --bic_dir and
add_corruptions (noise 8, JPEG 30) over the 1356 x 2040 ground-truth files, each with and without --device_png, and back_projection --device_png; ms per file.

The lines go to stdout and are appended to --out.  Nothing here is asserted by a test.

    python scripts/folder_cli_ab.py [--tree PATH] [--label NAME] [--runs 7] [--only TEXT] [--out profiles/eval_refactor_raw.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = [('5 pairs 1356x2040, 6 workers', 5, 1356, 2040, 6), ('40 pairs 340x512, 2 workers', 40, 340, 512, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(HERE))
    ap.add_argument('--label', default='tree')
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--only', default=None, help='time only the reports whose name contains this text, e.g. dsn_evaluate')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.tree)
    sys.path.insert(0, HERE)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from PIL import Image
    from dasr_amd import add_corruptions as A, back_projection as B, dsn_evaluate as E, imgio, metrics, prepare_data as P   # (first: evaluate_ab puts its own checkout in front of sys.path)
    from evaluate_ab import write_pair
    if not os.path.abspath(E.__file__).startswith(root + os.sep):
        raise SystemExit('dasr_amd was imported from %s, not from --tree %s' % (E.__file__, root))
    if not torch.cuda.is_available():
        raise SystemExit('folder_cli_ab.py needs the GPU')
    lines = []

    def timed(fn, per):
        ts = []
        for _ in range(a.runs):
            with contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) / per * 1e3)
        return ts

    def report(what, name, unit, fn, per):
        if a.only and a.only not in what:
            return
        ts = timed(fn, per)
        lines.append('%-8s %-28s %-30s %s: %s' % (a.label, what, name, unit, ' '.join('%.4g' % t for t in ts)))
        print(lines[-1], flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for k, (name, n, h, w, workers) in enumerate(CONFIGS):
            res, gt, lr, out = (os.path.join(tmp, '%s%d' % (d, k)) for d in ('res', 'gt', 'lr', 'out'))
            for d in (res, gt, lr):
                os.makedirs(d)
            for i in range(n):
                write_pair(res, gt, 'img_%02d.png' % i, h, w, 100 + i)
                Image.open(os.path.join(gt, 'img_%02d.png' % i)).resize((w // 4, h // 4), Image.BICUBIC).save(os.path.join(lr, 'img_%02d.png' % i))
            report('dsn_evaluate.main', name, 'ms per pair', lambda: E.main(
                ['--dir', res, '--gt_dir', gt, '--border_crop', '4', '--allow_random_perceptual', '--num_workers', str(workers)]), n)
            report('back_projection.main', name, 'ms per pair', lambda: B.main(
                ['--lr_dir', lr, '--sr_dir', res, '--out_dir', out, '--num_workers', str(workers)]), n)
            if k:
                continue
            for flag in ([], ['--device_png']):
                tag, sub = ' '.join(flag), os.path.join(out, 'png' + ''.join(flag))
                report(('png prepare_data ' + tag).strip(), name, 'ms per file', lambda: P.main(
                    ['--input_dir', gt, '--sub_dir', os.path.join(sub, 'sub'), '--lr_dir', os.path.join(sub, 'lr'), '--bic_dir', os.path.join(sub, 'bic'), '--overwrite',
                     '--num_workers', str(workers)] + flag), n)
                report(('png add_corruptions ' + tag).strip(), name, 'ms per file', lambda: A.main(
                    ['--input_dir', gt, '--output_dir', os.path.join(sub, 'noisy'), '--overwrite', '--num_workers', str(workers)] + flag), n)
            report('png back_projection --device_png', name, 'ms per file', lambda: B.main(
                ['--lr_dir', lr, '--sr_dir', res, '--out_dir', os.path.join(out, 'png_bp'), '--num_workers', str(workers), '--device_png']), n)
    dev = imgio.device_of(None)
    img = np.random.RandomState(0).randint(0, 256, size=(1356, 2040, 3)).astype(np.uint8)
    on_dev = torch.from_numpy(img).to(dev)
    report('metrics.u8_planes', 'device tensor 1356x2040', 'ms per call', lambda: [metrics.u8_planes(on_dev) for _ in range(100)], 100)
    report('upload + metrics.u8_planes', 'array 1356x2040', 'ms per call', lambda: [metrics.u8_planes(torch.from_numpy(img).to(dev)) for _ in range(100)], 100)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
