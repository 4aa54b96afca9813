"""Score a folder of result images against a folder of ground truth: PSNR, PSNR of the mean colour, SSIM in scikit-image's form and LPIPS(alex) --
codes/DSN/evaluate.py on the MI355X.

    python -m dasr_amd.dsn_evaluate --dir results/ --gt_dir gt/ [--border_crop 4] --lpips_alexnet alexnet.pth --lpips_lin alex.pth [--num_workers 6]

The files are decoded on host threads (PIL, imgio.decode_ahead), the BYTES are uploaded, and everything per pixel runs on the device: the planar re-layout
(metrics.u8_planes: imgio.planar_f32, dasr_tensor2img_u8), the squared-error and channel sums, the 7 x 7 box SSIM (csrc/metrics.hip) and LPIPS on byte / 255 at any image
size from 31 x 31 (LPIPSAlexHIP.distance; dasr_lpips_s2d_any where a side is no multiple of 4).  One read-back per pair brings the integer and fp64 result
words to the host, where the two PSNRs are formed in double (dasr_amd/metrics.py pair_metrics_u8).

Semantics of evaluate.py:25-57: both folders listed with the project's image-file test, sorted, paired by index (a basename mismatch prints the reference's
warning); the result loses an alpha channel; a larger ground truth is cut to the result's rows and columns from the top-left; --border_crop pixels leave
every side of both.  Deliberate deviation: unequal file counts are a ValueError (the reference zips the two lists and then divides by the longer count,
which gives a wrong average).  The LPIPS weights come from --lpips_alexnet / --lpips_lin as in dsn_train; without them --allow_random_perceptual seeds the
network and every LPIPS value is labelled LPIPS(random)."""
import argparse
import os

import torch

from . import imgio
from .dsn_data import is_image_file

SSIM_MIN, LPIPS_MIN = 7, 31   # smallest side of the scored region: the SSIM window; what the LPIPS backbone needs (lpips.MIN_SIDE)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Score a folder of images against its ground truth: PSNR, PSNR_col, SSIM, LPIPS')
    p.add_argument('--dir', required=True, type=str, help='directory of the images that are being tested')
    p.add_argument('--gt_dir', required=True, type=str, help='directory of the gt images')
    p.add_argument('--border_crop', default=None, type=int, help='number of pixels to remove at the border')
    p.add_argument('--lpips_alexnet', default=None, type=str, help='torchvision alexnet state_dict')
    p.add_argument('--lpips_lin', default=None, type=str, help="the reference's codes/PerceptualSimilarity/models/weights/v0.1/alex.pth")
    p.add_argument('--allow_random_perceptual', action='store_true',
                   help='without the weight files: score against a seeded random network; the value is labelled LPIPS(random) and is not the LPIPS metric')
    p.add_argument('--num_workers', default=6, type=int, help='decode threads (at most %d)' % imgio.MAX_DECODE_THREADS)
    return p.parse_args(argv)


def list_pairs(result_dir, gt_dir):
    """[(result file, ground-truth file)]: both folders sorted and paired by index; unequal counts are a ValueError"""
    files = sorted(os.path.join(result_dir, x) for x in os.listdir(result_dir) if is_image_file(x))
    gt_files = sorted(os.path.join(gt_dir, x) for x in os.listdir(gt_dir) if is_image_file(x))
    if len(files) != len(gt_files):
        raise ValueError('%s holds %d image files, %s holds %d: the folders must pair up file by file' % (result_dir, len(files), gt_dir, len(gt_files)))
    if not files:
        raise ValueError('%s holds no image files' % result_dir)
    return list(zip(files, gt_files))


def load_pair(file, gt_file, border=0, lpips=True):
    """the two decoded images as evaluate.py:35-40 pairs them, uint8 [H, W, 3] of ONE size: the result without its alpha channel, the ground truth cut to the
    result's rows and columns from the top-left.  The border is NOT removed here (the kernels take it as their crop) but the region it leaves is checked.
    ValueError: a file that is not 8-bit RGB (RGBA is accepted on the result side), a ground truth smaller than its result on either axis, a region under
    7 x 7 (31 x 31 with `lpips`)."""
    h, w, mode = imgio.image_header(file)
    if mode not in ('RGB', 'RGBA'):
        raise ValueError('%s: mode %s, expected an 8-bit RGB or RGBA image' % (file, mode))
    gh, gw, gmode = imgio.image_header(gt_file)
    if gmode != 'RGB':
        raise ValueError('%s: mode %s, expected an 8-bit RGB image' % (gt_file, gmode))
    if gh < h or gw < w:
        raise ValueError('%s (%d x %d) is smaller than its result %s (%d x %d)' % (gt_file, gh, gw, file, h, w))
    need = LPIPS_MIN if lpips else SSIM_MIN
    if border < 0 or h - 2 * border < need or w - 2 * border < need:
        raise ValueError('%s: %d x %d with --border_crop %d leaves %d x %d, under the %d x %d that %s needs' % (
            file, h, w, border, h - 2 * border, w - 2 * border, need, need, 'LPIPS' if lpips else 'the SSIM window'))
    img = imgio.decode_u8(file)   # (convert('RGB') of an RGBA file drops the alpha channel: [..., :3])
    gt = imgio.decode_u8(gt_file, None if (gh, gw) == (h, w) else (0, 0, w, h))
    return img, gt


def score_pair(net, img, gt, border, device):
    """the four numbers of one decoded pair (load_pair), all per-pixel work on the device, one read-back"""
    from . import metrics
    h, w = img.shape[:2]
    fa, ua = metrics.u8_planes(torch.from_numpy(img).to(device))
    fb, ub = metrics.u8_planes(torch.from_numpy(gt).to(device))
    region = (slice(None), slice(border, h - border), slice(border, w - border))
    d = net.distance(fa[region][None], fb[region][None])   # on byte / 255: distance folds the 2x - 1 of normalize=True
    return metrics.pair_metrics_u8(ua, ub, border=border, lpips=d)


def main(argv=None):
    """returns {'psnr', 'psnr_col', 'ssim', 'lpips': the averages, 'lpips_label', 'files': one dict per pair}"""
    o = parse_args(argv)
    from .lpips import load_lpips, lpips_label
    border = int(o.border_crop) if o.border_crop is not None and o.border_crop > 0 else 0
    pairs = list_pairs(o.dir, o.gt_dir)
    device = imgio.device_of(None)
    net = load_lpips({'path': {'lpips_alexnet': o.lpips_alexnet, 'lpips_lin': o.lpips_lin}, 'allow_random_perceptual': o.allow_random_perceptual}, device)
    label = lpips_label(net)
    rows, keys = [], ('psnr', 'psnr_col', 'ssim', 'lpips')
    for (img, gt), (file, gt_file) in zip(imgio.decode_ahead(lambda f, g: load_pair(f, g, border), pairs, o.num_workers), pairs):
        if os.path.basename(file) != os.path.basename(gt_file):
            print('WARNING: file and gt_file do not have the same name')
        m = score_pair(net, img, gt, border, device)
        rows.append(dict(m, file=file, gt_file=gt_file))
        print('%s: PSNR %s PSNR_col %s SSIM %s %s %s' % (os.path.basename(file), m['psnr'], m['psnr_col'], m['ssim'], label, m['lpips']))
    out = {k: sum(r[k] for r in rows) / len(rows) for k in keys}
    print('PSNR: ' + str(out['psnr']))
    print('PSNR_col: ' + str(out['psnr_col']))
    print('SSIM: ' + str(out['ssim']))
    print(label + ': ' + str(out['lpips']))
    out.update(lpips_label=label, files=rows)
    return out


if __name__ == '__main__':
    main()
