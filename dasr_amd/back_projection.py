"""Back-project a folder of SR images onto their LR images -- codes/SRN/scripts/back_projection/main_bp.m on the MI355X.

    python -m dasr_amd.back_projection --lr_dir LR --sr_dir results --out_dir results_20bp [--iters 20] [--num_workers 6] [--reverse_filter] [--device_png]

Every PNG file of --sr_dir is paired with the file of the same name in --lr_dir (main_bp.m:14-16).  The files are decoded on host threads (PIL, imgio.decode_ahead), the BYTES are
uploaded, and everything per pixel runs on the device: byte / 255 as planar fp32 (imgio.planar_f32: dasr_u8_to_planar, MATLAB's im2double), `iters` iterations of
backprojection.m (backproject.back_project), the clamp and rounding to bytes (metrics.tensor2img_device, MATLAB's imwrite of a double image).  The result is
written as PNG under the same name in --out_dir (png.FileWriter: by default the bytes are read back and PIL encodes them on the main thread).  Accepted input is 8-bit RGB; a missing partner or an SR size that is not 2, 3 or 4 times the LR size is a
ValueError naming both files.  With --device_png the bytes are not read back: the device encodes the file (png.FileWriter in device mode, fmt 'bgr'; --num_workers host threads add
the container and the checksums), the pixels are those of the default path.  With --reverse_filter the iterations are those of main_reverse_filter.m:18-22 (backproject.reverse_filter) instead, everything else
as above."""
import argparse
import os

from . import imgio, png, util
from .backproject import DEFAULT_ITERS, SCALES, back_project, reverse_filter


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Iterative back-projection of a folder of SR images onto their LR images')
    p.add_argument('--lr_dir', required=True, type=str, help='directory of the LR images')
    p.add_argument('--sr_dir', required=True, type=str, help='directory of the SR images (the pre-output)')
    p.add_argument('--out_dir', required=True, type=str, help='directory the back-projected images are written to')
    p.add_argument('--iters', default=DEFAULT_ITERS, type=int, help='iterations (main_bp.m: 20)')
    p.add_argument('--num_workers', default=6, type=int, help='decode threads (at most %d)' % imgio.MAX_DECODE_THREADS)
    p.add_argument('--reverse_filter', action='store_true', help='run the reverse filter (main_reverse_filter.m) in place of the back-projection')
    p.add_argument('--device_png', action='store_true', help='encode the PNG files on the device (png.FileWriter in device mode) instead of with PIL on the main thread')
    return p.parse_args(argv)


def list_pairs(sr_dir, lr_dir):
    """[(SR file, LR file, scale)]: the PNG files of sr_dir (main_bp.m:6), sorted, each with the file of the same name in lr_dir.  Checked on the file headers, before anything is
    decoded: ValueError for a missing partner, a file that is not 8-bit RGB, or an SR size that is not s x the LR size for one s in {2, 3, 4}"""
    names = sorted(x for x in os.listdir(sr_dir) if x.lower().endswith('.png'))   # main_bp.m:6 dir(fullfile(preout_folder, '*.png'))
    if not names:
        raise ValueError('%s holds no PNG files' % sr_dir)
    pairs = []
    for name in names:
        sr_file, lr_file = os.path.join(sr_dir, name), os.path.join(lr_dir, name)
        if not os.path.isfile(lr_file):
            raise ValueError('%s has no LR partner: %s does not exist' % (sr_file, lr_file))
        (H, W, mode), (h, w, lmode) = imgio.image_header(sr_file), imgio.image_header(lr_file)
        for f, m in ((sr_file, mode), (lr_file, lmode)):
            if m != 'RGB':
                raise ValueError('%s: mode %s, expected an 8-bit RGB image (its partner: %s)' % (f, m, lr_file if f == sr_file else sr_file))
        if H % h or W % w or H // h != W // w or H // h not in SCALES:
            raise ValueError('%s is %d x %d, which is not 2, 3 or 4 times the %d x %d of its LR image %s' % (sr_file, H, W, h, w, lr_file))
        pairs.append((sr_file, lr_file, H // h))
    return pairs


def main(argv=None):
    """returns the list of written paths, in the order of the sorted file names"""
    from . import metrics
    o = parse_args(argv)
    if o.iters < 0:
        raise ValueError('--iters must be >= 0, got %d' % o.iters)
    pairs = list_pairs(o.sr_dir, o.lr_dir)
    device = imgio.device_of(None)
    util.mkdir(o.out_dir)
    project = reverse_filter if o.reverse_filter else back_project

    def load(sr_file, lr_file, _s):
        return imgio.decode_u8(sr_file), imgio.decode_u8(lr_file)
    # without --device_png the bytes are read back and encoded by PIL on this thread, inside write()
    with png.FileWriter(o.device_png, o.num_workers if o.device_png else 0) as writer:
        for (sr_u8, lr_u8), (sr_file, _lr_file, _s) in zip(imgio.decode_ahead(load, pairs, o.num_workers), pairs):
            out = project(imgio.planar_f32(sr_u8, device, batch=True), imgio.planar_f32(lr_u8, device, batch=True), o.iters)
            writer.write(metrics.tensor2img_device(out), os.path.join(o.out_dir, os.path.basename(sr_file)), 'bgr')   # HWC BGR bytes, as util.tensor2img gives them
            print(os.path.basename(sr_file))
    return writer.paths


if __name__ == '__main__':
    main()
