"""Prepare the training folders of the SRN option files from a folder of HR images -- codes/SRN/scripts/extract_subimgs_single.py and generate_mod_LR_bic.m (MATLAB only)
in one pass over the files, on the MI355X (codes/SRN/data/README.md:26-27: DIV2K800 -> DIV2K800_sub, DIV2K800_sub_bicLRx4).

    python -m dasr_amd.prepare_data --input_dir HR [--sub_dir D --crop_sz 480 --step 240 --thres_sz 48] [--mod_dir D] [--lr_dir D] [--bic_dir D] [--scale 4]
                                    [--num_workers 6] [--overwrite] [--device_png]

Every PNG file of --input_dir is decoded once on host threads (PIL, imgio.decode_ahead) and its BYTES are uploaded once.  With --sub_dir the units are the sub-images of
extract_subimgs_single.py:62-83 (window_grid; written to --sub_dir as name_s001.png, ... in row-major order), without it the whole images.  Every unit is mod-cropped to a
multiple of --scale, then --mod_dir gets name.png (the mod-cropped bytes), --lr_dir name_bicLRx{s}.png (MATLAB's imresize(., 1 / s) of the unit, written as imwrite
writes a double image) and --bic_dir name_bicx{s}.png (imresize(., s) of the DOUBLE LR image).  The sub and mod files are byte copies, slices of the decoded array; the LR images of
all units of a file are ONE dasr_windows_down_u8 launch, their Bic images ONE dasr_imresize_up launch (bicubic.py), one read-back per file and product; the PNG files
are encoded on the host threads of a png.FileWriter (zlib level 3, as extract_subimgs_single.py:19 sets it: the pixels do not depend on it), at most two files' worth of
products outstanding.  With --device_png all products of a file are one write_many of that writer, ONE png.write_batch (sub and mod as windows of the uploaded image): no read-back of raw bytes, no PIL encode; the host threads add the
container and the checksums.  It needs --lr_dir or --bic_dir (without them no device is opened).  The mirror edge of the resampling
is the unit's edge: a file of --lr_dir is what MATLAB makes of the file of --sub_dir, not a crop of the whole image's LR image.

Accepted input is 8-bit RGB.  A grey, palette or alpha file, a file smaller than --crop_sz (the reference script raises IndexError there) or than --scale, no output
folder, an output folder that already holds files without --overwrite: ValueError naming the file or flag, from the file headers, before anything is decoded or
written."""
import argparse
import os
import time

from . import imgio, util

FOLDERS = ('sub', 'mod', 'lr', 'bic')
PNG_COMPRESSION = 3         # zlib level of every written file: extract_subimgs_single.py:19 (PIL's default 6 takes 2.4 x as long to encode the same pixels)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Sub-images, mod-cropped HR, bicubic LR and bicubic-upsampled (Bic) folders from a folder of HR images')
    p.add_argument('--input_dir', required=True, type=str, help='directory of the HR images (8-bit RGB PNG files)')
    p.add_argument('--sub_dir', default=None, type=str, help='directory the sub-images are written to; given: the sub-images are the units of everything else')
    p.add_argument('--crop_sz', default=480, type=int, help='side of a sub-image (extract_subimgs_single.py: 480)')
    p.add_argument('--step', default=240, type=int, help='stride of the sub-image grid (240)')
    p.add_argument('--thres_sz', default=48, type=int, help='a remainder above this many pixels gets one more sub-image flush with the border (48)')
    p.add_argument('--mod_dir', default=None, type=str, help='directory of the mod-cropped units')
    p.add_argument('--lr_dir', default=None, type=str, help='directory of the bicubic LR images')
    p.add_argument('--bic_dir', default=None, type=str, help='directory of the bicubic-upsampled LR images')
    p.add_argument('--scale', default=4, type=int, help='2, 3 or 4 (generate_mod_LR_bic.m: up_scale = mod_scale = 4)')
    p.add_argument('--num_workers', default=6, type=int, help='decode / encode threads (at most %d)' % imgio.MAX_DECODE_THREADS)
    p.add_argument('--overwrite', action='store_true', help='write into output folders that already hold files')
    p.add_argument('--device_png', action='store_true', help='encode the PNG files on the device (png.write_batch) instead of with PIL on the host threads')
    return p.parse_args(argv)


def axis_grid(n, crop_sz, step, thres_sz):
    """extract_subimgs_single.py:62-64 along one axis of n pixels: arange(0, n - crop_sz + 1, step), plus n - crop_sz when more than thres_sz pixels remain"""
    space = list(range(0, n - crop_sz + 1, step))
    if n - (space[-1] + crop_sz) > thres_sz:
        space.append(n - crop_sz)
    return space


def window_grid(h, w, crop_sz, step, thres_sz):
    """the top-left corners [(y0, x0)] of the sub-images of an h x w image in the order extract_subimgs_single.py:69-83 numbers them (row-major, _s001 first)"""
    if h < crop_sz or w < crop_sz:
        raise ValueError('a %d x %d image is smaller than crop_sz %d' % (h, w, crop_sz))
    return [(y, x) for y in axis_grid(h, crop_sz, step, thres_sz) for x in axis_grid(w, crop_sz, step, thres_sz)]


def plan(o):
    """everything that can be refused, from the flags, the folders and the file headers: ({folder key: directory}, [(file, name, H, W, [(y0, x0)], (uh, uw))]) with
    (uh, uw) the size of a unit before the mod-crop.  Decodes nothing and writes nothing."""
    from .bicubic import SCALES
    dirs = {k: getattr(o, k + '_dir') for k in FOLDERS if getattr(o, k + '_dir')}
    if not dirs:
        raise ValueError('no output folder given: at least one of --sub_dir, --mod_dir, --lr_dir, --bic_dir')
    if o.scale not in SCALES:
        raise ValueError('--scale must be one of %s, got %d' % (SCALES, o.scale))
    if getattr(o, 'device_png', False) and 'lr' not in dirs and 'bic' not in dirs:
        raise ValueError('--device_png needs --lr_dir or --bic_dir: --sub_dir and --mod_dir alone are byte copies made on the host, no device is opened for them')
    if o.crop_sz < 1 or o.step < 1 or o.thres_sz < 0:
        raise ValueError('--crop_sz and --step must be positive and --thres_sz not negative, got %d, %d, %d' % (o.crop_sz, o.step, o.thres_sz))
    if 'sub' in dirs and o.crop_sz < o.scale:
        raise ValueError('--crop_sz %d is smaller than --scale %d' % (o.crop_sz, o.scale))
    if not o.overwrite:
        for k, d in dirs.items():
            util.refuse_filled_folder(d, '--%s_dir' % k)
    names = sorted(x for x in os.listdir(o.input_dir) if x.lower().endswith('.png'))
    if not names:
        raise ValueError('--input_dir %s holds no PNG files' % o.input_dir)
    files = []
    for name in names:
        path = os.path.join(o.input_dir, name)
        H, W = imgio.rgb8_header(path, getattr(o, 'device_png', False), o.crop_sz if 'sub' in dirs else None)
        if 'sub' in dirs:
            if H < o.crop_sz or W < o.crop_sz:
                raise ValueError('%s: image %d x %d is smaller than --crop_sz %d' % (path, H, W, o.crop_sz))
            origins, unit = window_grid(H, W, o.crop_sz, o.step, o.thres_sz), (o.crop_sz, o.crop_sz)
        else:
            if H < o.scale or W < o.scale:
                raise ValueError('%s: image %d x %d is smaller than --scale %d' % (path, H, W, o.scale))
            origins, unit = [(0, 0)], (H, W)
        files.append((path, os.path.splitext(name)[0], H, W, origins, unit))
    return dirs, files


def run(o, times=None):
    """main behind the argument parser.  `times`: a list that receives one dict of seconds per file ('decode' as the consumer waits for it, 'upload', 'down', 'up', 'readback',
    'submit' and 'encode_wait', the consumer's wait for the encoders, both from the writer; with --device_png 'device_png', the batch's tables, launches and read-backs, in place of 'readback' and 'submit'); the device stages are then synchronised one by one, which an ordinary run does not do."""
    import torch
    from . import bicubic, png
    dirs, files = plan(o)
    s = o.scale
    device_png = getattr(o, 'device_png', False)
    device = imgio.device_of(None) if ('lr' in dirs or 'bic' in dirs) else None
    for d in dirs.values():
        util.mkdir(d)
    written = {k: [] for k in dirs}
    threads = max(1, min(imgio.MAX_DECODE_THREADS, int(o.num_workers)))
    clock, tick = time.perf_counter, imgio.tick
    # a call is a file: at most two files wait encoded or to be encoded next to the one in hand
    with png.FileWriter(device_png, threads, max_pending=2, compress_level=PNG_COMPRESSION) as writer:
        decoded = imgio.decode_ahead(imgio.decode_u8, [(f[0],) for f in files], threads)
        t0 = clock()
        for img, (path, name, H, W, origins, (uh, uw)) in zip(decoded, files):
            t = None
            if times is not None:
                t = writer.times = {'file': path, 'units': len(origins)}   # (the writer adds 'device_png' or 'submit', and 'encode_wait')
                times.append(t)
            t0 = tick(t, 'decode', t0)
            hh, ww = uh - uh % s, uw - uw % s
            units = [name + '_s%03d' % (k + 1) for k in range(len(origins))] if 'sub' in dirs else [name]
            src, lr, bic = img, None, None
            if 'lr' in dirs or 'bic' in dirs:
                dev_img = torch.from_numpy(img).to(device)
                t0 = tick(t, 'upload', t0, True)
                lr, lr_f64 = bicubic.down_windows_u8(dev_img, origins, (hh, ww), s, want_f64='bic' in dirs)
                t0 = tick(t, 'down', t0, True)
                bic = bicubic.upsample(lr_f64, s, out='u8') if 'bic' in dirs else None
                t0 = tick(t, 'up', t0, True)
                if device_png:      # sub and mod are windows of the uploaded image (pitch descriptors); nothing is read back
                    src = dev_img
                else:               # sub and mod are slices of the decoded array; one read-back per product
                    lr = lr.cpu().numpy() if 'lr' in dirs else None
                    bic = bic.cpu().numpy() if 'bic' in dirs else None
                    t0 = tick(t, 'readback', t0)
            images, paths = [], []
            for k, (unit, (y0, x0)) in enumerate(zip(units, origins)):
                for key, image, fname in (('sub', src[y0:y0 + uh, x0:x0 + uw], unit + '.png'), ('mod', src[y0:y0 + hh, x0:x0 + ww], unit + '.png'),
                                          ('lr', lr[k] if 'lr' in dirs else None, '%s_bicLRx%d.png' % (unit, s)),
                                          ('bic', bic[k] if 'bic' in dirs else None, '%s_bicx%d.png' % (unit, s))):
                    if key in dirs:
                        images.append(image)
                        paths.append(os.path.join(dirs[key], fname))
                        written[key].append(paths[-1])
            writer.write_many(images, paths)    # every product of the file: with --device_png ONE batch
            t0 = clock()
            print(name)
    return written


def main(argv=None):
    """returns {folder key ('sub', 'mod', 'lr', 'bic'): the written paths, in the order of the sorted file names and the window grid} for the folders given"""
    return run(parse_args(argv))


if __name__ == '__main__':
    main()
