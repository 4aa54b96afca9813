"""Prepare the training folders of the SRN option files from a folder of HR images -- codes/SRN/scripts/extract_subimgs_single.py and generate_mod_LR_bic.m (MATLAB only)
in one pass over the files, on the MI355X (codes/SRN/data/README.md:26-27: DIV2K800 -> DIV2K800_sub, DIV2K800_sub_bicLRx4).

    python -m dasr_amd.prepare_data --input_dir HR [--sub_dir D --crop_sz 480 --step 240 --thres_sz 48] [--mod_dir D] [--lr_dir D] [--bic_dir D] [--scale 4]
                                    [--num_workers 6] [--overwrite] [--device_png]

Every PNG file of --input_dir is decoded once on host threads (PIL, imgio.decode_ahead) and its BYTES are uploaded once.  With --sub_dir the units are the sub-images of
extract_subimgs_single.py:62-83 (window_grid; written to --sub_dir as name_s001.png, ... in row-major order), without it the whole images.  Every unit is mod-cropped to a
multiple of --scale, then --mod_dir gets name.png (the mod-cropped bytes), --lr_dir name_bicLRx{s}.png (MATLAB's imresize(., 1 / s) of the unit, written as imwrite
writes a double image) and --bic_dir name_bicx{s}.png (imresize(., s) of the DOUBLE LR image).  The sub and mod files are byte copies sliced on the host; the LR images of
all units of a file are ONE dasr_windows_down_u8 launch, their Bic images ONE dasr_imresize_up launch (bicubic.py), one read-back per file and product; the PNG files
are encoded on host threads (zlib level 3, as extract_subimgs_single.py:19 sets it: the pixels do not depend on it).  With --device_png all products of a file are
encoded on the device in one png.write_batch (sub and mod as windows of the uploaded image): no read-back of raw bytes, no PIL encode; the host threads add the
container and the checksums.  It needs --lr_dir or --bic_dir (without them no device is opened).  The mirror edge of the resampling
is the unit's edge: a file of --lr_dir is what MATLAB makes of the file of --sub_dir, not a crop of the whole image's LR image.

Accepted input is 8-bit RGB.  A grey, palette or alpha file, a file smaller than --crop_sz (the reference script raises IndexError there) or than --scale, no output
folder, an output folder that already holds files without --overwrite: ValueError naming the file or flag, from the file headers, before anything is decoded or
written."""
import argparse
import os
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor

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
            if os.path.isdir(d) and os.listdir(d):
                raise ValueError('--%s_dir %s already holds files (pass --overwrite to write into it)' % (k, d))
    names = sorted(x for x in os.listdir(o.input_dir) if x.lower().endswith('.png'))
    if not names:
        raise ValueError('--input_dir %s holds no PNG files' % o.input_dir)
    files = []
    for name in names:
        path = os.path.join(o.input_dir, name)
        H, W, mode = imgio.image_header(path)
        if mode != 'RGB':
            raise ValueError('%s: mode %s, expected an 8-bit RGB image' % (path, mode))
        if H > 65535 or W > 65535:
            raise ValueError('%s: %d x %d, a side above 65535' % (path, H, W))
        if 'sub' in dirs:
            if H < o.crop_sz or W < o.crop_sz:
                raise ValueError('%s: image %d x %d is smaller than --crop_sz %d' % (path, H, W, o.crop_sz))
            origins, unit = window_grid(H, W, o.crop_sz, o.step, o.thres_sz), (o.crop_sz, o.crop_sz)
        else:
            if H < o.scale or W < o.scale:
                raise ValueError('%s: image %d x %d is smaller than --scale %d' % (path, H, W, o.scale))
            origins, unit = [(0, 0)], (H, W)
        if getattr(o, 'device_png', False) and unit[1] > 21844:
            raise ValueError('%s: --device_png encodes rows of at most 21844 pixels, a unit here has %d (leave the flag out: PIL encodes on the host)' % (path, unit[1]))
        files.append((path, os.path.splitext(name)[0], H, W, origins, unit))
    return dirs, files


def _save_rgb(arr, path):
    """RGB bytes [h, w, 3] -> PNG"""
    from PIL import Image
    Image.fromarray(arr).save(path, compress_level=PNG_COMPRESSION)
    return path


def run(o, times=None):
    """main behind the argument parser.  `times`: a list that receives one dict of seconds per file ('decode' as the consumer waits for it, 'upload', 'down', 'up', 'readback',
    'submit' and 'encode_wait', the consumer's wait for the encoders; with --device_png 'device_png', the batch's tables, launches and read-backs, in place of 'readback'); the device stages are then synchronised one by one, which an ordinary run does not do."""
    import numpy as np
    import torch
    from . import bicubic, png
    dirs, files = plan(o)
    s = o.scale
    device_png = getattr(o, 'device_png', False)
    if device_png:
        print('--device_png: the PNG files are encoded on the device (filter, Huffman-only deflate), the host adds the container and the checksums')
    device = imgio.device_of(None) if ('lr' in dirs or 'bic' in dirs) else None
    for d in dirs.values():
        util.mkdir(d)
    written = {k: [] for k in FOLDERS}
    threads = max(1, min(imgio.MAX_DECODE_THREADS, int(o.num_workers)))
    clock = time.perf_counter

    def tick(t, key, t0, sync=False):
        if times is not None:
            if sync:
                torch.cuda.synchronize()
            t[key] = t.get(key, 0.0) + clock() - t0
        return clock()

    with ThreadPoolExecutor(max_workers=threads) as enc:
        pending = deque()   # the encode jobs of the files in flight: at most two files wait encoded or to be encoded next to the one in hand

        def drain(keep):
            while len(pending) > keep:
                t0 = clock()
                for k, fut in pending.popleft():
                    written[k].append(fut.result())
                if times is not None:
                    times[-1]['encode_wait'] = times[-1].get('encode_wait', 0.0) + clock() - t0
        decoded = imgio.decode_ahead(imgio.decode_u8, [(f[0],) for f in files], threads)
        t0 = clock()
        for img, (path, name, H, W, origins, (uh, uw)) in zip(decoded, files):
            t = {'file': path, 'units': len(origins)}
            if times is not None:
                times.append(t)
            t0 = tick(t, 'decode', t0)
            hh, ww = uh - uh % s, uw - uw % s
            units = [name + '_s%03d' % (k + 1) for k in range(len(origins))] if 'sub' in dirs else [name]
            jobs = []
            if 'lr' in dirs or 'bic' in dirs:
                dev_img = torch.from_numpy(img).to(device)
                t0 = tick(t, 'upload', t0, True)
                lr_u8, lr_f64 = bicubic.down_windows_u8(dev_img, origins, (hh, ww), s, want_f64='bic' in dirs)
                t0 = tick(t, 'down', t0, True)
                bic_u8 = bicubic.upsample(lr_f64, s, out='u8') if 'bic' in dirs else None
                t0 = tick(t, 'up', t0, True)
                if not device_png:
                    lr_host = lr_u8.cpu().numpy() if 'lr' in dirs else None
                    bic_host = bic_u8.cpu().numpy() if 'bic' in dirs else None
                    t0 = tick(t, 'readback', t0)
            if device_png:
                # every product of the file in one batch, from the tensors that sit on the device: sub and mod are windows of the uploaded image (pitch descriptors)
                keys, tensors, paths = [], [], []
                for k, (unit, (y0, x0)) in enumerate(zip(units, origins)):
                    for key, tensor, path in (('sub', dev_img[y0:y0 + uh, x0:x0 + uw], unit + '.png'), ('mod', dev_img[y0:y0 + hh, x0:x0 + ww], unit + '.png'),
                                              ('lr', lr_u8[k] if 'lr' in dirs else None, '%s_bicLRx%d.png' % (unit, s)),
                                              ('bic', bic_u8[k] if 'bic' in dirs else None, '%s_bicx%d.png' % (unit, s))):
                        if key in dirs:
                            keys.append(key)
                            tensors.append(tensor)
                            paths.append(os.path.join(dirs[key], path))
                jobs = list(zip(keys, png.write_batch(tensors, paths, enc)))
                t0 = tick(t, 'device_png', t0)
            else:
                for k, (unit, (y0, x0)) in enumerate(zip(units, origins)):
                    if 'sub' in dirs:
                        jobs.append(('sub', enc.submit(_save_rgb, np.ascontiguousarray(img[y0:y0 + uh, x0:x0 + uw]), os.path.join(dirs['sub'], unit + '.png'))))
                    if 'mod' in dirs:
                        jobs.append(('mod', enc.submit(_save_rgb, np.ascontiguousarray(img[y0:y0 + hh, x0:x0 + ww]), os.path.join(dirs['mod'], unit + '.png'))))
                    if 'lr' in dirs:
                        jobs.append(('lr', enc.submit(_save_rgb, lr_host[k], os.path.join(dirs['lr'], '%s_bicLRx%d.png' % (unit, s)))))
                    if 'bic' in dirs:
                        jobs.append(('bic', enc.submit(_save_rgb, bic_host[k], os.path.join(dirs['bic'], '%s_bicx%d.png' % (unit, s)))))
            pending.append(jobs)
            t0 = tick(t, 'submit', t0)
            drain(2)
            t0 = clock()
            print(name)
        drain(0)
    return {k: v for k, v in written.items() if k in dirs}


def main(argv=None):
    """returns {folder key ('sub', 'mod', 'lr', 'bic'): the written paths, in the order of the sorted file names and the window grid} for the folders given"""
    return run(parse_args(argv))


if __name__ == '__main__':
    main()
