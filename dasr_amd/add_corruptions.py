"""Make the corrupted source-domain folders of the DSN workflow -- codes/DSN/add_corruptions.py (codes/DSN/README.md:72-91) with the noise and the JPEG round trip on the MI355X.

    python -m dasr_amd.add_corruptions [--noise_std_dev 8.0] [--blur_std_dev None] [--jpg_quality 30] [--artifacts gaussian] [--dataset df2k] [--resolution hr|lr]
                                       [--paths paths.yml | --input_dir IN --output_dir OUT [--input_dir IN2 --output_dir OUT2 ...]]
                                       [--seed 0] [--num_workers 6] [--overwrite] [--device_png]

The flags of the reference with its defaults; the literal None (any case) switches a stage off (the reference's README passes `--noise_std_dev None`, which its own
type=float cannot parse).  The folders come from the yaml file as the reference reads it, [dataset]['clean'][resolution]['train' | 'valid'] ->
[dataset][artifacts][resolution]['train' | 'valid'] (created if missing), or from --input_dir / --output_dir pairs.

Every image file of an input folder is decoded on host threads (PIL, imgio.decode_ahead) and its bytes are uploaded once.  The stages run in the reference's order,
noise -> blur -> JPEG: corrupt.gaussian_noise (one launch; image index = position of the file in the sorted list of its folder, so a file does not depend on thread
counts or on the other files) and corrupt.jpeg_roundtrip (two launches; equal, bit for bit, to PIL's save + open with libjpeg-turbo) on the device.  --blur_std_dev is
PIL's own extended box blur (ImageFilter.GaussianBlur), run on the host exactly as the reference runs it: one read-back and re-upload for that file, logged once.  The
result is read back once and written as PNG under the input's base name on the host threads of a png.FileWriter (PIL, level 6).  With --device_png the file is encoded
on the device instead (the writer's device mode, png.write_batch: no read-back of the raw bytes, no PIL encode; the host threads add the container and the checksums); not together with --blur_std_dev, whose result
is made on the host.

The noise is NOT the reference's stream: utils.gaussian_noise draws from numpy's unseeded global generator, so its files differ from run to run; here they are a
function of --seed (corrupt.gaussian_noise_ref).

Accepted input is 8-bit RGB.  A grey, palette or alpha file, an output folder that already holds files without --overwrite, an output folder that is its input folder,
no stage switched on, a quality outside 1 .. 100, a folder without image files: ValueError naming the file or flag, from the flags and the file headers, before
anything is decoded or written."""
import argparse
import os
import time

from . import imgio, util
from .dsn_data import is_image_file

PNG_COMPRESSION = 6         # PIL's default, what the reference's image.save(path, 'PNG') uses (the pixels do not depend on it)


def _or_none(kind):
    def parse(s):
        return None if s.strip().lower() == 'none' else kind(s)
    parse.__name__ = kind.__name__
    return parse


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Generate noisy images')
    p.add_argument('--noise_std_dev', default=8.0, type=_or_none(float), help='standard deviation of the added gaussian noise (None: no noise)')
    p.add_argument('--blur_std_dev', default=None, type=_or_none(float), help='standard deviation of the added gaussian blur (None: no blur; runs on the host)')
    p.add_argument('--jpg_quality', default=30, type=_or_none(int), help='quality used for jpeg compression (None: no JPEG round trip)')
    p.add_argument('--artifacts', default='gaussian', type=str, help='selecting different artifacts type')
    p.add_argument('--dataset', default='df2k', type=str, help='selecting different datasets')
    p.add_argument('--resolution', default='hr', type=str, choices=['hr', 'lr'], help='choose whether to use HR or LR')
    # additions of this build
    p.add_argument('--paths', default='paths.yml', type=str, help="yaml file with the dataset folders (the reference reads 'paths.yml')")
    p.add_argument('--input_dir', action='append', default=None, type=str, help='folder of clean images, instead of the names from --paths; repeatable, one --output_dir each')
    p.add_argument('--output_dir', action='append', default=None, type=str, help='folder the corrupted images of the matching --input_dir are written to')
    p.add_argument('--seed', default=0, type=int, help='64-bit key of the noise generator')
    p.add_argument('--num_workers', default=6, type=int, help='decode / encode threads (at most %d)' % imgio.MAX_DECODE_THREADS)
    p.add_argument('--overwrite', action='store_true', help='write into output folders that already hold files')
    p.add_argument('--device_png', action='store_true', help='encode the PNG files on the device (png.write_batch) instead of with PIL on the host threads')
    return p.parse_args(argv)


def folder_pairs(o):
    """[(input folder, output folder)]: the --input_dir / --output_dir pairs, else the train and valid folders of --paths (add_corruptions.py:25-31)"""
    if o.input_dir or o.output_dir:
        if len(o.input_dir or []) != len(o.output_dir or []):
            raise ValueError('--input_dir and --output_dir come in pairs: got %d and %d' % (len(o.input_dir or []), len(o.output_dir or [])))
        return list(zip(o.input_dir, o.output_dir))
    from .dsn_data import load_paths
    paths = load_paths(o.paths)
    try:
        return [(paths[o.dataset]['clean'][o.resolution][k], paths[o.dataset][o.artifacts][o.resolution][k]) for k in ('train', 'valid')]
    except (KeyError, TypeError):
        raise KeyError("%s has no entries ['%s']['clean' and '%s']['%s']['train' and 'valid'] (codes/DSN/paths.yml layout)" % (o.paths, o.dataset, o.artifacts, o.resolution))


def plan(o):
    """everything that can be refused, from the flags, the folders and the file headers: [(output folder, [(input file, output file, image index, H, W)])].  Decodes
    nothing and writes nothing."""
    from .corrupt import check_quality
    if o.noise_std_dev is None and o.blur_std_dev is None and o.jpg_quality is None:
        raise ValueError('no stage switched on: --noise_std_dev, --blur_std_dev and --jpg_quality are all None')
    if o.jpg_quality is not None:
        try:
            check_quality(o.jpg_quality)
        except ValueError:
            raise ValueError('--jpg_quality must lie in 1 .. 100, got %r' % (o.jpg_quality,))
    if o.noise_std_dev is not None and not 0.0 <= o.noise_std_dev < float('inf'):
        raise ValueError('--noise_std_dev must be finite and not negative, got %r' % (o.noise_std_dev,))
    if getattr(o, 'device_png', False) and o.blur_std_dev is not None:
        raise ValueError('--device_png cannot be combined with --blur_std_dev: the blurred image is made by PIL on the host')
    if o.blur_std_dev is not None and not 0.0 <= o.blur_std_dev < float('inf'):
        raise ValueError('--blur_std_dev must be finite and not negative, got %r' % (o.blur_std_dev,))
    work = []
    for src, dst in folder_pairs(o):
        if not os.path.isdir(src):
            raise ValueError('input folder %s does not exist' % src)
        if os.path.abspath(src) == os.path.abspath(dst):
            raise ValueError('output folder %s is its own input folder' % dst)
        if not o.overwrite:
            util.refuse_filled_folder(dst, 'output folder')
        names = sorted(x for x in os.listdir(src) if is_image_file(x))
        if not names:
            raise ValueError('input folder %s holds no image files' % src)
        files = []
        for index, name in enumerate(names):
            path = os.path.join(src, name)
            H, W = imgio.rgb8_header(path, getattr(o, 'device_png', False))
            files.append((path, os.path.join(dst, name), index, H, W))
        work.append((dst, files))
    return work


def _blur_host(dev_img, std):
    """ImageFilter.GaussianBlur(std) of a device image on the host, as add_corruptions.py:47-48 applies it"""
    import numpy as np
    import torch
    from PIL import Image, ImageFilter
    a = np.array(Image.fromarray(dev_img.cpu().numpy()).filter(ImageFilter.GaussianBlur(std)), dtype=np.uint8)
    return torch.from_numpy(a).to(dev_img.device)


def run(o, times=None):
    """main behind the argument parser.  `times`: a list that receives one dict of seconds per file ('decode' as the consumer waits for it, 'upload', 'kernels', 'blur',
    'readback', 'submit' and 'encode_wait', the consumer's wait for the encoders, both from the writer; with --device_png 'device_png' in place of 'readback' and 'submit'); the device stages are then synchronised one by one, which an ordinary run does not do."""
    import torch
    from . import corrupt, png
    work = plan(o)
    device_png = getattr(o, 'device_png', False)
    device = imgio.device_of(None)
    for dst, _ in work:
        util.mkdir(dst)
    threads = max(1, min(imgio.MAX_DECODE_THREADS, int(o.num_workers)))
    clock, tick = time.perf_counter, imgio.tick
    if o.blur_std_dev is not None:
        print('--blur_std_dev %g: PIL GaussianBlur on the host, one read-back and re-upload per file' % o.blur_std_dev)
    # at most 2 x threads results wait encoded or to be encoded next to the one in hand
    with png.FileWriter(device_png, threads, compress_level=PNG_COMPRESSION) as writer:
        for dst, files in work:
            print('\nComputing images from directory ' + os.path.dirname(files[0][0]))
            decoded = imgio.decode_ahead(imgio.decode_u8, [(f[0],) for f in files], threads)
            t0 = clock()
            for img, (path, out_path, index, H, W) in zip(decoded, files):
                t = None
                if times is not None:
                    t = writer.times = {'file': path}   # (the writer adds 'device_png' or 'submit', and 'encode_wait')
                    times.append(t)
                t0 = tick(t, 'decode', t0)
                x = torch.from_numpy(img).to(device)
                t0 = tick(t, 'upload', t0, True)
                if o.noise_std_dev is not None:
                    x = corrupt.gaussian_noise(x, o.noise_std_dev, o.seed, index)
                    t0 = tick(t, 'kernels', t0, True)
                if o.blur_std_dev is not None:
                    x = _blur_host(x, o.blur_std_dev)
                    t0 = tick(t, 'blur', t0, True)
                if o.jpg_quality is not None:
                    x = corrupt.jpeg_roundtrip(x, o.jpg_quality)
                    t0 = tick(t, 'kernels', t0, True)
                if not device_png:
                    x = x.cpu().numpy()
                    t0 = tick(t, 'readback', t0)
                writer.write(x, out_path)   # PNG bytes under the input's base name, whatever its extension (the reference writes 'PNG' there)
                t0 = clock()
    return writer.paths


def main(argv=None):
    """returns the written files, folder by folder in the order of the sorted file names"""
    return run(parse_args(argv))


if __name__ == '__main__':
    main()
