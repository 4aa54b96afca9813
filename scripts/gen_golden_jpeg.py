"""Writes tests/golden/jpeg_roundtrip.npz: small RGB images and what PIL gives back for them after Image.save(buf, 'JPEG', quality=q) and Image.open -- the bytes
corrupt.jpeg_roundtrip_ref and the device path have to reproduce.  Uses PIL (and numpy for the arrays) only, nothing of this project.

The arrays are packed (a zip member per array would cost more than the pixels): 'names' = 'in_<H>x<W>_<content>' and 'out_<H>x<W>_<content>_q<quality>', 'shapes' int32
[n, 3], 'blob' = the uint8 [H, W, 3] arrays one after the other in the order of 'names'; 'versions' = [PIL version, libjpeg version string, 'libjpeg_turbo' flag].
unpack() below is the reader (the tests carry the same few lines).

Sizes: 1x1, 2x2, 3x5, 5x4 (chroma width 2: the replication path), 8x8, 16x16, 17x33, 40x24 (even H that is no multiple of 16: the chroma-row rule), 31x6, 37x53, 64x48,
50x130.  Quality 30 at every size; 1, 5, 50, 75, 95 and 100 at 17x33 and 40x24.  Contents: seeded random bytes, a constant colour, a 0 / 255 checkerboard at pixel pitch,
saturated primaries in stripes, a smooth gradient.

    python scripts/gen_golden_jpeg.py [--out tests/golden/jpeg_roundtrip.npz]
"""
import argparse
import io
import os

import numpy as np
from PIL import Image, features
import PIL

SIZES = ((1, 1), (2, 2), (3, 5), (5, 4), (8, 8), (16, 16), (17, 33), (40, 24), (31, 6), (37, 53), (64, 48), (50, 130))
MANY_QUALITIES = ((17, 33), (40, 24))
QUALITIES = (1, 5, 50, 75, 95, 100)
CONTENTS = ('random', 'constant', 'checker', 'primaries', 'gradient')


def content(kind, H, W):
    y, x = np.mgrid[0:H, 0:W]
    if kind == 'random':
        return np.random.RandomState(1000 * H + W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == 'constant':
        return np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8), (H, W, 3)).copy()
    if kind == 'checker':
        return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    if kind == 'primaries':   # stripes 3 pixels wide: red, green, blue, yellow, cyan, magenta, white, black
        table = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]], dtype=np.uint8)
        return table[((x // 3) + (y // 5)) % 8]
    if kind == 'gradient':
        fy, fx = y / max(H - 1, 1), x / max(W - 1, 1)
        return np.stack([255 * fx, 255 * fy, 255 * (1 - 0.5 * (fx + fy))], axis=-1).round().astype(np.uint8)
    raise ValueError(kind)


def roundtrip(a, q):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, 'JPEG', quality=q)
    buf.seek(0)
    return np.array(Image.open(buf), dtype=np.uint8)


def unpack(path):
    """{name: uint8 [H, W, 3]} and the version strings of a file this script wrote"""
    z = np.load(path)
    ends = np.cumsum(z['shapes'].prod(axis=1))
    return {str(n): z['blob'][e - s[0] * s[1] * s[2]:e].reshape(s) for n, s, e in zip(z['names'], z['shapes'], ends)}, [str(v) for v in z['versions']]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'jpeg_roundtrip.npz'))
    args = ap.parse_args()
    versions = np.array([PIL.__version__, str(features.version('jpg')), 'libjpeg_turbo=%s' % features.check('libjpeg_turbo')])
    data = {}
    for H, W in SIZES:
        for kind in CONTENTS:
            a = content(kind, H, W)
            data['in_%dx%d_%s' % (H, W, kind)] = a
            for q in (30,) + (QUALITIES if (H, W) in MANY_QUALITIES else ()):
                data['out_%dx%d_%s_q%d' % (H, W, kind, q)] = roundtrip(a, q)
    np.savez_compressed(args.out, names=np.array(list(data)), shapes=np.array([a.shape for a in data.values()], dtype=np.int32),
                        blob=np.concatenate([a.reshape(-1) for a in data.values()]), versions=versions)
    back, _ = unpack(args.out)
    assert list(back) == list(data) and all(np.array_equal(back[k], data[k]) for k in data)
    print('%s: %d arrays, %d bytes; %s' % (args.out, len(data), os.path.getsize(args.out), ' '.join(versions)))


if __name__ == '__main__':
    main()
