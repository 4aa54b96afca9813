"""tests/golden/imresize_up.npz: outputs of the reference's MATLAB-style bicubic UP-sampling `data/util.py::imresize_np(img, s, True)` (codes/SRN/data/util.py:367-433)
for s = 2, 3, 4 on seeded random images of 6 x 9 ... 13 x 11 samples, plus a 1 x 3 and a 2 x 2 image (every tap mirrored).  It is the direction the back-projection
(dasr_amd/backproject.py) needs beside the down-sampling that tests/golden/imresize.npz pins.

TEST INFRASTRUCTURE: runs the reference code (oracle.ref_import), so it only works where the reference tree is importable:
    python scripts/gen_golden_imresize_up.py
Only the .npz (data) is committed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle import ref_import  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
CASES = ((6, 9, 2), (13, 11, 3), (8, 8, 4), (7, 10, 3), (1, 3, 2), (1, 3, 3), (1, 3, 4), (2, 2, 2), (2, 2, 3), (2, 2, 4))   # (h, w, s)


def main():
    if not ref_import.available():
        sys.exit('reference tree missing; fixtures can only be generated where it is importable')
    ref_import._mod('cv2')
    ref_import._mod('lmdb')
    sys.path[:0] = [os.path.join(ref_import.REF_ROOT, 'SRN'), ref_import.REF_ROOT]
    import data.util as dutil
    g = np.random.RandomState(23)
    out = {}
    for i, (h, w, s) in enumerate(CASES):
        img = g.rand(h, w, 3).astype(np.float32)
        out['in%d' % i] = img
        out['scale%d' % i] = np.int64(s)
        out['out%d' % i] = dutil.imresize_np(img, float(s), True).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, 'imresize_up.npz'), **out)
    print('wrote imresize_up.npz', {k: v.shape for k, v in out.items() if k.startswith('out')})


if __name__ == '__main__':
    main()
