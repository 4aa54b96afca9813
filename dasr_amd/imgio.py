"""Host side of csrc/imgio.hip, shared by the SRN datasets (data.py), the DSN datasets (dsn_data.py) and the folder CLIs: the one PIL decode and its decode-ahead loop,
the hand-off of decoded bytes to a planar fp32 device image, the store of decoded bytes resident in device memory, the fp64 tap tables of MATLAB's bicubic with their
device cache, and the descriptor upload in front of the batch-assembly launches.  Imports neither of the two dataset modules; both import this one."""
import ctypes as C
import itertools
import math
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .engine import _stream, ensure_runtime_ready

MAX_DECODE_THREADS = 16


def image_header(path):
    """(H, W, PIL mode) from the file header, without decoding"""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0], im.mode


def image_size(path):
    return image_header(path)[:2]


def rgb8_header(path, device_png=False, unit_width=None):
    """(H, W) of a file the folder CLIs accept, from its header: ValueError naming the file for a mode other than RGB, a side above 65535 or, with `device_png`, rows
    wider than the device encoder takes (png.max_width('rgb')); `unit_width`: the width of what is encoded when that is not the whole file (prepare_data's sub-images)"""
    from .png import max_width
    H, W, mode = image_header(path)
    if mode != 'RGB':
        raise ValueError('%s: mode %s, expected an 8-bit RGB image' % (path, mode))
    if H > 65535 or W > 65535:
        raise ValueError('%s: %d x %d, a side above 65535' % (path, H, W))
    if device_png and (unit_width or W) > max_width('rgb'):
        raise ValueError('%s: --device_png encodes rows of at most %d pixels, %s has %d (leave the flag out: PIL encodes on the host)' % (
            path, max_width('rgb'), 'this file' if unit_width is None else 'a unit here', unit_width or W))
    return H, W


def tick(times, key, t0, sync=False):
    """THE stage clock: adds the seconds since t0 to times[key] and returns the new t0.  `times` None: nothing is measured and nothing synchronised; `sync`: the device is
    synchronised first, so the stage's launches are in the number (which an ordinary run does not do)"""
    if times is not None:
        if sync:
            torch.cuda.synchronize()
        times[key] = times.get(key, 0.0) + time.perf_counter() - t0
    return time.perf_counter()


def decode_u8(path, box=None):
    """THE decode: file -> uint8 [H, W, 3] RGB array (grey / palette / alpha files are converted); box (left, upper, right, lower): that window only"""
    from PIL import Image
    with Image.open(path) as im:   # (the converted whole image stays a temporary: with a box it is freed before the array is made, which the allocator rewards)
        return np.array(im.convert('RGB') if box is None else im.convert('RGB').crop(box), dtype=np.uint8)


def u8_to_chw(a):
    """decoded bytes [H, W, 3] -> CHW fp32 in [0, 1] (`to_tensor`: one correctly rounded division by 255, bit for bit np.float32(a) / 255.0; a permuted view,
    not contiguous)"""
    return torch.from_numpy(a).permute(2, 0, 1).float().div_(255.0)


def planar_f32(a, device=None, window=None, batch=False):
    """THE hand-off of decoded bytes: uint8 [H, W, 3], a numpy array (uploaded to `device`, None: the current GPU; one byte per sample crosses) or a device tensor -> the planar fp32 device
    image [3, Hc, Wc] = byte / 255 correctly rounded (bit for bit u8_to_chw), `window` (Hc, Wc): that top-left window only (None: the whole image), `batch`: with a
    leading axis of 1.  One dasr_u8_to_planar launch on the current stream."""
    u8 = a if torch.is_tensor(a) else torch.from_numpy(a).to(device_of(device))
    H, W = u8.shape[:2]
    Hc, Wc = window or (H, W)
    out = torch.empty(((1, 3, Hc, Wc) if batch else (3, Hc, Wc)), dtype=torch.float32, device=u8.device)
    _lib.check(_lib.lib().dasr_u8_to_planar(u8.data_ptr(), H, W, Hc, Wc, out.data_ptr(), _stream()), 'dasr_u8_to_planar')
    return out


def decode_ahead(load, jobs, threads):
    """yields load(*job) for every job, in order, from a pool of `threads` host threads (clamped to [1, MAX_DECODE_THREADS]) that runs ahead of the consumer: 2 x threads
    jobs are submitted at the start, then one more behind every result taken from the queue, so at most 2 x threads results are decoded or wait in host memory next to
    the one the consumer holds.  An exception of `load` surfaces at its item."""
    threads = max(1, min(MAX_DECODE_THREADS, int(threads)))
    with ThreadPoolExecutor(max_workers=threads) as pool:
        todo = iter(jobs)
        ahead = deque(pool.submit(load, *job) for job in itertools.islice(todo, 2 * threads))
        while ahead:
            result = ahead.popleft().result()
            for job in itertools.islice(todo, 1):
                ahead.append(pool.submit(load, *job))
            yield result


def device_of(device):
    """the device the images live on (None: the current GPU, with its index); 'cpu' touches no GPU"""
    if device is not None and torch.device(device).type == 'cpu':
        return torch.device('cpu')
    ensure_runtime_ready()
    dev = torch.device('cuda') if device is None else torch.device(device)
    return dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())


def load_resident(file_lists, device=None, threads=6, max_bytes=None, min_size=0, remedy='train with the host loader (without --device_data)'):
    """the files of every list decoded once (PIL, RGB, uint8 [H, W, 3]) on a pool of at most 16 threads and uploaded to `device`: (the device, lists of uint8 tensors).
    The sizes are read from the file headers and summed BEFORE anything is decoded or the device is touched: an image with a side under `min_size` is a
    ValueError naming the file, a total of H W 3 bytes above `max_bytes` (default: half of the device memory free right now) a MemoryError.  Nothing spills
    to the host.  (The default cap is taken per call: a validation set loaded after its train set is held to half of what the train set left free.)
    device 'cpu' keeps the bytes in host memory: enough for plan_item, not for assembling batches.  `remedy`: what the MemoryError tells the caller to do instead."""
    from concurrent.futures import ThreadPoolExecutor
    total = 0
    for files in file_lists:
        for path in files:
            h, w = image_size(path)
            if h < min_size or w < min_size:
                raise ValueError('%s: image %dx%d is smaller than the crop size %d' % (path, h, w, min_size))
            total += h * w * 3

    def refuse(cap):
        raise MemoryError('the decoded images take %d bytes, above the cap of %d bytes for images resident in device memory: %s or raise max_bytes' % (total, cap, remedy))
    if max_bytes is not None and total > max_bytes:
        refuse(max_bytes)
    dev = device_of(device)
    if max_bytes is None and dev.type == 'cuda' and total > torch.cuda.mem_get_info(dev)[0] // 2:
        refuse(torch.cuda.mem_get_info(dev)[0] // 2)
    threads = max(1, min(MAX_DECODE_THREADS, int(threads)))
    out = []
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for files in file_lists:
            imgs = []
            for k in range(0, len(files), 4 * threads):   # (decoded arrays wait in host memory one chunk at a time)
                imgs += [torch.from_numpy(a).to(dev) for a in pool.map(decode_u8, files[k:k + 4 * threads])]
            out.append(imgs)
    return dev, out


def bicubic_taps(n_in, scale):
    """per-output-sample taps of MATLAB's imresize along one axis, in float64: (j, w), both [n_out, taps] with taps = ceil(kernel width) + 2.  Bicubic kernel (a = -0.5),
    widened by 1 / scale and scaled by `scale` when shrinking (antialiasing), weights normalised to sum 1 per output sample, samples beyond the ends mirrored about the edge
    (the edge sample itself repeated): j is the 0-based source index after mirroring.  Output sample k (1-based) sits at u = k / scale + (1 - 1 / scale) / 2 in input
    coordinates.  What codes/SRN/data/util.py:243-297 computes.  The dense matrix of data.imresize_matlab and every device table (tap_table) come from here."""
    n_out = int(math.ceil(n_in * scale))
    width = 4.0 / scale if scale < 1 else 4.0
    taps = int(math.ceil(width)) + 2
    k = torch.arange(1, n_out + 1, dtype=torch.float64)
    u = k / scale + 0.5 * (1.0 - 1.0 / scale)
    left = torch.floor(u - width / 2.0)
    idx = left[:, None] + torch.arange(taps, dtype=torch.float64)[None, :]        # 1-based input positions
    d = (u[:, None] - idx) * (scale if scale < 1 else 1.0)
    a = d.abs()
    w = torch.where(a <= 1, 1.5 * a ** 3 - 2.5 * a ** 2 + 1, torch.where(a <= 2, -0.5 * a ** 3 + 2.5 * a ** 2 - 4 * a + 2, torch.zeros_like(a)))
    if scale < 1:
        w = w * scale
    w = w / w.sum(1, keepdim=True)
    j = idx.long() - 1                                                              # 0-based; mirror: -1 -> 0, -2 -> 1, n -> n - 1, n + 1 -> n - 2
    j = torch.where(j < 0, -j - 1, j)
    j = torch.where(j >= n_in, 2 * n_in - 1 - j, j).clamp_(0, n_in - 1)
    return j, w


_TABLES, _W18 = {}, None


def tap_table(n_in, s, device):
    """device tap table of bicubic_taps(n_in, 1 / s) as dasr_imresize_down and dasr_crops_bicubic_down read it: (int32 index, fp64 weight), both [n_in / s, 4 s + 2];
    uploaded once per (device, n_in, s) for the whole process"""
    key = (device, n_in, s)
    if key not in _TABLES:
        j, w = bicubic_taps(n_in, 1.0 / s)
        _TABLES[key] = (j.to(torch.int32).contiguous().to(device), w.contiguous().to(device))
    return _TABLES[key]


def down_table_ptrs(H, W, s, device):
    """the device pointers (row index, row weight, column index, column weight) of the tap_table pair of an H x W image shrunk by s, in the argument order of
    dasr_imresize_down and dasr_bp_residual"""
    return [t.data_ptr() for n in (H, W) for t in tap_table(n, s, device)]


def up_tap_table(n_in, s, device):
    """device tap table of bicubic_taps(n_in, s), the up-sampling by the integer s as dasr_bp_update reads it: (int32 index, fp64 weight), both [s n_in, 6];
    uploaded once per (device, n_in, s) for the whole process"""
    key = (device, n_in, s, 'up')
    if key not in _TABLES:
        j, w = bicubic_taps(n_in, float(s))
        _TABLES[key] = (j.to(torch.int32).contiguous().to(device), w.contiguous().to(device))
    return _TABLES[key]


def down4_weights():
    """the 18 weights of MATLAB's antialiased bicubic at scale 1 / 4 as a ctypes array: ONE row of bicubic_taps(n, 0.25)[1] -- the sample positions u = 4 k - 1.5 have the
    same fractional part for every k, so every output sample has bit-equal weights (tests/test_srn_device_data_host.py)"""
    global _W18
    if _W18 is None:
        _W18 = (C.c_double * 18)(*bicubic_taps(32, 0.25)[1][0].tolist())
    return _W18


def upload(device, *arrays):
    """the descriptor upload of one batch: every ctypes array copied into ONE block of pinned memory that crosses in one asynchronous copy on the current stream; no host
    synchronisation.  Returns (the device block, the byte offset of each array in it); the caller keeps the block until its launches are enqueued."""
    if device.type != 'cuda':
        raise _lib.DasrHipError('batches are assembled by HIP kernels on images resident in device memory; this dataset was built on %s' % device)
    offsets = [0]
    for a in arrays:
        offsets.append(offsets[-1] + C.sizeof(a))
    staging = torch.empty(offsets[-1], dtype=torch.uint8, pin_memory=True)   # (torch's pinned-memory cache hands a block out again only after the copy below is done)
    for a, off in zip(arrays, offsets):
        C.memmove(staging.data_ptr() + off, a, C.sizeof(a))
    return staging.to(device, non_blocking=True), offsets[:-1]


def fill_crop_desc(d, t, virt, y0, x0, flags):
    """one dasr_crop_desc of dasr_gather_crops: the window at (y0, x0) of the planar fp32 image t [C, H, W] seen resized bilinearly to virt = (vH, vW) (None: as it is)"""
    d.src, d.C, d.H, d.W = t.data_ptr(), t.shape[0], t.shape[1], t.shape[2]
    d.vH, d.vW = virt if virt is not None else (t.shape[1], t.shape[2])
    d.y0, d.x0, d.flags = y0, x0, flags
