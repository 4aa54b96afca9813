"""Device-side input pipeline for the DASR unpaired dataset.

Reference: codes/SRN/data/LRHR_wavelet_unpairEq_fake_w_dataset.py:50-166 (`__getitem__`), data/util.py:78-128 (read_img, augment),
DataLoader collation.  The reference decodes four images per sample on CPU workers, resizes the domain-distance map with
cv2.INTER_LINEAR, crops, flips / transposes with numpy and ships the batch over PCIe.  Here every image (and every ddm array) is
uploaded ONCE as a CHW fp32 RGB tensor; a batch is n descriptors (image, crop origin, flags) and five `dasr_gather_crops`
launches that write the five batch tensors of the reference's dict directly in HBM.  Random draws are made on the host in the
reference's order (np.random for the unpaired indices, `random` for the crop origins and the three augmentation coins), so with
equal seeds and num_workers=0 the batches coincide.  Image decoding (PIL) stays on the host and happens once per file.

`"resident_u8": true` in `datasets.train` (both training datasets): the files are decoded once on `n_workers` threads (imgio.load_resident) and stay in device
memory as the BYTES PIL decodes (uint8 [H][W][3], a quarter of the fp32 store); the domain-distance maps stay fp32.  A batch is one descriptor block in pinned memory,
one asynchronous upload (imgio.upload: the fp32 store takes the same road) and at most three launches: dasr_gather_srn_u8 (every 3-channel tensor of the batch), dasr_gather_crops (fake_w) and, for `mode: "LRHR"` without
LR files, dasr_crops_down4_u8 (the LR crops, straight from the HR bytes).  The random draws are the same calls in the same order, so equal seeds give equal batches with
and without the key: bit for bit, except the LR images made on the device (one rounding to fp32 of the fp64 evaluation: within 2^-23 of imresize_matlab).
The host side of csrc/imgio.hip that the DSN datasets use as well (decode, resident store, tap tables, descriptor upload) is imgio.py.
"""
import ctypes as C
import logging
import os
import random
import time

import numpy as np
import torch

from . import _lib
from .engine import _stream
from .imgio import bicubic_taps, decode_u8, device_of, down4_weights, down_table_ptrs, fill_crop_desc, image_header, load_resident, planar_f32, u8_to_chw, upload

IMG_EXTENSIONS = ('.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP')


def image_paths(root):
    """sorted image (and .npy) files under root (data/util.py:24-38)"""
    out = []
    for dirpath, _, fnames in sorted(os.walk(root)):
        for f in sorted(fnames):
            if f.endswith(IMG_EXTENSIONS) or f.endswith('.npy'):
                out.append(os.path.join(dirpath, f))
    return sorted(out)


def load_image(path):
    """file -> CHW fp32 RGB in [0,1] (read_img gives HWC BGR; the dataset flips to RGB at the end: same values)"""
    if path.endswith('.npy'):
        a = np.load(path)
        return torch.from_numpy(np.ascontiguousarray(a[0] if a.ndim == 4 else a)).float()
    return u8_to_chw(decode_u8(path)).contiguous()


def _hw(t):
    """(H, W) of a stored image: planar fp32 [C, H, W], or the decoded bytes [H, W, 3] of `resident_u8`"""
    return (t.shape[0], t.shape[1]) if t.dtype == torch.uint8 else (t.shape[1], t.shape[2])


def _u8_header(path):
    """(H, W) of an image file that can be stored as the bytes PIL decodes, from its header; ValueError naming the file otherwise"""
    if path.endswith('.npy'):
        raise ValueError('%s: a .npy file in an image folder cannot be kept as 8-bit samples; drop "resident_u8" or convert the file' % path)
    h, w, mode = image_header(path)
    if mode != 'RGB':
        raise ValueError("%s: mode '%s' (grey, palette or alpha), which convert('RGB') would have to change; \"resident_u8\" takes 8-bit RGB files only" % (path, mode))
    return h, w


def load_resident_u8(lists, ds_opt, device=None, max_bytes=None, t0=None):
    """`resident_u8` store: lists {name: [paths]} -> (device, {name: [uint8 [H, W, 3] tensors]}), decoded once on `n_workers` threads (16 at most) by
    imgio.load_resident.  Cap: max_bytes, else `resident_max_bytes` of the options, else half of the device memory free right now; over it: MemoryError.  Logs once
    (logger 'base') the number of files, the bytes resident on this rank (every rank holds the whole set) and the construction time since t0."""
    t0 = time.perf_counter() if t0 is None else t0
    cap = max_bytes if max_bytes is not None else ds_opt.get('resident_max_bytes')
    dev, out = load_resident(list(lists.values()), device, threads=ds_opt.get('n_workers') or 1, max_bytes=cap,
                             remedy='drop "resident_u8" from datasets.train')
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)
    nbytes = sum(t.numel() for imgs in out for t in imgs)
    logging.getLogger('base').info('resident_u8 [{}]: {:d} files, {:,d} bytes resident in device memory on this rank, built in {:.2f} s'.format(
        ds_opt.get('name'), sum(len(v) for v in out), nbytes, time.perf_counter() - t0))
    return dev, dict(zip(lists, out)), nbytes


def assemble_u8(device, gather, ddm=None, down=None):
    """the launches of one `resident_u8` batch.  gather / down: lists of (uint8 image [H, W, 3], y0, x0, size, flags, destination [3, size, size] fp32 view) for
    dasr_gather_srn_u8 / dasr_crops_down4_u8 (for `down` the window is given in the x1/4 image); ddm: (CropDesc array, channels, size, destination) for dasr_gather_crops.
    ALL descriptors cross in one imgio.upload; no host synchronisation.  Returns the device block (kept by the caller)."""
    n_g, n_d = len(gather), len(down or ())
    descs = (_lib.SrnU8Desc * (n_g + n_d))()
    for k, (img, y0, x0, size, flags, dst) in enumerate(list(gather) + list(down or ())):
        H, W = img.shape[:2]
        Hv, Wv = (H, W) if k < n_g else (H // 4, W // 4)
        if not (0 <= y0 and y0 + size <= Hv and 0 <= x0 and x0 + size <= Wv and img.device == device and img.dtype == torch.uint8 and img.is_contiguous()
                and tuple(dst.shape) == (3, size, size) and dst.is_contiguous()):
            raise ValueError('crop descriptor outside its image: window %r of %d x %d' % ((y0, x0, size), Hv, Wv))
        d = descs[k]
        d.src, d.H, d.W, d.y0, d.x0, d.size, d.flags, d.dst = img.data_ptr(), H, W, y0, x0, size, flags, dst.data_ptr()
    dd, offsets = upload(device, descs, *([ddm[0]] if ddm else []))
    L, off_d = _lib.lib(), n_g * C.sizeof(_lib.SrnU8Desc)
    if n_g:
        _lib.check(L.dasr_gather_srn_u8(dd.data_ptr(), n_g, max(g[3] for g in gather), _stream()), 'dasr_gather_srn_u8')
    if ddm:
        _lib.check(L.dasr_gather_crops(dd.data_ptr() + offsets[1], len(ddm[0]), ddm[1], ddm[2], ddm[3].data_ptr(), _stream()), 'gather_crops')
    if n_d:   # (the entry point checks the host copy of its descriptors before it launches)
        _lib.check(L.dasr_crops_down4_u8(dd.data_ptr() + off_d, C.addressof(descs) + off_d, n_d, down[0][3], C.addressof(down4_weights()), _stream()), 'dasr_crops_down4_u8')
    return dd


class _DeviceBatches:
    """What the two training datasets share: the option parsing, the size checks of the `resident_u8` store, util.augment's three coins, the fp32-store batch and the
    iteration in batches over the `count_key` list of the subclass.  A subclass reads its folders, draws a sample and lays out its batch."""
    count_key = None

    def __init__(self, ds_opt, scale, images, shuffle, drop_last):
        self.opt, self.scale, self.drop_last = ds_opt, scale, drop_last
        self.n, self.hr_size = int(ds_opt['batch_size']), int(ds_opt['HR_size'])
        self.use_flip, self.use_rot = bool(ds_opt.get('use_flip')), bool(ds_opt.get('use_rot'))
        self.shuffle = bool(ds_opt.get('use_shuffle')) if shuffle is None else shuffle
        self.resident = bool(ds_opt.get('resident_u8'))
        if self.resident and images is not None:
            raise ValueError('images=: "resident_u8" reads the dataroot_* folders itself (decoded bytes); pass images without the key')

    def _store_f32(self, images):
        self.img = {k: [t.to(self.device, torch.float32).contiguous() for t in v] for k, v in images.items()}

    def _checked_sizes(self, lists, least, lr_key):
        """{name: [(H, W)]} of the files of lists {name: [paths]}, from their headers (_u8_header refuses what cannot be kept as bytes).  The u8 kernels clamp a window
        that leaves its image where the fp32 one writes zeros, so a file smaller than its window (least[name]) is refused here, and so is an HR file smaller than
        scale x its `lr_key` file."""
        s = self.scale
        sizes = {k: [_u8_header(p) for p in v] for k, v in lists.items()}
        for k in lists:
            for p, (h, w) in zip(lists[k], sizes[k]):
                if h < least.get(k, 0) or w < least.get(k, 0):
                    raise ValueError('%s: image %dx%d is smaller than the crop size %d' % (p, h, w, least[k]))
        for p, (h, w), (hl, wl) in zip(lists['HR'], sizes['HR'], sizes.get(lr_key, ())):
            if h < s * hl or w < s * wl:
                raise ValueError('%s: %dx%d is smaller than %d x its LR image (%dx%d)' % (p, h, w, s, hl, wl))
        return sizes

    def _coins(self):
        """util.augment's coins as the flag bits of the kernels: hflip 1, vflip 2, transpose 4.  random.random() is drawn only for a switch that is on"""
        hflip = self.use_flip and random.random() < 0.5
        vflip = self.use_rot and random.random() < 0.5
        rot90 = self.use_rot and random.random() < 0.5
        return int(hflip) | (int(vflip) << 1) | (int(rot90) << 2)

    def _batch_f32(self, tensors):
        """the fp32-store batch.  tensors: [(key, channels, size, [(image, virt, y0, x0, flags) per sample])] (the arguments of fill_crop_desc): every CropDesc array
        crosses in ONE imgio.upload, then one dasr_gather_crops launch per tensor; no host synchronisation"""
        arrays = []
        for _, _, _, crops in tensors:
            arrays.append((_lib.CropDesc * len(crops))())
            for d, crop in zip(arrays[-1], crops):
                fill_crop_desc(d, *crop)
        dd, offsets = upload(self.device, *arrays)
        L, out = _lib.lib(), {'_keep': [dd]}
        for (key, Cc, size, crops), off in zip(tensors, offsets):
            out[key] = torch.empty((len(crops), Cc, size, size), dtype=torch.float32, device=self.device)
            _lib.check(L.dasr_gather_crops(dd.data_ptr() + off, len(crops), Cc, size, out[key].data_ptr(), _stream()), 'gather_crops')
        return out

    def __len__(self):
        m = len(self.img[self.count_key])
        return m // self.n if self.drop_last else (m + self.n - 1) // self.n

    def __iter__(self):
        m = len(self.img[self.count_key])
        order = torch.randperm(m).tolist() if self.shuffle else list(range(m))   # DataLoader(shuffle=True): RandomSampler draws from torch's global generator
        for b in range(len(self)):
            idx = order[b * self.n:(b + 1) * self.n]
            if idx:
                yield self.batch(idx)


class DeviceUnpairedDataset(_DeviceBatches):
    """Iterable of batch dicts {'LR_fake','LR_real','HR','HR_unpair','fake_w'} (CUDA tensors) built on the device.

    images: dict with lists of CHW fp32 tensors 'fake_LR', 'real_LR', 'HR' and 'fake_w' ([1,h',w'] domain-distance maps, any size)
    -- or None to read `dataroot_*` folders of `ds_opt` (PNG / .npy files)."""
    count_key = 'fake_LR'

    def __init__(self, ds_opt, scale=4, images=None, device=None, shuffle=None, drop_last=True, max_bytes=None):
        super().__init__(ds_opt, scale, images, shuffle, drop_last)
        folders = (('fake_LR', 'dataroot_fake_LR'), ('real_LR', 'dataroot_real_LR'), ('HR', 'dataroot_HR'), ('fake_w', 'dataroot_fake_weights'))
        LRs = self.hr_size // scale
        self.shapes = (('LR_fake', 3, LRs), ('LR_real', 3, LRs), ('HR', 3, self.hr_size), ('HR_unpair', 3, self.hr_size), ('fake_w', 1, LRs))
        if self.resident:   # the three image folders as bytes, the domain-distance maps as fp32 (dasr_gather_crops resizes them bilinearly)
            t0 = time.perf_counter()
            lists = {k: image_paths(ds_opt[r]) for k, r in folders[:3]}
            self._checked_sizes(lists, {'fake_LR': LRs, 'real_LR': LRs, 'HR': self.hr_size}, 'fake_LR')
            self.device, self.img, self.resident_bytes = load_resident_u8(lists, ds_opt, device, max_bytes, t0)
            self.img['fake_w'] = [load_image(p).to(self.device, torch.float32).contiguous() for p in image_paths(ds_opt[folders[3][1]])]
        else:
            self.device = device_of(device)
            self._store_f32(images if images is not None else {k: [load_image(p) for p in image_paths(ds_opt[r])] for k, r in folders})
        assert self.img['HR'], 'Error: HR path is empty.'
        assert len(self.img['fake_LR']) == len(self.img['HR']) == len(self.img['fake_w'])

    def sample(self, index):
        """descriptor of one sample; consumes the RNGs exactly like the reference's __getitem__ (train phase)"""
        s, HRs = self.scale, self.hr_size
        LRs = HRs // s
        index_real = np.random.randint(0, len(self.img['real_LR']))
        index_unpair = np.random.randint(0, len(self.img['HR']))
        lf, lr_, hr, hu, fw = (self.img['fake_LR'][index], self.img['real_LR'][index_real], self.img['HR'][index], self.img['HR'][index_unpair],
                               self.img['fake_w'][index])
        H, W = _hw(lf)
        Hr, Wr = _hw(lr_)
        y_f, x_f = random.randint(0, max(0, H - LRs)), random.randint(0, max(0, W - LRs))
        y_r, x_r = random.randint(0, max(0, Hr - LRs)), random.randint(0, max(0, Wr - LRs))
        Hu, Wu = _hw(hu)
        y_u, x_u = random.randint(0, max(0, Hu - HRs)), random.randint(0, max(0, Wu - HRs))
        return {'LR_fake': (lf, None, y_f, x_f), 'LR_real': (lr_, None, y_r, x_r), 'HR': (hr, None, y_f * s, x_f * s), 'HR_unpair': (hu, None, y_u, x_u),
                'fake_w': (fw, (H, W), y_f, x_f), 'flags': self._coins()}

    def batch(self, indices):
        samples = [self.sample(i) for i in indices]
        if not self.resident:
            return self._batch_f32([(key, Cc, size, [smp[key] + (smp['flags'],) for smp in samples]) for key, Cc, size in self.shapes])
        out = {key: torch.empty((len(samples), Cc, size, size), dtype=torch.float32, device=self.device) for key, Cc, size in self.shapes}
        gather = [(smp[key][0], smp[key][2], smp[key][3], size, smp['flags'], out[key][k]) for key, _, size in self.shapes[:4] for k, smp in enumerate(samples)]
        descs = (_lib.CropDesc * len(samples))()
        for d, smp in zip(descs, samples):
            fill_crop_desc(d, *smp['fake_w'], smp['flags'])
        out['_keep'] = [assemble_u8(self.device, gather, ddm=(descs, 1, self.shapes[4][2], out['fake_w']))]
        return out


def _bicubic_resample_matrix(n_in, scale):
    """(n_out x n_in) matrix of MATLAB's imresize along one axis: the taps of bicubic_taps scattered into one dense float64 matrix (the per-row products of imresize_np,
    codes/SRN/data/util.py:367-433)."""
    j, w = bicubic_taps(n_in, scale)
    M = torch.zeros(j.shape[0], n_in, dtype=torch.float64)
    M.scatter_add_(1, j, w)
    return M


def imresize_matlab(img, scale):
    """MATLAB-style bicubic resize with antialiasing of a CHW float tensor by `scale` (both axes; rows first, as the reference): the LR images of `mode: "LRHR"` datasets
    without an LR folder (codes/SRN/data/LRHR_dataset.py:85, util.imresize_np).  Pinned by tests/golden/imresize.npz (generated by the reference's function)."""
    C_, H, W = img.shape
    Mh, Mw = _bicubic_resample_matrix(H, scale), _bicubic_resample_matrix(W, scale)
    x = img.to(torch.float64)
    return torch.einsum('oh,chw,pw->cop', Mh, x, Mw).to(img.dtype)


class DevicePairedDataset(_DeviceBatches):
    """`mode: "LRHR"` with LR files given (codes/SRN/data/LRHR_dataset.py:44-126, train phase): {'LR','HR'} batches assembled on the
    device.  Per sample the reference draws random.randint twice (crop origin in the LR image) and then util.augment's coins.
    Without `dataroot_LR` the LR images are made from the HR images by MATLAB-style bicubic down-sampling (imresize_matlab), once, at construction: the reference's train
    phase does the same per sample with random_scale_list = [1] (LRHR_dataset.py:63-88) whenever the HR size is a multiple of `scale` -- the case taken here; other sizes
    go through cv2.resize(INTER_LINEAR) there first, and an HR image smaller than HR_size is resized: both stay on the reference's side (NotImplementedError).
    Under `resident_u8` without LR files nothing is made at construction: dasr_crops_down4_u8 makes the LR crops per batch from the HR bytes (img['LR'] is None)."""
    count_key = 'HR'

    def __init__(self, ds_opt, scale=4, images=None, device=None, shuffle=None, drop_last=True, max_bytes=None):
        super().__init__(ds_opt, scale, images, shuffle, drop_last)
        if self.resident:
            t0 = time.perf_counter()
            lists = {'HR': self.hr_paths(ds_opt)}
            if ds_opt.get('dataroot_LR'):
                lists['LR'] = image_paths(ds_opt['dataroot_LR'])
            elif scale != 4 or self.hr_size // scale > 128:
                raise NotImplementedError('"resident_u8" without dataroot_LR: the LR crops are made on the device for scale 4 and LR crops up to 128 x 128 (got scale %d, '
                                          'HR_size %d); provide LR files or drop "resident_u8"' % (scale, self.hr_size))
            sizes = self._checked_sizes(lists, {'LR': self.hr_size // scale}, 'LR')
            if 'LR' not in lists:
                for h, w in sizes['HR']:
                    self._check_multiple(h, w)
            self.device, self.img, self.resident_bytes = load_resident_u8(lists, ds_opt, device, max_bytes, t0)
            self.img.setdefault('LR', None)
        else:
            paths_HR = self.hr_paths(ds_opt) if images is None else None
            self.device = device_of(device)
            if images is None:
                hr = [load_image(p) for p in paths_HR]
                images = {'HR': hr, 'LR': [load_image(p) for p in image_paths(ds_opt['dataroot_LR'])] if ds_opt.get('dataroot_LR') else None}
            if images.get('LR') is None:   # down-sampling on the fly (LRHR_dataset.py:63-88)
                for t in images['HR']:
                    self._check_multiple(t.shape[1], t.shape[2])
                images = dict(images, LR=[imresize_matlab(t.float().cpu(), 1.0 / scale) for t in images['HR']])
            self._store_f32(images)
        assert self.img['HR'], 'Error: HR path is empty.'
        if self.img['LR'] is not None:
            assert len(self.img['LR']) == len(self.img['HR']), 'HR and LR datasets have different number of images - {}, {}.'.format(
                len(self.img['LR']), len(self.img['HR']))

    @staticmethod
    def hr_paths(ds_opt):
        """the HR files: the folder, or the names `subset_file` lists under it (LRHR_dataset.py:26-31: train phase, and only when the LR images are made on the fly)"""
        if ds_opt.get('subset_file') is not None and ds_opt.get('phase', 'train') == 'train':
            with open(ds_opt['subset_file']) as f:
                paths = sorted([os.path.join(ds_opt['dataroot_HR'], line.rstrip('\n')) for line in f])
            if ds_opt.get('dataroot_LR') is not None:
                raise NotImplementedError('Now subset only supports generating LR on-the-fly.')
            return paths
        return image_paths(ds_opt['dataroot_HR'])

    def _check_multiple(self, H, W):
        if H % self.scale or W % self.scale:
            raise NotImplementedError('LRHR without dataroot_LR: HR image of %d x %d is not a multiple of scale %d (the reference resizes it with cv2 first); '
                                      'crop the HR images or provide LR files' % (H, W, self.scale))

    def _draw(self, idx):
        """(y0, x0, flags) of sample idx: the crop origin in the LR image, then util.augment's three coins"""
        s, HRs = self.scale, self.hr_size
        LRs = HRs // s
        Hh, Wh = _hw(self.img['HR'][idx])
        if Hh < HRs or Wh < HRs:
            raise NotImplementedError('HR image smaller than HR_size (the reference resizes it and re-derives LR by imresize on the host)')
        Hl, Wl = _hw(self.img['LR'][idx]) if self.img['LR'] is not None else (Hh // s, Wh // s)
        y0, x0 = random.randint(0, max(0, Hl - LRs)), random.randint(0, max(0, Wl - LRs))
        return y0, x0, self._coins()

    def batch(self, indices):
        s, HRs = self.scale, self.hr_size
        LRs, n = HRs // s, len(indices)
        draws = [(idx,) + self._draw(idx) for idx in indices]
        if not self.resident:
            return self._batch_f32([('LR', 3, LRs, [(self.img['LR'][i], None, y0, x0, flags) for i, y0, x0, flags in draws]),
                                    ('HR', 3, HRs, [(self.img['HR'][i], None, y0 * s, x0 * s, flags) for i, y0, x0, flags in draws])])
        out = {'LR': torch.empty((n, 3, LRs, LRs), dtype=torch.float32, device=self.device),
               'HR': torch.empty((n, 3, HRs, HRs), dtype=torch.float32, device=self.device)}
        made = self.img['LR'] is None   # the LR crops come from the HR bytes: dasr_crops_down4_u8
        gather = [(self.img['HR'][i], y0 * s, x0 * s, HRs, flags, out['HR'][k]) for k, (i, y0, x0, flags) in enumerate(draws)]
        lr_plans = [(self.img['HR' if made else 'LR'][i], y0, x0, LRs, flags, out['LR'][k]) for k, (i, y0, x0, flags) in enumerate(draws)]
        out['_keep'] = [assemble_u8(self.device, gather, down=lr_plans) if made else assemble_u8(self.device, lr_plans + gather)]
        return out


# ---- evaluation / validation folders (`mode: "LRHR"` in the val / test phase, `mode: "LR"`) -----------------------------------------
def eval_folder_check_options(ds_opt):
    """what the val / test datasets of the reference can be asked for and this one does not do: one NotImplementedError each, before any file is touched"""
    mode = ds_opt.get('mode')
    if mode not in ('LRHR', 'LR'):
        raise NotImplementedError('EvalFolderDataset reads mode "LRHR" (val / test phase) and mode "LR", not [{}]'.format(mode))
    if ds_opt.get('data_type') == 'lmdb':
        raise NotImplementedError('data_type "lmdb" is not read here: unpack the database into a folder of image files')
    if ds_opt.get('color') is not None:
        raise NotImplementedError('color "{}": colour-space conversion of the inputs (channel_convert) is not implemented; leave `color` null'.format(ds_opt['color']))
    if ds_opt.get('subset_file') is not None:
        raise NotImplementedError('subset_file is a training-phase list (LRHR_dataset.py:26-31); the val / test datasets read whole folders')


def eval_folder_pairs(ds_opt):
    """(HR paths or None, LR paths or None) of a val / test dataset: each folder listed by image_paths (sorted), paired by index, with the reference's assertions
    (LRHR_dataset.py:33-40, LR_dataset.py:17-18).  An LRHR set whose LR folder is missing or lists nothing makes its LR images from the HR images, like the reference."""
    eval_folder_check_options(ds_opt)

    def listing(key):
        root = ds_opt.get(key)
        if root is None:
            return None
        assert os.path.isdir(root), '{:s} is not a valid directory'.format(root)
        return image_paths(root)
    if ds_opt['mode'] == 'LR':
        paths_LR = listing('dataroot_LR')
        assert paths_LR, 'Error: LR paths are empty.'
        return None, paths_LR
    paths_HR, paths_LR = listing('dataroot_HR'), listing('dataroot_LR')
    assert paths_HR, 'Error: HR path is empty.'
    if paths_LR:
        assert len(paths_LR) == len(paths_HR), 'HR and LR datasets have different number of images - {}, {}.'.format(len(paths_LR), len(paths_HR))
    return paths_HR, (paths_LR or None)


def modcrop_size(H, W, scale):
    """size of the window util.modcrop keeps (data/util.py:133-145): H % scale bottom rows and W % scale right columns go"""
    return H - H % scale, W - W % scale


class EvalFolderDataset:
    """The val / test phase of `mode: "LRHR"` (codes/SRN/data/LRHR_dataset.py:44-126) and `mode: "LR"` (LR_dataset.py) over folders of image files: an iterable with a
    length whose items are batches of one, {'LR' [1,3,h,w], 'HR' [1,3,H,W] (LRHR only), 'LR_path', 'HR_path' (lists of one string)}, fp32 on the device.

    Per item the file is decoded by PIL on the host (RGB, uint8), its BYTES are uploaded, and csrc/imgio.hip does the rest: dasr_u8_to_planar gives the planar fp32
    image in [0, 1] (bit for bit load_image), cropped to a multiple of `scale` for HR (modcrop); without LR files the LR image is dasr_imresize_down of the cropped HR
    (MATLAB bicubic with antialiasing, the fp64 taps of bicubic_taps, one rounding to fp32: within one fp32 unit of imresize_matlab).  .npy files (CHW or 1CHW float
    arrays, as load_image reads them) are uploaded as they are.  Nothing is kept across items but the fp64 intermediate per shape (the tap tables per length and scale are imgio.tap_table's)."""

    def __init__(self, ds_opt, scale=4, device=None):
        self.opt, self.scale = ds_opt, int(scale)
        self.mode = ds_opt.get('mode')
        self.paths_HR, self.paths_LR = eval_folder_pairs(ds_opt)
        self._device = device
        self._tmp = {}

    def __len__(self):
        return len(self.paths_HR if self.paths_HR is not None else self.paths_LR)

    @property
    def device(self):
        if not isinstance(self._device, torch.device):   # resolved on first use: listing and pairing (the constructor) need no GPU
            self._device = device_of(self._device)
        return self._device

    @staticmethod
    def decode(path):
        """host part of reading one file: the uint8 [H, W, 3] RGB array PIL decodes (a .npy file: the CHW fp32 tensor load_image gives)"""
        return load_image(path) if path.endswith('.npy') else decode_u8(path)

    def to_device(self, a, crop_to=None, path='image'):
        """decoded image -> [1, 3, Hc, Wc] fp32 on the device; crop_to: the scale whose multiple the size is cut down to (modcrop), None: the whole image"""
        H, W = a.shape[1:] if torch.is_tensor(a) else a.shape[:2]
        Hc, Wc = modcrop_size(H, W, crop_to) if crop_to else (H, W)
        if Hc < 1 or Wc < 1:
            raise ValueError('{}: {} x {} is smaller than the scale {}'.format(path, H, W, crop_to))
        if torch.is_tensor(a):
            return a.to(self.device)[:, :Hc, :Wc].contiguous()[None]
        return planar_f32(a, self.device, window=(Hc, Wc), batch=True)     # one byte per sample crosses to the device

    def _read(self, path, crop_to=None):
        return self.to_device(self.decode(path), crop_to, path)

    def downsample(self, img):
        """[1, C, H, W] (or [C, H, W]) fp32 device image with H and W multiples of scale -> [1, C, H / scale, W / scale]: dasr_imresize_down"""
        x = (img if img.dim() == 4 else img[None]).to(self.device, torch.float32).contiguous()
        n, c, H, W = x.shape
        s = self.scale
        if n != 1:
            raise ValueError('downsample takes one image, got a batch of %d' % n)
        if s not in (2, 3, 4) or H % s or W % s:
            raise NotImplementedError('LR images are made on the fly for scale 2, 3 or 4 and sizes that are multiples of it (got scale %d, %d x %d); provide LR files' % (s, H, W))
        tmp = self._tmp.get((c, H, W))
        if tmp is None:
            self._tmp = {(c, H, W): torch.empty((c, H // s, W), dtype=torch.float64, device=self.device)}   # one shape at a time: a folder of mixed sizes does not pile them up
            tmp = self._tmp[(c, H, W)]
        out = torch.empty((1, c, H // s, W // s), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().dasr_imresize_down(x.data_ptr(), c, H, W, s, *down_table_ptrs(H, W, s, self.device), tmp.data_ptr(), out.data_ptr(), _stream()),
                   'dasr_imresize_down')
        return out

    def item(self, index):
        if self.mode == 'LR':
            return {'LR': self._read(self.paths_LR[index]), 'LR_path': [self.paths_LR[index]]}
        s = self.scale
        HR_path = self.paths_HR[index]
        hr = self._read(HR_path, crop_to=s)
        if self.paths_LR:
            LR_path = self.paths_LR[index]
            lr = self._read(LR_path)
            if (lr.shape[2] * s, lr.shape[3] * s) != tuple(hr.shape[2:]):
                raise ValueError('{} ({} x {} after the crop to a multiple of {}) is not {} x the size of {} ({} x {})'.format(
                    HR_path, hr.shape[2], hr.shape[3], s, s, LR_path, lr.shape[2], lr.shape[3]))
        else:
            LR_path = HR_path            # LRHR_dataset.py:123-124
            lr = self.downsample(hr)
        return {'LR': lr, 'HR': hr, 'LR_path': [LR_path], 'HR_path': [HR_path]}

    def __iter__(self):
        for i in range(len(self)):
            yield self.item(i)
