"""Image-folder datasets of the DSN training driver (the caller side of codes/DSN/train.py:81-121): the host half of the hand-off to
`DSNModel.iteration(hr, bicubic_lr, real_lr)`.

    TrainDeresnetDataset   codes/DSN/data_loader.py:12-59    (clean HR crop, its bicubic x1/4 image, a crop/4 crop of a source-domain image)
    ValDeresnetDataset     codes/DSN/data_loader.py:157-190  (HR centre crop, its bicubic x1/4 image, a random and the centre crop of the paired LR)
    imresize               codes/DSN/utils.py:37-160         (MATLAB-style bicubic with antialiasing, clamped to [0, 1])
    display_transform      codes/DSN/utils.py:25-31          (validation image strips: Resize(400) + CenterCrop(400))

The reference builds these on PIL + torchvision transforms; torchvision is not a dependency here.  Images are decoded with PIL and handled as
CHW float tensors in [0, 1] (`to_tensor` semantics); flips / crops / quarter-turn rotations are tensor ops driven by python's `random` (the
reference's transforms draw from torch's and python's global generators: the crops are random either way, no stream is reproduced).  `imresize`
is evaluated as two dense resampling matrices (rows = output pixels, symmetric boundary folded into the columns) instead of the reference's
per-row loops: same weights, same result up to fp32 summation order (tests/test_dsn_data.py pins it against vectors of the reference function).

`--device_data` (DeviceTrainDeresnet, DeviceValDeresnet, DeviceDeresnetLoader): the same batches assembled on the GPU.  Every file is decoded ONCE and its
bytes stay resident in device memory; per item the host only draws the random numbers (`plan_item`, the calls of the host datasets in their order, so equal
seeds give equal batches) and a batch is one descriptor upload and three launches of csrc/imgio.hip (clean crops, source crops, the bicubic image), with no
host synchronisation.  hr and real are bit-equal to the host path, bicubic is the fp64 evaluation rounded once (within one fp32 unit of it, and of the host's image within that
plus the host's own fp32 error).  The decode, the resident store, the tap tables and the descriptor upload are imgio.py's, shared with data.py.
"""
import collections
import math
import os
import random

import numpy as np
import torch

from . import _lib
from .engine import _stream
from .imgio import decode_u8, image_size, load_resident, tap_table, u8_to_chw, upload

IMG_EXTENSIONS = ('.png', '.jpg', '.jpeg', '.PNG', '.JPG', '.JPEG')
DERESNET_DATASETS = ('aim2019', 'ntire2020', 'realsr', 'camerasr')   # codes/DSN/train.py:84-115: the branches whose loaders return (hr, bicubic, real) triples


def is_image_file(filename):
    return filename.endswith(IMG_EXTENSIONS)


def calculate_valid_crop_size(crop_size, upscale_factor):
    return crop_size - (crop_size % upscale_factor)


def _cubic(x):
    a = x.abs()
    a2, a3 = a * a, a * a * a
    return (1.5 * a3 - 2.5 * a2 + 1) * (a <= 1).to(x.dtype) + (-0.5 * a3 + 2.5 * a2 - 4 * a + 2) * ((a > 1) & (a <= 2)).to(x.dtype)


# resize_matrix / imresize evaluate the weights in fp32, as the reference's function does: tests/test_dsn_data.py pins the host loader's bicubic image to the reference's
# own vectors.  imgio.bicubic_taps is the same kernel in fp64 (the device tables); building this matrix from it would change bits of every host batch.  Keep the two apart.
def resize_matrix(in_length, scale, antialiasing=True, dtype=torch.float32):
    """[out_length, in_length] matrix of the 1-D bicubic resampling of utils.py:46-98: output pixel k takes the kernel (stretched by 1 / scale when
    shrinking with antialiasing) centred on u = k / scale + 0.5 (1 - 1 / scale), weights normalised per output pixel, taps outside the image
    mirrored back in (symmetric extension including the edge pixel)."""
    out_length = math.ceil(in_length * scale)
    kernel_width = 4.0
    shrink = scale < 1 and antialiasing
    if shrink:
        kernel_width = kernel_width / scale
    x = torch.arange(1, out_length + 1, dtype=dtype)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = torch.floor(u - kernel_width / 2)
    P = math.ceil(kernel_width) + 2
    idx = left[:, None] + torch.arange(P, dtype=dtype)[None, :]            # 1-based input coordinates of the taps
    dist = u[:, None] - idx
    w = scale * _cubic(dist * scale) if shrink else _cubic(dist)
    w = w / w.sum(1, keepdim=True)
    j = idx.long() - 1                                                     # 0-based, may leave [0, in_length)
    j = torch.where(j < 0, -j - 1, j)                                      # symmetric: -1 -> 0, -2 -> 1
    j = torch.where(j >= in_length, 2 * in_length - 1 - j, j)              # in_length -> in_length - 1
    j = j.clamp(0, in_length - 1)                                          # (zero-weight taps further out)
    R = torch.zeros(out_length, in_length, dtype=dtype)
    R.scatter_add_(1, j, w)
    return R


def imresize(img, scale, antialiasing=True):
    """img CHW in [0, 1] -> CHW [C, ceil(H scale), ceil(W scale)], rows first then columns, clamped to [0, 1] (utils.py:101-160)"""
    img = img.float()
    Rh = resize_matrix(img.shape[1], scale, antialiasing)
    Rw = resize_matrix(img.shape[2], scale, antialiasing)
    out = torch.matmul(torch.matmul(Rh, img), Rw.t())
    return out.clamp(0, 1)


def open_image(path):
    """file -> CHW fp32 RGB in [0, 1] (Image.open + to_tensor; grey / palette / alpha files are converted to RGB)"""
    return u8_to_chw(decode_u8(path))


def _list_images(dirs):
    if isinstance(dirs, str):
        dirs = [dirs]
    files = []
    for d in dirs:
        files += [os.path.join(d, x) for x in os.listdir(d) if is_image_file(x)]
    return files


def random_crop(img, size):
    """T.RandomCrop(size) on a CHW tensor"""
    _, h, w = img.shape
    if h < size or w < size:
        raise ValueError('image %dx%d is smaller than the crop size %d' % (h, w, size))
    y, x = random.randint(0, h - size), random.randint(0, w - size)
    return img[:, y:y + size, x:x + size]


def _centre(h, w, size):
    """(y, x) of the window T.CenterCrop(size) keeps of an h x w image (torchvision rounds the offsets): center_crop and DeviceValDeresnet"""
    if h < size or w < size:
        raise ValueError('image %dx%d is smaller than the crop size %d' % (h, w, size))
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def center_crop(img, size):
    """T.CenterCrop(size) on a CHW tensor"""
    y, x = _centre(img.shape[1], img.shape[2], size)
    return img[:, y:y + size, x:x + size]


def _plan_window(h, w, crop, flips, rotations):
    """(y0, x0, flags) of one augmented crop: THE order of its draws, for the host loader (load_augmented_crop) and the device one (plan_item) -- randint y, randint x,
    the vflip coin (flags bit 0), the hflip coin (bit 1), the choice of quarter-turns (bits 2-3); the coins only with `flips`, the choice only with `rotations`"""
    y, x = random.randint(0, h - crop), random.randint(0, w - crop)
    vflip = flips and random.random() < 0.5
    hflip = flips and random.random() < 0.5
    k = random.choice([0, 1, 2, 3]) if rotations else 0
    return y, x, int(vflip) | (int(hflip) << 1) | (k << 2)


def load_augmented_crop(path, crop_size, flips, rotations):
    """RandomVerticalFlip, RandomHorizontalFlip (p = 0.5 when `flips`), RandomCrop(crop_size), then a quarter-turn by a random multiple of 90 degrees
    when `rotations` (TF.rotate of the square crop, counter-clockwise): data_loader.py:27-31,43-47 -- without converting the whole image to floats:
    the crop window is cut from the decoded 8-bit image first and the flips are applied to the crop (a uniformly random window of the flipped
    image = the flip of a uniformly random window)"""
    h, w = image_size(path)
    if h < crop_size or w < crop_size:
        raise ValueError('%s: image %dx%d is smaller than the crop size %d' % (path, h, w, crop_size))
    y, x, flags = _plan_window(h, w, crop_size, flips, rotations)
    img = u8_to_chw(decode_u8(path, (x, y, x + crop_size, y + crop_size)))
    if flags & 1:
        img = img.flip(1)
    if flags & 2:
        img = img.flip(2)
    if flags >> 2:
        img = torch.rot90(img, flags >> 2, (1, 2))
    return img.contiguous()


class TrainDeresnetDataset:
    """item -> (clean HR crop [3,c,c], its bicubic x1/upscale image, crop [3,c/up,c/up] of a source-domain image): data_loader.py:12-59 with
    `cropped=True`, as train.py:85-111 builds it (`noisy_dir` = the `source` folder(s), `cleandir` = the `target` folder(s) of paths.yml).
    The clean image is drawn at random per item, the epoch length is the number of source images."""

    def __init__(self, noisy_dir, cleandir, crop_size, upscale_factor=4, cropped=False, flips=False, rotations=False, **kwargs):
        self.noisy_dir_files = _list_images(noisy_dir)
        self.cleandir_files = _list_images(cleandir)
        if not self.noisy_dir_files or not self.cleandir_files:
            raise FileNotFoundError('no image files under %s / %s' % (noisy_dir, cleandir))
        self.crop_size, self.upscale_factor = int(crop_size), int(upscale_factor)
        self.cropped, self.flips, self.rotations = bool(cropped), bool(flips), bool(rotations)

    def __len__(self):
        return len(self.noisy_dir_files)

    def __getitem__(self, index):
        index_clean = np.random.randint(0, len(self.cleandir_files))
        noisy = load_augmented_crop(self.noisy_dir_files[index], self.crop_size, self.flips, self.rotations)
        clean = load_augmented_crop(self.cleandir_files[index_clean], self.crop_size, self.flips, self.rotations)
        resized = imresize(clean, 1.0 / self.upscale_factor, True)
        if self.cropped:
            return clean, resized, random_crop(noisy, self.crop_size // self.upscale_factor).contiguous()
        return resized


class ValDeresnetDataset:
    """item -> (HR centre crop, its bicubic x1/upscale image, random LR crop, centre LR crop) of the sorted file pair `index`:
    data_loader.py:157-190.  cs = min(w, h) rounded down to a multiple of the factor, capped by crop_size_val."""

    def __init__(self, hr_dir, upscale_factor, lr_dir=None, crop_size_val=None, **kwargs):
        self.hr_files = sorted(_list_images(hr_dir))
        self.lr_files = None if lr_dir is None else sorted(_list_images(lr_dir))
        self.upscale_factor, self.crop_size = int(upscale_factor), crop_size_val
        if self.lr_files is None:
            raise NotImplementedError('Val_Deresnet_Dataset without lr_dir returns an undefined name in the reference (data_loader.py:180-181)')

    def __len__(self):
        return len(self.hr_files)

    def __getitem__(self, index):
        hr = open_image(self.hr_files[index])
        cs = calculate_valid_crop_size(min(hr.shape[1], hr.shape[2]), self.upscale_factor)
        if self.crop_size is not None:
            cs = min(cs, int(self.crop_size))
        hr = center_crop(hr, cs).contiguous()
        resized = imresize(hr, 1.0 / self.upscale_factor, True)
        lr = open_image(self.lr_files[index])
        return hr, resized, random_crop(lr, cs // self.upscale_factor).contiguous(), center_crop(lr, cs // self.upscale_factor).contiguous()


class ShardSampler:
    """sampler of torch.utils.data.DataLoader: a new permutation per epoch (shuffle=True of train.py:87), of which data-parallel rank r walks the
    strided share r, r + world, ... (every rank draws the SAME permutation from `seed + epoch`; equal item counts on every rank)"""

    def __init__(self, n, shuffle=True, seed=0, rank=0, world=1):
        self.n, self.shuffle, self.seed, self.rank, self.world, self.epoch = n, shuffle, seed, rank, world, 0

    def __len__(self):
        return self.n // self.world if self.world > 1 else self.n

    def __iter__(self):
        order = list(range(self.n))
        if self.shuffle:
            random.Random(self.seed + self.epoch).shuffle(order)
        self.epoch += 1
        if self.world > 1:   # every rank must run the same number of iterations (collectives): the n % world left-over items sit out this epoch
            order = order[:self.n // self.world * self.world]
        return iter(order[self.rank::self.world])


def make_loader(dataset, batch_size, shuffle, num_workers=0, seed=0, rank=0, world=1):
    """DataLoader(dataset, num_workers, batch_size, shuffle) of train.py:87,90 (drop_last=False: the last batch of an epoch may be short); under data
    parallelism the per-rank batch is batch_size // world"""
    from torch.utils.data import DataLoader
    return DataLoader(dataset, batch_size=max(1, int(batch_size) // world), sampler=ShardSampler(len(dataset), shuffle, seed, rank, world),
                      num_workers=int(num_workers))


def load_paths(path):
    import yaml
    with open(path, 'r') as f:
        return yaml.safe_load(f)


def _dataset_folders(o, paths):
    """(folders of the dataset's paths.yml entry, its target folder): camerasr takes its target folder from aim2019 (train.py:110)"""
    ds = o.dataset
    if ds not in DERESNET_DATASETS:
        raise NotImplementedError("dataset [%s]: the reference's training loop unpacks (hr, bicubic, real) triples, which only its aim2019 / ntire2020 / "
                                  "realsr / camerasr branches provide (train.py:84-115, 204); built in here: those four and 'synthetic'" % ds)
    src = paths[ds][o.artifacts]
    return src, paths['aim2019'][o.artifacts]['target'] if ds == 'camerasr' else src['target']


def make_datasets(o, paths):
    """train.py:84-115: the four `Train_Deresnet_Dataset` branches"""
    src, target = _dataset_folders(o, paths)
    kw = dict(crop_size=o.crop_size, upscale_factor=o.upscale_factor, flips=o.flips, rotations=o.rotations)
    train_set = TrainDeresnetDataset(src['source'], target, cropped=True, **kw)
    val_set = ValDeresnetDataset(src['valid_hr'], o.upscale_factor, lr_dir=src['valid_lr'], crop_size_val=o.crop_size_val)
    return train_set, val_set


# ---- --device_data: the same datasets on images resident in device memory -------------------------------------------------------------
# one window of a resident image as dasr_gather_crops_u8 cuts it: `image` uint8 [H, W, 3]; the crop x crop window at (y0, x0), flipped vertically (flags bit 0),
# then horizontally (bit 1), then turned by k = bits 2-3 quarter-turns (torch.rot90(., k, (1, 2))); of that the size x size window at (sub_y, sub_x)
CropPlan = collections.namedtuple('CropPlan', 'image y0 x0 crop flags sub_y sub_x size')


def _gather_u8(plan_groups, device):
    """one output tensor [n, 3, size, size] per group of CropPlans (equal `size` inside a group): ALL descriptors in one imgio.upload, one dasr_gather_crops_u8
    launch per group, no host synchronisation"""
    arrays = []
    for g in plan_groups:
        arrays.append((_lib.CropU8Desc * len(g))())
        for d, p in zip(arrays[-1], g):
            H, W = p.image.shape[:2]
            if not (0 <= p.y0 and p.y0 + p.crop <= H and 0 <= p.x0 and p.x0 + p.crop <= W and 0 <= p.sub_y and p.sub_y + p.size <= p.crop
                    and 0 <= p.sub_x and p.sub_x + p.size <= p.crop and p.image.device == device and p.image.dtype == torch.uint8 and p.image.is_contiguous()):
                raise ValueError('crop descriptor outside its image: %r of %d x %d' % (p[1:], H, W))
            d.src, d.H, d.W, d.y0, d.x0, d.crop, d.flags, d.sub_y, d.sub_x = p.image.data_ptr(), H, W, p.y0, p.x0, p.crop, p.flags, p.sub_y, p.sub_x
    dd, offsets = upload(device, *arrays)
    L, out = _lib.lib(), []
    for g, off in zip(plan_groups, offsets):
        size = g[0].size
        out.append(torch.empty((len(g), 3, size, size), dtype=torch.float32, device=device))
        _lib.check(L.dasr_gather_crops_u8(dd.data_ptr() + off, len(g), size, out[-1].data_ptr(), _stream()), 'dasr_gather_crops_u8')
    return out


def _check_bicubic_side(c, upscale_factor, what):
    """what dasr_crops_bicubic_down covers, asked before anything is decoded"""
    if int(upscale_factor) != 4 or c % 4 or c > 1024:
        raise NotImplementedError('%s: the bicubic image is made on the device for upscale_factor 4 and crops whose side is a multiple of 4 up to 1024 '
                                  '(got factor %d, side %d); use the host loader' % (what, upscale_factor, c))


class _BicubicDown:
    """dasr_crops_bicubic_down with the tap tables (imgio.tap_table) of the crop sides it has seen"""

    def __init__(self, upscale_factor, device):
        self.s, self.device, self._tables = int(upscale_factor), device, {}

    def __call__(self, hr):
        n, _, c, _ = hr.shape
        _check_bicubic_side(c, self.s, 'crops of side %d' % c)
        j, w = self._tables[c] = tap_table(c, self.s, self.device)
        out = torch.empty((n, 3, c // self.s, c // self.s), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().dasr_crops_bicubic_down(hr.data_ptr(), n, c, self.s, j.data_ptr(), w.data_ptr(), out.data_ptr(), _stream()), 'dasr_crops_bicubic_down')
        return out


class DeviceTrainDeresnet:
    """TrainDeresnetDataset(cropped=True) on images resident in device memory: the same file lists, the same random draws, batches made by `batch`
    (hr [n,3,c,c], bicubic [n,3,c/up,c/up], real [n,3,c/up,c/up] on the device).  See load_resident for `threads` and `max_bytes`."""

    def __init__(self, noisy_dir, cleandir, crop_size, upscale_factor=4, flips=False, rotations=False, device=None, threads=6, max_bytes=None):
        self.noisy_dir_files = _list_images(noisy_dir)
        self.cleandir_files = _list_images(cleandir)
        if not self.noisy_dir_files or not self.cleandir_files:
            raise FileNotFoundError('no image files under %s / %s' % (noisy_dir, cleandir))
        self.crop_size, self.upscale_factor = int(crop_size), int(upscale_factor)
        self.flips, self.rotations = bool(flips), bool(rotations)
        _check_bicubic_side(self.crop_size, self.upscale_factor, '--crop_size %d' % self.crop_size)
        self.device, (self.noisy, self.clean) = load_resident([self.noisy_dir_files, self.cleandir_files], device, threads, max_bytes, min_size=self.crop_size)
        self._down = _BicubicDown(self.upscale_factor, self.device)

    def __len__(self):
        return len(self.noisy)

    def plan_item(self, index):
        """(source-domain CropPlan, clean CropPlan) of item `index`: host only; consumes np.random and random exactly like TrainDeresnetDataset.__getitem__"""
        c, small = self.crop_size, self.crop_size // self.upscale_factor
        clean = self.clean[np.random.randint(0, len(self.clean))]
        noisy = self.noisy[index]
        ny, nx, nflags = _plan_window(noisy.shape[0], noisy.shape[1], c, self.flips, self.rotations)
        cy, cx, cflags = _plan_window(clean.shape[0], clean.shape[1], c, self.flips, self.rotations)
        sy, sx = random.randint(0, c - small), random.randint(0, c - small)
        return CropPlan(noisy, ny, nx, c, nflags, sy, sx, small), CropPlan(clean, cy, cx, c, cflags, 0, 0, c)

    def batch(self, indices):
        plans = [self.plan_item(i) for i in indices]
        hr, real = _gather_u8([[p[1] for p in plans], [p[0] for p in plans]], self.device)
        return hr, self._down(hr), real


class DeviceValDeresnet:
    """ValDeresnetDataset on images resident in device memory: item -> (HR centre crop, its bicubic image, random LR crop, centre LR crop), the same
    draws (random.randint y, x of the random LR crop).  Iterating gives batches of one ([1,3,..] tensors), what make_loader(val_set, 1, False) yields."""

    def __init__(self, hr_dir, upscale_factor, lr_dir=None, crop_size_val=None, device=None, threads=6, max_bytes=None):
        self.hr_files = sorted(_list_images(hr_dir))
        if lr_dir is None:
            raise NotImplementedError('Val_Deresnet_Dataset without lr_dir returns an undefined name in the reference (data_loader.py:180-181)')
        self.lr_files = sorted(_list_images(lr_dir))
        self.upscale_factor, self.crop_size = int(upscale_factor), crop_size_val
        for hr_path, lr_path in zip(self.hr_files, self.lr_files):   # every item's sizes, from the file headers: refused here, not at the first validation pass
            cs = self._crop_side(*image_size(hr_path))
            _check_bicubic_side(cs, self.upscale_factor, hr_path)
            h, w = image_size(lr_path)
            if h < cs // self.upscale_factor or w < cs // self.upscale_factor:
                raise ValueError('%s: image %dx%d is smaller than the crop size %d' % (lr_path, h, w, cs // self.upscale_factor))
        self.device, (self.hr, self.lr) = load_resident([self.hr_files, self.lr_files], device, threads, max_bytes)
        self._down = _BicubicDown(self.upscale_factor, self.device)

    def _crop_side(self, h, w):
        cs = calculate_valid_crop_size(min(h, w), self.upscale_factor)
        return cs if self.crop_size is None else min(cs, int(self.crop_size))

    def __len__(self):
        return len(self.hr)

    def __getitem__(self, index):
        def centre(img, size):   # center_crop
            return CropPlan(img, *_centre(img.shape[0], img.shape[1], size), size, 0, 0, 0, size)
        hr, lr = self.hr[index], self.lr[index]
        cs = self._crop_side(hr.shape[0], hr.shape[1])
        small = cs // self.upscale_factor
        hr_plan = centre(hr, cs)
        h, w = lr.shape[:2]
        if h < small or w < small:
            raise ValueError('image %dx%d is smaller than the crop size %d' % (h, w, small))
        rnd = CropPlan(lr, random.randint(0, h - small), random.randint(0, w - small), small, 0, 0, 0, small)
        hr_t, lr_t = _gather_u8([[hr_plan], [rnd, centre(lr, small)]], self.device)
        return hr_t[0], self._down(hr_t)[0], lr_t[0], lr_t[1]

    def __iter__(self):
        for i in range(len(self)):
            yield tuple(t[None] for t in self[i])


class DeviceDeresnetLoader:
    """batches of a DeviceTrainDeresnet in the order of `sampler` (a ShardSampler: a new permutation per epoch, the rank's strided share), batch_size items
    each, the last batch of an epoch possibly short (drop_last=False): what make_loader yields, as device tensors"""

    def __init__(self, dataset, batch_size, sampler):
        self.dataset, self.batch_size, self.sampler = dataset, max(1, int(batch_size)), sampler

    def __len__(self):
        return (len(self.sampler) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = list(self.sampler)
        for k in range(0, len(order), self.batch_size):
            yield self.dataset.batch(order[k:k + self.batch_size])


def make_device_datasets(o, paths, device=None):
    """make_datasets for --device_data; --num_workers is the number of decode threads"""
    src, target = _dataset_folders(o, paths)
    train_set = DeviceTrainDeresnet(src['source'], target, o.crop_size, o.upscale_factor, flips=o.flips, rotations=o.rotations, device=device, threads=o.num_workers)
    val_set = DeviceValDeresnet(src['valid_hr'], o.upscale_factor, lr_dir=src['valid_lr'], crop_size_val=o.crop_size_val, device=device, threads=o.num_workers)
    return train_set, val_set


def display_transform(img, size=400):
    """utils.py:25-31: ToPILImage -> Resize(400) (shorter side, bilinear) -> CenterCrop(400) -> ToTensor, on a CHW tensor in [0, 1]"""
    from PIL import Image
    a = img.detach().float().cpu().mul(255).byte().permute(1, 2, 0).numpy()   # ToPILImage: mul(255).byte()
    im = Image.fromarray(a if a.shape[2] == 3 else a[:, :, 0])
    w, h = im.size
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    im = im.resize((nw, nh), Image.BILINEAR)
    x0, y0 = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
    im = im.crop((x0, y0, x0 + size, y0 + size))
    return u8_to_chw(np.array(im.convert('RGB'), dtype=np.uint8))
