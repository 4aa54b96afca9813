"""CPU: the device-side image-quality path (dasr_amd/metrics.py, csrc/metrics.hip) as far as it goes without a GPU -- the C ABI lists the new entry
points and rejects bad arguments before it launches anything, image_metrics hands images without a valid SSIM region to the host functions, and the
drivers touch the device path only when the option `device_metrics` asks for it."""
import logging
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dasr_tensor2img_u8', 'dasr_img_sse', 'dasr_img_ssim', 'dasr_img_ws_bytes')
EINVAL = -22


def test_metric_entry_points_are_bound_declared_and_exported():
    from dasr_amd import build, _lib
    hdr = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    declared = set(re.findall(r'^\s*int\s+(dasr_\w+)\s*\(', hdr, flags=re.M))
    for name in NEW:
        assert name in _lib._SIGS, name
        assert name in declared, name
    assert _lib.ABI_VERSION == 22 and '#define DASR_ABI_VERSION 22' in hdr
    assert 'metrics.hip' in build.SOURCES
    build.build()
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert '`%s`' % name in doc, name


def test_entry_points_reject_bad_arguments_before_any_launch():
    """null pointers, N <= 0, a channel count other than 1 / 3, a crop that leaves nothing and a cropped side under the 11-pixel window: DASR_EINVAL
    (checked in front of the first HIP call, so this runs without a device; the non-null pointers are never dereferenced)"""
    from dasr_amd import _lib
    L = _lib.lib()
    p = 4096   # stands for a device address
    assert L.dasr_img_ws_bytes(1, 3, 1356, 2040, 4) > 0
    assert L.dasr_img_ws_bytes(0, 3, 64, 64, 4) == EINVAL and L.dasr_img_ws_bytes(1, 2, 64, 64, 4) == EINVAL
    assert L.dasr_img_ws_bytes(1, 3, 8, 64, 4) == EINVAL
    assert L.dasr_tensor2img_u8(None, 1, 3, 8, 8, 0.0, 1.0, p, p, None, None) == EINVAL
    assert L.dasr_tensor2img_u8(p, 1, 3, 8, 8, 0.0, 1.0, None, None, None, None) == EINVAL
    assert L.dasr_tensor2img_u8(p, 0, 3, 8, 8, 0.0, 1.0, p, p, None, None) == EINVAL
    assert L.dasr_tensor2img_u8(p, 1, 3, 8, 8, 1.0, 1.0, p, p, None, None) == EINVAL
    ws = 1 << 20
    for fn, tail in ((L.dasr_img_sse, lambda a, b, out, w: (a, b, 1, 3, 64, 64, 4, out, None, w, ws, None)),
                     (L.dasr_img_ssim, lambda a, b, out, w: (a, b, 1, 3, 64, 64, 4, 0, out, w, ws, None))):
        assert fn(*tail(None, p, p, p)) == EINVAL and fn(*tail(p, None, p, p)) == EINVAL
        assert fn(*tail(p, p, None, p)) == EINVAL and fn(*tail(p, p, p, None)) == EINVAL
    assert L.dasr_img_sse(p, p, 0, 3, 64, 64, 4, p, None, p, ws, None) == EINVAL
    assert L.dasr_img_sse(p, p, 1, 3, 64, 64, 32, p, None, p, ws, None) == EINVAL     # nothing left of the image
    assert L.dasr_img_sse(p, p, 1, 1, 64, 64, 4, p, p, p, ws, None) == EINVAL         # Y of a one-channel image
    assert L.dasr_img_sse(p, p, 1, 3, 64, 64, 4, p, None, p, 8, None) == EINVAL        # workspace too small
    assert L.dasr_img_ssim(p, p, 0, 3, 64, 64, 4, 0, p, p, ws, None) == EINVAL
    assert L.dasr_img_ssim(p, p, 1, 3, 18, 64, 4, 0, p, p, ws, None) == EINVAL         # cropped height 10 < 11
    assert L.dasr_img_ssim(p, p, 1, 3, 64, 18, 4, 0, p, p, ws, None) == EINVAL
    assert L.dasr_img_ssim(p, p, 1, 1, 64, 64, 4, 1, p, p, ws, None) == EINVAL
    assert L.dasr_img_ssim(p, p, 1, 3, 64, 64, 4, 0, p, p, 8, None) == EINVAL


def _host_sequence(sr, hr, c):
    """what test.evaluate does on the host with the two fp32 images"""
    from dasr_amd import util
    a, b = util.tensor2img(sr) / 255., util.tensor2img(hr) / 255.
    ca, cb = a[c:-c, c:-c, :], b[c:-c, c:-c, :]
    out = OrderedDict(psnr=util.calculate_psnr(ca * 255, cb * 255))
    out['ssim'] = util.calculate_ssim(ca * 255, cb * 255)
    ay, by = util.bgr2ycbcr(a, only_y=True), util.bgr2ycbcr(b, only_y=True)
    out['psnr_y'] = util.calculate_psnr(ay[c:-c, c:-c] * 255, by[c:-c, c:-c] * 255)
    out['ssim_y'] = util.calculate_ssim(ay[c:-c, c:-c] * 255, by[c:-c, c:-c] * 255)
    return out


def test_image_metrics_hands_images_without_a_valid_region_to_the_host_functions(monkeypatch):
    """12 x 12 with crop 4: the cropped side (4) is under the 11-pixel window, the device SSIM has nothing to average and the host functions decide --
    today util.calculate_ssim refuses such an image with numpy's ValueError, and so does image_metrics; what the host functions return is passed on"""
    from dasr_amd import metrics, util
    g = torch.Generator().manual_seed(3)
    sr, hr = torch.rand(1, 3, 12, 12, generator=g), torch.rand(1, 3, 12, 12, generator=g)
    with pytest.raises(ValueError) as want:
        _host_sequence(sr[0], hr[0], 4)
    with pytest.raises(ValueError) as got:
        metrics.image_metrics(sr, hr, 4)
    assert str(got.value) == str(want.value)
    # whatever the host function returns is passed on, next to the host PSNR values
    calls = []
    monkeypatch.setattr(util, 'calculate_ssim', lambda a, b: calls.append(a.shape) or float('nan'))
    m = metrics.image_metrics(sr, hr, 4)
    assert calls == [(4, 4, 3), (4, 4)] and np.isnan(m['ssim']) and np.isnan(m['ssim_y'])
    a, b = util.tensor2img(sr) / 255., util.tensor2img(hr) / 255.
    assert m['psnr'] == util.calculate_psnr(a[4:-4, 4:-4] * 255, b[4:-4, 4:-4] * 255)
    ay, by = util.bgr2ycbcr(a, only_y=True), util.bgr2ycbcr(b, only_y=True)
    assert m['psnr_y'] == util.calculate_psnr(ay[4:-4, 4:-4] * 255, by[4:-4, 4:-4] * 255)
    # 19 x 40 with crop 4 (cropped height 11) is the smallest the device takes: on a CPU tensor that is an error, not a quiet host evaluation
    from dasr_amd._lib import DasrHipError
    with pytest.raises(DasrHipError):
        metrics.image_metrics(torch.rand(1, 3, 19, 40), torch.rand(1, 3, 19, 40), 4)


class _FakeModel:
    """the surface test.evaluate / train.validate use, on the CPU"""
    lpips_label = 'LPIPS'

    def __init__(self, device_path):
        self.device_path = device_path
        self.used = []

    def feed_data(self, data, need_HR=True):
        self.lr, self.hr = data['LR'], data.get('HR')

    def test(self):
        self.sr = torch.nn.functional.interpolate(self.lr, scale_factor=4, mode='nearest')

    def get_current_visuals(self, need_HR=True):
        self.used.append('visuals')
        out = OrderedDict(LR=self.lr[0], SR=self.sr[0])
        if need_HR and self.hr is not None:
            out['HR'] = self.hr[0]
        return out

    def current_sr_u8(self):
        assert self.device_path, 'device path used without the option'
        self.used.append('sr_u8')
        from dasr_amd import util
        return util.tensor2img(self.sr[0])

    def current_metrics(self, crop):
        assert self.device_path, 'device path used without the option'
        self.used.append('metrics')
        return dict(_host_sequence(self.sr[0], self.hr[0], crop))


def _loader(n=2):
    g = torch.Generator().manual_seed(11)
    for i in range(n):
        hr = torch.rand(1, 3, 48, 56, generator=g)
        yield {'LR': torch.nn.functional.avg_pool2d(hr, 4), 'HR': hr, 'LR_path': ['x/img_%d.png' % i], 'HR_path': ['x/img_%d.png' % i]}


def _capture_logger(name):
    lines = []

    class H(logging.Handler):
        def emit(self, rec):
            lines.append(rec.getMessage())
    lg = logging.getLogger(name)
    lg.setLevel(logging.INFO)
    lg.propagate = False
    lg.handlers = [H()]
    return lg, lines


def test_drivers_use_the_device_path_only_when_asked(tmp_path, monkeypatch):
    """`device_metrics` absent: test.evaluate and train.validate never import dasr_amd.metrics and never call the trainer's device entry points; set: the PNG
    comes from current_sr_u8 and the numbers from current_metrics, with the same log lines and result dict"""
    from dasr_amd import options, test as dtest, train
    monkeypatch.setitem(sys.modules, 'dasr_amd.metrics', None)   # any import of the module raises ImportError from here on
    results = {}
    for dev in (False, True):
        opt = options.dict_to_nonedict({'scale': 4, 'suffix': None, 'val_lpips': False, 'path': {'val_images': str(tmp_path / ('val%d' % dev))},
                                        **({'device_metrics': True} if dev else {})})
        lg, lines = _capture_logger('metrics_host_test_%d' % dev)
        out = tmp_path / ('eval%d' % dev)
        out.mkdir()
        m = _FakeModel(dev)
        res = dtest.evaluate(m, _loader(), opt, str(out), lg, 4)
        assert set(m.used) == ({'sr_u8', 'metrics'} if dev else {'visuals'})
        pngs = {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}
        m2 = _FakeModel(dev)
        psnr = train.validate(m2, _loader(), opt, 7, lg)
        assert set(m2.used) == ({'sr_u8', 'metrics'} if dev else {'visuals'})
        results[dev] = (res, lines, pngs, psnr)
    assert 'dasr_amd.metrics' in sys.modules and sys.modules['dasr_amd.metrics'] is None
    (r0, l0, p0, v0), (r1, l1, p1, v1) = results[False], results[True]
    assert list(p0) == ['img_0.png', 'img_1.png'] and p0 == p1
    assert r0 == r1 and l0 == l1 and v0 == v1
    assert len(r0['psnr']) == 2 and len(r0['ssim_y']) == 2 and any('PSNR_Y' in l for l in l0) and any('# Validation # PSNR' in l for l in l0)
