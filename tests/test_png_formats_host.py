"""Host side of the pixel formats of the device PNG encoder (`fmt='bgr'` / `'grey'` of dasr_amd/png.py, dasr_png_filter_fmt / dasr_png_pack_fmt of csrc/png.hip) and of the
option key `"device_png"`: the numpy / pure-Python restatement against PIL and zlib (mode, pixels, the inflated IDAT with its Adler-32, every chunk CRC), the entry points in
header and binding, what options.parse accepts.  No device."""
import io
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest

from test_png_host import chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'dasr_png_filter_fmt': 12, 'dasr_png_pack_fmt': 15}
SIZES = ((1, 1), (5, 7), (33, 17))


def check_file_fmt(data, img, fmt, what):
    """the file decodes with PIL to mode RGB and the channel-reversed pixels of a BGR img (mode L and the pixels of a grey img); its one IDAT inflates (Adler-32 verified
    by zlib) to filter_ref's bytes; IHDR names the colour type; the chunk CRCs hold (chunks)"""
    from PIL import Image
    from dasr_amd.png import filter_ref
    grey = fmt == 'grey'
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == 'PNG' and im.mode == ('L' if grey else 'RGB'), what
        assert np.array_equal(np.array(im), img if fmt != 'bgr' else img[:, :, ::-1]), what
    ch = chunks(data)
    assert [k for k, _ in ch] == [b'IHDR', b'IDAT', b'IEND'], what
    assert ch[0][1] == struct.pack('>IIBBBBB', img.shape[1], img.shape[0], 8, 0 if grey else 2, 0, 0, 0), what
    idat = ch[1][1]
    assert idat[:2] == b'\x78\x01' and idat[-6:-4] == b'\x03\x00', what
    assert zlib.decompress(idat) == filter_ref(img, fmt).tobytes(), what


def test_entry_points_in_header_and_binding():
    from dasr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r'^int %s\(([^;]*)\);' % name, header, flags=re.M)
        assert m and len(m.group(1).split(',')) == nargs, name
        assert 'int32_t fmt, void* stream' in m.group(1), name
        assert name in _lib._SIGS and len(_lib._SIGS[name]) == nargs, name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r'^#define DASR_ABI_VERSION 22$', header, flags=re.M) and _lib.ABI_VERSION == 22   # additions only
    for name, value in (('RGB', 0), ('BGR', 1), ('GREY', 2)):
        assert re.search(r'^#define DASR_PNG_%s %d$' % (name, value), header, flags=re.M)


@pytest.mark.parametrize('hw', SIZES)
def test_bgr_reference_files(hw):
    from dasr_amd.png import encode_ref, filter_ref, photo
    a = photo(hw[0], hw[1], 1000 * hw[0] + hw[1])
    data = encode_ref(a, fmt='bgr')
    check_file_fmt(data, a, 'bgr', hw)
    assert data == encode_ref(np.ascontiguousarray(a[:, :, ::-1]))           # the RGB file of the channel-reversed image
    assert np.array_equal(filter_ref(a, 'bgr'), filter_ref(np.ascontiguousarray(a[:, :, ::-1])))


@pytest.mark.parametrize('hw', SIZES)
def test_grey_reference_files(hw):
    from dasr_amd.png import encode_ref, photo
    g = np.ascontiguousarray(photo(hw[0], hw[1], 1000 * hw[0] + hw[1])[:, :, 0])
    check_file_fmt(encode_ref(g, fmt='grey'), g, 'grey', hw)


def test_grey_filter_equals_a_literal_loop():
    """bpp 1: the left neighbour is the byte before"""
    from dasr_amd.png import filter_ref, photo
    raw = photo(5, 7, 57)[:, :, 1].astype(int)
    H, W = raw.shape
    want = []
    for y in range(H):
        rows = []
        for t in range(5):
            row = []
            for j in range(W):
                a = raw[y][j - 1] if j >= 1 else 0
                b = raw[y - 1][j] if y > 0 else 0
                c = raw[y - 1][j - 1] if y > 0 and j >= 1 else 0
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                paeth = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                row.append((raw[y][j] - (0, a, b, (a + b) // 2, paeth)[t]) % 256)
            rows.append(row)
        costs = [sum(min(v, 256 - v) for v in row) for row in rows]
        t = costs.index(min(costs))
        want.append([t] + rows[t])
    assert np.array_equal(filter_ref(raw.astype(np.uint8), 'grey'), np.array(want, dtype=np.uint8))


def test_strip_rows_widths_and_refusals_per_format():
    from dasr_amd import png
    assert png.strip_rows(341, 'bgr') == png.strip_rows(341) == 32 and png.strip_rows(341, 'grey') == 95
    assert png.strip_rows(65534, 'grey') == 1 and png.strip_rows(1, 'grey') == 16384
    assert png.max_width('rgb') == png.max_width('bgr') == png.MAX_WIDTH == 21844 and png.max_width('grey') == 65534
    f = png.filter_ref(np.ascontiguousarray(png.photo(200, 341, 5)[:, :, 0]), 'grey')
    hist, adler = png.strip_stats_ref(f, 'grey')
    assert hist.shape == (3, 257) and hist[:, :256].sum(axis=1).tolist() == [95 * 342, 95 * 342, 10 * 342]
    assert png.adler_combine(adler, [95 * 342, 95 * 342, 10 * 342]) == zlib.adler32(f.tobytes())
    with pytest.raises(ValueError, match='PIL'):
        png.encode_ref(np.zeros((1, 65535), np.uint8), fmt='grey')
    with pytest.raises(ValueError, match='PIL'):
        png.encode_ref(np.zeros((1, 21845, 3), np.uint8), fmt='bgr')
    for bad, fmt in ((np.zeros((4, 4, 3), np.uint8), 'grey'), (np.zeros((4, 4), np.uint8), 'bgr'), (np.zeros((4, 4), np.uint8), 'rgb'), (np.zeros((4, 4), np.float32), 'grey')):
        with pytest.raises(ValueError):
            png.encode_ref(bad, fmt=fmt)
    with pytest.raises(ValueError, match='fmt'):
        png.encode_ref(np.zeros((4, 4, 3), np.uint8), fmt='rgba')
    with pytest.raises(ValueError, match='fmt'):
        png.encode_batch([np.zeros((4, 4, 3), np.uint8)], fmt='gray')


def test_device_writer_pool_is_bounded_and_refuses_host_memory(tmp_path):
    import torch
    from dasr_amd import png
    for asked, threads in ((1, 1), (6, 6), (64, 16), (0, 1)):
        w = png.DeviceWriter(asked)
        assert w.threads == threads and w.max_pending == 2 * threads
        w.close()
        w.close()                                                            # (a second close is a no-op)
    with pytest.raises(ValueError, match=r'images\[0\]'):
        with png.DeviceWriter(2) as w:
            w.write(torch.zeros(4, 4, dtype=torch.uint8), str(tmp_path / 'a.png'), 'grey')
    with pytest.raises(ValueError, match='close'):
        w.write(torch.zeros(4, 4, dtype=torch.uint8), str(tmp_path / 'a.png'), 'grey')
    assert not (tmp_path / 'a.png').exists()


def _opt_file(tmp_path, name, **extra):
    opt = {'name': name, 'use_tb_logger': False, 'model': 'sr', 'scale': 4, 'gpu_ids': None, 'datasets': {},
           'path': {'root': str(tmp_path), 'pretrain_model_G': None},
           'network_G': {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 32, 'nb': 1, 'in_nc': 3, 'out_nc': 3, 'gc': 32}}
    opt.update(extra)
    p = tmp_path / (name + '.json')
    p.write_text(json.dumps(opt))
    return str(p)


def test_options_accept_true_and_false_and_refuse_anything_else(tmp_path):
    from dasr_amd import options
    assert options.dict_to_nonedict(options.parse(_opt_file(tmp_path, 'absent'), is_train=False))['device_png'] is None
    assert options.parse(_opt_file(tmp_path, 'on', device_png=True), is_train=False)['device_png'] is True
    assert options.parse(_opt_file(tmp_path, 'off', device_png=False), is_train=False)['device_png'] is False
    for bad in (3, 1, 0, 'true', [True]):
        with pytest.raises(ValueError, match='device_png'):
            options.parse(_opt_file(tmp_path, 'bad', device_png=bad), is_train=False)
    assert options.device_png_flag(None) is False and options.device_png_flag(True) is True


def test_cli_flags_are_off_by_default():
    from dasr_amd import back_projection, dsn_create_dataset
    base = ['--lr_dir', 'a', '--sr_dir', 'b', '--out_dir', 'c']
    assert back_projection.parse_args(base).device_png is False and back_projection.parse_args(base + ['--device_png']).device_png is True
    p = dsn_create_dataset.build_parser()
    assert p.parse_args([]).device_png is False and p.parse_args(['--device_png']).device_png is True
