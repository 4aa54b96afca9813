"""Host side of the device PNG encoder (dasr_amd/png.py, csrc/png.hip): the numpy / pure-Python restatement of the stream against PIL and zlib (decoded pixels, the
inflated IDAT with its Adler-32, every chunk CRC), the filter against a literal per-pixel loop, the file sizes against PIL's compress_level=3, the Huffman lengths, the
entry points in header, binding and library, and what the CLIs refuse before they open a device.  No device."""
import heapq
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'dasr_png_filter': 11, 'dasr_png_codes': 6, 'dasr_png_emit': 13, 'dasr_png_pack': 14}
PHOTO_SIZES = ((1, 1), (5, 7), (33, 17), (64, 64), (120, 120), (128, 192))
SIZE_CASES = ((120, 120, 120120), (128, 192, 128192))


def contents(h, w):
    """the test contents at h x w (tests/test_gpu_png.py runs the same list on the device)"""
    from dasr_amd.png import photo
    rng = np.random.default_rng(7)
    return {'photo': photo(h, w, 1000 * h + w), 'zero': np.zeros((h, w, 3), np.uint8), 'full': np.full((h, w, 3), 255, np.uint8),
            'ramp': np.ascontiguousarray(np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)[None, :, None], (h, w, 3))),
            'random': rng.integers(0, 256, (h, w, 3), dtype=np.uint8)}


def chunks(data):
    """[(type, data)] of a PNG file; asserts the signature and every CRC"""
    from dasr_amd.png import SIGNATURE
    assert data[:8] == SIGNATURE
    out, p = [], 8
    while p < len(data):
        n, kind = struct.unpack('>I', data[p:p + 4])[0], data[p + 4:p + 8]
        body = data[p + 8:p + 8 + n]
        assert struct.unpack('>I', data[p + 8 + n:p + 12 + n])[0] == zlib.crc32(kind + body), kind
        out.append((kind, body))
        p += 12 + n
    assert p == len(data)
    return out


def check_file(data, img, what):
    """the file decodes with PIL to mode RGB and the pixels of img; its one IDAT inflates (Adler-32 verified by zlib) to filter_ref's bytes; the chunk CRCs hold"""
    from PIL import Image
    from dasr_amd.png import filter_ref
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == 'PNG' and im.mode == 'RGB', what
        assert np.array_equal(np.array(im), img), what
    ch = chunks(data)
    assert [k for k, _ in ch] == [b'IHDR', b'IDAT', b'IEND'], what
    assert ch[0][1] == struct.pack('>IIBBBBB', img.shape[1], img.shape[0], 8, 2, 0, 0, 0), what
    idat = ch[1][1]
    assert idat[:2] == b'\x78\x01' and idat[-6:-4] == b'\x03\x00', what
    assert zlib.decompress(idat) == filter_ref(img).tobytes(), what


def pil_level3(img):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'PNG', compress_level=3)
    return len(buf.getvalue())


def heapq_cost(freq):
    """total bits of an unrestricted Huffman code for freq (the sum of the internal nodes' weights)"""
    h = [int(f) for f in freq if f > 0]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a = heapq.heappop(h) + heapq.heappop(h)
        cost += a
        heapq.heappush(h, a)
    return cost


def check_code(freq, lens, codes, max_bits=15):
    """lengths <= max_bits, every used symbol has a code, Kraft sum exactly 1, the codes are the canonical ones of RFC 1951 3.2.2 and prefix-free"""
    from dasr_amd.png import canonical_codes
    lens, codes = [int(v) for v in lens], [int(v) for v in codes]
    assert max(lens) <= max_bits
    assert all(l > 0 for f, l in zip(freq, lens) if f > 0)
    assert sum(1 << (max_bits - l) for l in lens if l) == 1 << max_bits
    assert codes == canonical_codes(lens)
    words = sorted(format(c, '0%db' % l) for c, l in zip(codes, lens) if l)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))


@pytest.mark.parametrize('hw', PHOTO_SIZES)
def test_reference_files_decode_inflate_and_carry_right_crcs(hw):
    from dasr_amd.png import encode_ref, photo
    img = photo(hw[0], hw[1], 1000 * hw[0] + hw[1])
    check_file(encode_ref(img), img, hw)


@pytest.mark.parametrize('name', ['zero', 'full', 'ramp', 'random'])
def test_reference_files_of_the_other_contents(name):
    from dasr_amd.png import encode_ref
    img = contents(33, 17)[name]
    data = encode_ref(img)
    check_file(data, img, name)
    strip = chunks(data)[1][1][2:-6]
    assert (strip[0] & 7 == 0) == (name == 'random')   # uniform random bytes: one stored block; everything else: a dynamic block, BFINAL 0


def test_filter_equals_a_literal_loop():
    from dasr_amd.png import filter_ref, photo
    img = photo(5, 7, 57)
    H, W = img.shape[:2]
    raw = img.reshape(H, 3 * W).astype(int)
    want = []
    for y in range(H):
        rows = []
        for t in range(5):
            row = []
            for j in range(3 * W):
                a = raw[y][j - 3] if j >= 3 else 0
                b = raw[y - 1][j] if y > 0 else 0
                c = raw[y - 1][j - 3] if y > 0 and j >= 3 else 0
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                paeth = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                row.append((raw[y][j] - (0, a, b, (a + b) // 2, paeth)[t]) % 256)
            rows.append(row)
        costs = [sum(min(v, 256 - v) for v in row) for row in rows]
        t = costs.index(min(costs))
        want.append([t] + rows[t])
    assert np.array_equal(filter_ref(img), np.array(want, dtype=np.uint8))


def test_strip_statistics_and_adler_combination():
    from dasr_amd.png import adler_combine, filter_ref, photo, strip_rows, strip_stats_ref
    W = 341
    rows = strip_rows(W)
    assert rows == 32768 // 1024 and strip_rows(1) == 8192 and strip_rows(21844) == 1 and strip_rows(5462) == 1 and strip_rows(5461) == 2
    img = photo(2 * rows + 1, W, 5)
    f = filter_ref(img)
    hist, adler = strip_stats_ref(f)
    assert hist.shape == (3, 257) and (hist[:, 256] == 1).all() and hist[:, :256].sum(axis=1).tolist() == [rows * 1024, rows * 1024, 1024]
    assert adler_combine(adler, [rows * 1024, rows * 1024, 1024]) == zlib.adler32(f.tobytes())


@pytest.mark.parametrize('case', SIZE_CASES)
def test_reference_files_are_no_larger_than_pil_level_3(case):
    """measured: 20 558 <= 24 598 and 33 929 <= 41 791 bytes"""
    from dasr_amd.png import encode_ref, photo
    img = photo(*case)
    assert len(encode_ref(img)) <= pil_level3(img)


def fibonacci_hist():
    f = [1, 1]
    while len(f) < 24:
        f.append(f[-1] + f[-2])
    return [0] * (257 - 24) + f   # (the last of the 24 symbols is end-of-block)


def test_huffman_lengths_are_optimal_complete_and_limited():
    from dasr_amd.png import canonical_codes, filter_ref, huffman_lengths, photo, strip_stats_ref
    two = [0] * 257
    two[0], two[256] = 500, 1
    flat = [3] * 257
    own = strip_stats_ref(filter_ref(photo(64, 64, 64064)))[0][0].tolist()
    for freq in (two, flat, own):
        lens = huffman_lengths(freq, 15)
        check_code(freq, lens, canonical_codes(lens))
        assert sum(f * l for f, l in zip(freq, lens)) == heapq_cost(freq)
    fib = fibonacci_hist()
    lens = huffman_lengths(fib, 15)
    check_code(fib, lens, canonical_codes(lens))
    assert sum(f * l for f, l in zip(fib, lens)) >= heapq_cost(fib)
    for freq in ([0] * 19, [0] * 7 + [9] + [0] * 11, [5] + [0] * 18):   # fewer than two used symbols: two codes of one bit
        lens = huffman_lengths(freq, 7)
        assert sorted(lens)[-2:] == [1, 1] and sum(lens) == 2


def test_entry_points_in_header_binding_and_library():
    from dasr_amd import _lib, build, png
    header = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r'^int %s\(([^;]*)\);' % name, header, flags=re.M)
        assert m and len(m.group(1).split(',')) == nargs, name
        assert name in _lib._SIGS and len(_lib._SIGS[name]) == nargs, name
    assert re.search(r'^#define DASR_ABI_VERSION 22$', header, flags=re.M) and _lib.ABI_VERSION == 22   # additions only
    assert re.search(r'^#define DASR_PNG_HDR_WORDS %d$' % png.HDR_WORDS, header, flags=re.M)
    assert 'png.hip' in build.MORE_SOURCES and os.path.exists(build.build())
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    data = open(_lib.LIB_PATH, 'rb').read()
    for kernel in (b'png_filter_kernel', b'png_codes_kernel', b'png_emit_kernel', b'png_scan_kernel', b'png_gather_kernel'):
        assert kernel in data, kernel
    assert png.IMAGE_DESC.itemsize == 32 and png.STRIP_DESC.itemsize == 32   # dasr_png_image, dasr_png_strip


def test_encode_batch_refuses_what_it_cannot_encode():
    import torch
    from dasr_amd import png
    assert png.encode_batch([]) == []
    for bad in (torch.zeros(4, 4, 3, dtype=torch.uint8), np.zeros((4, 4, 3), np.uint8)):   # host memory
        with pytest.raises(ValueError, match=r'images\[0\]'):
            png.encode_batch([bad])
    with pytest.raises(ValueError, match='paths'):
        png.write_batch([torch.zeros(4, 4, 3, dtype=torch.uint8)], [], None)
    with pytest.raises(ValueError, match='PIL'):
        png.encode_ref(np.zeros((1, 21845, 3), np.uint8))
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32)):
        with pytest.raises(ValueError):
            png.encode_ref(bad)


# ---- the CLIs ---------------------------------------------------------------------------------------------------------------------------
def _png(path, size=(48, 48), seed=3):
    from PIL import Image
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, size + (3,)).astype(np.uint8)).save(str(path))


def test_flag_is_off_by_default():
    from dasr_amd import add_corruptions, prepare_data
    assert prepare_data.parse_args(['--input_dir', 'x']).device_png is False and prepare_data.parse_args(['--input_dir', 'x', '--device_png']).device_png is True
    assert add_corruptions.parse_args([]).device_png is False and add_corruptions.parse_args(['--device_png']).device_png is True


def test_prepare_data_refuses_device_png_without_a_device_product(tmp_path):
    from dasr_amd.prepare_data import main
    hr = tmp_path / 'HR'
    hr.mkdir()
    _png(hr / 'a.png')
    for flags in (['--sub_dir', str(tmp_path / 'sub')], ['--mod_dir', str(tmp_path / 'mod')], ['--sub_dir', str(tmp_path / 'sub'), '--mod_dir', str(tmp_path / 'mod')]):
        with pytest.raises(ValueError, match='device_png'):
            main(['--input_dir', str(hr), '--crop_sz', '24', '--step', '12', '--device_png'] + flags)
    assert not (tmp_path / 'sub').exists() and not (tmp_path / 'mod').exists()


def test_add_corruptions_refuses_device_png_with_blur(tmp_path):
    from dasr_amd.add_corruptions import main
    src = tmp_path / 'in'
    src.mkdir()
    _png(src / 'a.png')
    with pytest.raises(ValueError, match='device_png'):
        main(['--input_dir', str(src), '--output_dir', str(tmp_path / 'out'), '--blur_std_dev', '1.5', '--device_png'])
    assert not (tmp_path / 'out').exists()
