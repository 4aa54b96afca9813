"""GPU: the device PNG encoder (dasr_amd/png.py, csrc/png.hip, `--device_png` of prepare_data and add_corruptions).  The filter stage bit for bit against png.filter_ref
(types, bytes, histograms, Adler partials), the code stage on hand-made histograms through the C ABI (lengths, Kraft sum, canonical codes, the heapq optimum), whole
batches by what the files decode and inflate to, the width limit, and the CLIs against the files their default path writes.

Two Huffman constructions may break ties differently, so files are compared by content (PIL's pixels, zlib's inflate with its Adler-32 check, the chunk CRCs), not by
their bytes; sizes are compared with PIL's compress_level=3 for the two images the host test names."""
import os
import zlib

import numpy as np
import pytest
import torch

from test_png_host import SIZE_CASES, check_code, check_file, contents, fibonacci_hist, heapq_cost, pil_level3

pytestmark = pytest.mark.gpu

EINVAL = -22
CLI_SIZES = ((16, 16), (40, 24), (37, 53))   # the sizes of the CLI tests of tests/test_gpu_corrupt.py


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_filter_stage(arrays, tensors):
    """stage 1 on `tensors` (device views of `arrays`) equals the restatement: every strip's bytes, histogram and Adler pair; the combined Adler equals zlib's"""
    from dasr_amd import png
    plan, filt, hist, meta = png.filter_batch(tensors)
    torch.cuda.synchronize()
    filt, hist, meta = filt.cpu().numpy(), hist.cpu().numpy().view(np.uint32), meta.cpu().numpy()
    adler = meta[plan.n_images + 3:].view(np.uint32).reshape(-1, 2)
    assert meta[0] == 0
    for k, a in enumerate(arrays):
        ref = png.filter_ref(a)
        ref_hist, ref_adler = png.strip_stats_ref(ref)
        first, cnt = int(plan.images['first_strip'][k]), int(plan.images['n_strips'][k])
        rows = png.strip_rows(a.shape[1])
        assert cnt == -(-a.shape[0] // rows) == len(ref_hist)
        for s in range(cnt):
            d = plan.strips[first + s]
            want = ref[s * rows:(s + 1) * rows].reshape(-1)
            assert d['n'] == want.size and d['row0'] == s * rows
            got = filt[d['filt_off']:d['filt_off'] + d['n']]
            assert np.array_equal(got.reshape(-1, ref.shape[1])[:, 0], want.reshape(-1, ref.shape[1])[:, 0]), ('types', k, a.shape, s)
            assert np.array_equal(got, want), ('bytes', k, a.shape, s)
        assert np.array_equal(hist[first:first + cnt], ref_hist), ('hist', k, a.shape)
        assert np.array_equal(adler[first:first + cnt], ref_adler), ('adler', k, a.shape)
        assert png.adler_combine(adler[first:first + cnt], plan.strips['n'][first:first + cnt]) == zlib.adler32(ref.tobytes()), ('adler32', k, a.shape)


# ---- 1. the filter stage ------------------------------------------------------------------------------------------------------------------
def test_filter_stage_at_the_edge_sizes():
    """1 x 1, 1 x W, H x 1, 5 x 7; row bytes on both sides of 64, 256 and 1024; one batch"""
    dev = _gpu()
    from dasr_amd.png import photo
    sizes = [(1, 1), (1, 9), (9, 1), (5, 7)] + [(6, w) for w in (21, 22, 85, 86, 341)]
    arrays = [photo(h, w, 100 * h + w) for h, w in sizes]
    _check_filter_stage(arrays, [torch.from_numpy(a).to(dev) for a in arrays])


def test_filter_stage_around_the_strip_height():
    dev = _gpu()
    from dasr_amd.png import photo, strip_rows
    W = 341
    r = strip_rows(W)
    arrays = [photo(h, W, h) for h in (r - 1, r, r + 1, 2 * r + 1)]
    _check_filter_stage(arrays, [torch.from_numpy(a).to(dev) for a in arrays])


def test_filter_stage_on_every_content_and_on_a_strided_window():
    dev = _gpu()
    from dasr_amd.png import photo
    arrays = list(contents(33, 17).values())
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    big = photo(50, 40, 5040)
    big_dev = torch.from_numpy(big).to(dev)
    arrays.append(np.ascontiguousarray(big[7:40, 5:22]))
    tensors.append(big_dev[7:40, 5:22])          # rows 120 bytes apart, the first pixel 15 bytes into its row
    assert not tensors[-1].is_contiguous()
    _check_filter_stage(arrays, tensors)


def test_filter_entry_point_refuses_bad_tables():
    dev = _gpu()
    from dasr_amd import _lib, png
    L = _lib.lib()
    x = torch.zeros((4, 5, 3), dtype=torch.uint8, device=dev)
    plan = png.Plan([x])
    filt = torch.zeros(plan.filt_bytes, dtype=torch.uint8, device=dev)
    hist = torch.zeros((plan.n_strips, 257), dtype=torch.int32, device=dev)
    adler = torch.zeros((plan.n_strips, 2), dtype=torch.int32, device=dev)

    def call(images, strips, filt_bytes=plan.filt_bytes):
        return L.dasr_png_filter(plan.images_dev, images.ctypes.data, 1, plan.strips_dev, strips.ctypes.data, 1, filt.data_ptr(), filt_bytes, hist.data_ptr(),
                                 adler.data_ptr(), _stream())
    assert call(plan.images, plan.strips) == 0
    for field, value in (('W', 21845), ('W', 0), ('H', 0), ('pitch', 14), ('src', 0), ('n_strips', 2)):
        bad = plan.images.copy()
        bad[field][0] = value
        assert call(bad, plan.strips) == EINVAL, field
    for field, value in (('rows', 5), ('n', 63), ('filt_off', 8), ('row0', 1), ('image', 1)):
        bad = plan.strips.copy()
        bad[field][0] = value
        assert call(plan.images, bad) == EINVAL, field
    assert call(plan.images, plan.strips, filt_bytes=plan.filt_bytes - 16) == EINVAL
    torch.cuda.synchronize()


# ---- 2. the code stage --------------------------------------------------------------------------------------------------------------------
def _code_cases():
    from dasr_amd.png import filter_ref, photo, strip_stats_ref
    two = [0] * 257
    two[0], two[256] = 500, 1
    return {'two': two, 'flat': [3] * 257, 'photo': strip_stats_ref(filter_ref(photo(64, 64, 64064)))[0][0].tolist(), 'fibonacci': fibonacci_hist()}


def test_code_stage_on_hand_made_histograms():
    dev = _gpu()
    from dasr_amd import png
    cases = _code_cases()
    hist = torch.tensor(list(cases.values()), dtype=torch.int32, device=dev)
    lens, codes, hdr = png.codes_batch(hist)
    torch.cuda.synchronize()
    lens, codes, hdr = lens.cpu().numpy(), codes.cpu().numpy().view(np.uint16), hdr.cpu().numpy().view(np.uint32)
    for k, (name, freq) in enumerate(cases.items()):
        check_code(freq, lens[k], codes[k])
        assert lens[k][256] > 0, name                                # end-of-block has a code
        cost, best = sum(f * int(l) for f, l in zip(freq, lens[k])), heapq_cost(freq)
        print('code stage %s: %d bits, heapq optimum %d, ratio %.6f' % (name, cost, best, cost / best))
        if name != 'fibonacci':                                      # an unrestricted tree of depth 23: the ratio is recorded (profiles/png_encode.txt), not asserted
            assert cost == best, name
        assert hdr[k][1] == cost and hdr[k][2] & 0xFFFF == 0x0100 and hdr[k][3] == 0, name
        # the header is the one the restatement writes for these lengths
        w, hclen = png.block_header([int(l) for l in lens[k]])
        assert hdr[k][0] == w.n and hdr[k][2] >> 16 == hclen, name
        assert hdr[k][4:4 + (w.n + 31) // 32].tobytes()[:(w.n + 7) // 8] == w.bytes(), name
    assert max(lens[3]) == 15 and sorted(lens[0].tolist())[-2:] == [1, 1]


def test_code_entry_point_refuses_bad_arguments():
    dev = _gpu()
    from dasr_amd import _lib
    L = _lib.lib()
    z = torch.zeros(257 * 4, dtype=torch.int32, device=dev)
    p = z.data_ptr()
    assert L.dasr_png_codes(p, 0, p, p, p, _stream()) == EINVAL
    assert L.dasr_png_codes(0, 1, p, p, p, _stream()) == EINVAL
    assert L.dasr_png_codes(p, 1, p, p + 1, p, _stream()) == EINVAL


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------------
def test_encode_batch_of_seven_images_in_one_call():
    dev = _gpu()
    from dasr_amd import png
    tall = 2 * png.strip_rows(120) + 1
    arrays = [png.photo(1, 1, 11), png.photo(*SIZE_CASES[0]), png.photo(*SIZE_CASES[1]), png.photo(tall, 120, 7), contents(33, 17)['random'], contents(33, 17)['zero'],
              png.photo(5, 7, 57)]
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    files = png.encode_batch(tensors)
    assert len(files) == 7 and all(isinstance(f, bytes) for f in files)
    for a, f in zip(arrays, files):
        check_file(f, a, a.shape)
    for k in (1, 2):
        print('device file %s: %d bytes, PIL level 3 %d' % (arrays[k].shape, len(files[k]), pil_level3(arrays[k])))
        assert len(files[k]) <= pil_level3(arrays[k])
    from test_png_host import chunks
    assert [chunks(f)[1][1][2] & 7 == 0 for f in files[:6]] == [True, False, False, False, True, False]   # a stored block for 1 x 1 and for random bytes, else BTYPE 10
    assert png.encode_batch(tensors) == files                      # the same inputs give the same bytes


def test_write_batch_writes_the_files_of_encode_batch(tmp_path):
    dev = _gpu()
    from concurrent.futures import ThreadPoolExecutor
    from dasr_amd import png
    arrays = [png.photo(40, 24, 1), png.photo(16, 16, 2)]
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    paths = [str(tmp_path / 'a.png'), str(tmp_path / 'b.png')]
    with ThreadPoolExecutor(max_workers=2) as pool:
        assert [f.result() for f in png.write_batch(tensors, paths, pool)] == paths
    assert [open(p, 'rb').read() for p in paths] == png.encode_batch(tensors)


def test_width_limit():
    dev = _gpu()
    from dasr_amd import png
    rng = np.random.default_rng(3)
    a = (rng.integers(0, 8, (2, 21844, 3)) + 100).astype(np.uint8)
    f = png.encode_batch([torch.from_numpy(a).to(dev)])[0]
    check_file(f, a, a.shape)
    with pytest.raises(ValueError, match='PIL'):
        png.encode_batch([torch.zeros((2, 21845, 3), dtype=torch.uint8, device=dev)])
    for bad in (torch.zeros((4, 4), dtype=torch.uint8, device=dev), torch.zeros((4, 4, 4), dtype=torch.uint8, device=dev), torch.zeros((4, 4, 3), device=dev),
                torch.zeros((4, 3, 8), dtype=torch.uint8, device=dev).permute(0, 2, 1)[:, :4]):
        with pytest.raises(ValueError, match=r'images\[1\]'):
            png.encode_batch([torch.zeros((4, 4, 3), dtype=torch.uint8, device=dev), bad])


# ---- 4. the CLIs ---------------------------------------------------------------------------------------------------------------------------
def _read(path):
    from PIL import Image
    with Image.open(str(path)) as im:
        assert im.format == 'PNG' and im.mode == 'RGB', path
        return np.array(im)


def _folder(tmp_path, sizes):
    from PIL import Image
    from dasr_amd.png import photo
    src = tmp_path / 'clean'
    src.mkdir()
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(photo(h, w, 900 + k)).save(str(src / ('img_%d.png' % k)))
    return src


def _same_pixels(a_dir, b_dir):
    names = sorted(os.listdir(str(a_dir)))
    assert names and names == sorted(os.listdir(str(b_dir)))
    for n in names:
        assert np.array_equal(_read(a_dir / n), _read(b_dir / n)), n
        chunks = open(str(b_dir / n), 'rb').read()
        assert chunks[:8] == b'\x89PNG\r\n\x1a\n'


def test_add_corruptions_device_png_writes_the_pixels_of_the_default_path(tmp_path, capsys):
    _gpu()
    from dasr_amd.add_corruptions import main
    src = _folder(tmp_path, CLI_SIZES)
    base = ['--input_dir', str(src), '--jpg_quality', '30', '--noise_std_dev', '8', '--seed', '11', '--num_workers', '2']
    host, dev = tmp_path / 'host', tmp_path / 'dev'
    want = main(base + ['--output_dir', str(host)])
    assert 'encoded on the device' not in capsys.readouterr().out   # (the default path logs what it logged before)
    got = main(base + ['--output_dir', str(dev), '--device_png'])
    assert capsys.readouterr().out.count('encoded on the device') == 1
    assert [os.path.basename(p) for p in got] == [os.path.basename(p) for p in want] and len(got) == 3
    _same_pixels(host, dev)
    with pytest.raises(ValueError, match='device_png'):
        main(base + ['--output_dir', str(tmp_path / 'blur'), '--device_png', '--blur_std_dev', '1.5'])
    assert not (tmp_path / 'blur').exists()


def test_prepare_data_device_png_writes_the_pixels_of_the_default_path(tmp_path, capsys):
    """three 100 x 130 files (the size of the CLI test of tests/test_gpu_prepare_data.py), 15 sub-images each, all four folders"""
    _gpu()
    from dasr_amd.prepare_data import main
    src = _folder(tmp_path, ((100, 130),) * 3)
    base = ['--input_dir', str(src), '--crop_sz', '48', '--step', '24', '--thres_sz', '8', '--scale', '4', '--num_workers', '2']

    def dirs(root):
        return {k: tmp_path / root / k for k in ('sub', 'mod', 'lr', 'bic')}

    def flags(d):
        return [x for k, p in d.items() for x in ('--%s_dir' % k, str(p))]
    host, dev = dirs('host'), dirs('dev')
    want = main(base + flags(host))
    assert 'encoded on the device' not in capsys.readouterr().out   # (the default path logs what it logged before)
    got = main(base + flags(dev) + ['--device_png'])
    assert capsys.readouterr().out.count('encoded on the device') == 1
    for k in host:
        assert [os.path.basename(p) for p in got[k]] == [os.path.basename(p) for p in want[k]] and len(got[k]) == 45
        _same_pixels(host[k], dev[k])
    # whole images as units (no --sub_dir), scale 3: the mod window is narrower than the uploaded image
    host3, dev3 = {k: tmp_path / 'host3' / k for k in ('mod', 'lr')}, {k: tmp_path / 'dev3' / k for k in ('mod', 'lr')}
    main(['--input_dir', str(src), '--scale', '3'] + flags(host3))
    main(['--input_dir', str(src), '--scale', '3', '--device_png'] + flags(dev3))
    for k in host3:
        _same_pixels(host3[k], dev3[k])
    with pytest.raises(ValueError, match='device_png'):
        main(base + ['--sub_dir', str(tmp_path / 'only' / 'sub'), '--mod_dir', str(tmp_path / 'only' / 'mod'), '--device_png'])
    assert not (tmp_path / 'only').exists()
