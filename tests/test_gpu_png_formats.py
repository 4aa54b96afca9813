"""GPU: the pixel formats of the device PNG encoder (`fmt='bgr'` / `'grey'` of dasr_amd/png.py; dasr_png_filter_fmt / dasr_png_pack_fmt of csrc/png.hip) and the device mode of png.FileWriter (png.DeviceWriter).
The filter stage bit for bit against png.filter_ref (types, bytes, histograms, Adler partials, the combined Adler-32 against zlib's), fmt 0 against dasr_png_filter, what the
two entry points refuse, whole batches by what the files decode and inflate to, and the writer against encode_batch.

Two Huffman constructions may break ties differently, so files are compared with the restatement by content (PIL's mode and pixels, zlib's inflate with its Adler-32 check,
the chunk CRCs); the device's own files are compared byte for byte (the same inputs give the same bytes)."""
import zlib

import numpy as np
import pytest
import torch

from test_png_formats_host import check_file_fmt
from test_png_host import contents

pytestmark = pytest.mark.gpu

EINVAL = -22


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _image(h, w, seed, fmt):
    """the test image of a format: png.photo, for 'grey' its first channel"""
    from dasr_amd.png import photo
    a = photo(h, w, seed)
    return a if fmt == 'bgr' else a[:, :, 0].copy()


def _check_filter_stage(arrays, tensors, fmt):
    """stage 1 on `tensors` (device views of `arrays`) equals the restatement: every strip's types, bytes, histogram and Adler pair; the combined Adler equals zlib's"""
    from dasr_amd import png
    plan, filt, hist, meta = png.filter_batch(tensors, fmt=fmt)
    torch.cuda.synchronize()
    filt, hist, meta = filt.cpu().numpy(), hist.cpu().numpy().view(np.uint32), meta.cpu().numpy()
    adler = meta[plan.n_images + 3:].view(np.uint32).reshape(-1, 2)
    assert meta[0] == 0 and plan.fmt == fmt
    bpp = 1 if fmt == 'grey' else 3
    for k, a in enumerate(arrays):
        ref = png.filter_ref(a, fmt)
        assert ref.shape == (a.shape[0], 1 + bpp * a.shape[1])
        ref_hist, ref_adler = png.strip_stats_ref(ref, fmt)
        first, cnt = int(plan.images['first_strip'][k]), int(plan.images['n_strips'][k])
        rows = png.strip_rows(a.shape[1], fmt)
        assert cnt == -(-a.shape[0] // rows) == len(ref_hist)
        for s in range(cnt):
            d = plan.strips[first + s]
            want = ref[s * rows:(s + 1) * rows].reshape(-1)
            assert d['n'] == want.size and d['row0'] == s * rows
            got = filt[d['filt_off']:d['filt_off'] + d['n']]
            assert np.array_equal(got.reshape(-1, ref.shape[1])[:, 0], want.reshape(-1, ref.shape[1])[:, 0]), ('types', fmt, k, a.shape, s)
            assert np.array_equal(got, want), ('bytes', fmt, k, a.shape, s)
        assert np.array_equal(hist[first:first + cnt], ref_hist), ('hist', fmt, k, a.shape)
        assert np.array_equal(adler[first:first + cnt], ref_adler), ('adler', fmt, k, a.shape)
        assert png.adler_combine(adler[first:first + cnt], plan.strips['n'][first:first + cnt]) == zlib.adler32(ref.tobytes()), ('adler32', fmt, k, a.shape)


# ---- 1. the filter stage ------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = {'bgr': [(1, 1), (1, 9), (9, 1), (5, 7)] + [(6, w) for w in (21, 22, 85, 86, 341)],                 # row bytes 3 W on both sides of 64, 256 and 1024
              'grey': [(1, 1), (1, 9), (9, 1)] + [(6, w) for w in (63, 64, 65, 255, 256, 257, 1023, 1025)]}      # row bytes W on both sides of them
STRIP_HEIGHTS = {'bgr': (32, (31, 32, 33, 65)), 'grey': (95, (94, 95, 96, 191))}                                 # rows per strip at W 341, the heights around it


@pytest.mark.parametrize('fmt', ['bgr', 'grey'])
def test_filter_stage_at_the_edge_sizes(fmt):
    dev = _gpu()
    arrays = [_image(h, w, 100 * h + w, fmt) for h, w in EDGE_SIZES[fmt]]
    _check_filter_stage(arrays, [torch.from_numpy(a).to(dev) for a in arrays], fmt)


@pytest.mark.parametrize('fmt', ['bgr', 'grey'])
def test_filter_stage_around_the_strip_height(fmt):
    dev = _gpu()
    from dasr_amd.png import strip_rows
    rows, heights = STRIP_HEIGHTS[fmt]
    assert strip_rows(341, fmt) == rows
    arrays = [_image(h, 341, h, fmt) for h in heights]
    _check_filter_stage(arrays, [torch.from_numpy(a).to(dev) for a in arrays], fmt)


@pytest.mark.parametrize('fmt', ['bgr', 'grey'])
def test_filter_stage_on_every_content_and_on_a_strided_window(fmt):
    dev = _gpu()
    arrays = [a if fmt == 'bgr' else a[:, :, 0].copy() for a in contents(33, 17).values()]
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    big = _image(50, 40, 5040, fmt)
    big_dev = torch.from_numpy(big).to(dev)
    arrays.append(np.ascontiguousarray(big[7:40, 5:22]))
    tensors.append(big_dev[7:40, 5:22])          # the first pixel 5 pixels into its row, rows 40 pixels apart
    assert not tensors[-1].is_contiguous()
    _check_filter_stage(arrays, tensors, fmt)


def test_bgr_is_rgb_of_the_channel_reversed_image():
    """the filtered bytes, histograms and Adler words of fmt 'bgr' are those of the default fmt on the image with its channels reversed in memory"""
    dev = _gpu()
    from dasr_amd import png
    arrays = [png.photo(h, w, 7 * h + w) for h, w in ((5, 7), (40, 341), (1, 1))]
    rev = [np.ascontiguousarray(a[:, :, ::-1]) for a in arrays]
    out = []
    for batch, fmt in ((arrays, 'bgr'), (rev, 'rgb')):
        plan, filt, hist, meta = png.filter_batch([torch.from_numpy(a).to(dev) for a in batch], fmt=fmt)
        torch.cuda.synchronize()
        f = filt.cpu().numpy()
        out.append(([f[d['filt_off']:d['filt_off'] + d['n']].tobytes() for d in plan.strips], hist.cpu().numpy().tobytes(), meta.cpu().numpy()[plan.n_images + 3:].tobytes()))
    assert out[0] == out[1]


def _buffers(plan, dev):
    return (torch.zeros(plan.filt_bytes, dtype=torch.uint8, device=dev), torch.zeros((plan.n_strips, 257), dtype=torch.int32, device=dev),
            torch.zeros((plan.n_strips, 2), dtype=torch.int32, device=dev))


def test_filter_fmt_0_gives_the_bits_of_dasr_png_filter():
    dev = _gpu()
    from dasr_amd import _lib, png
    L = _lib.lib()
    arrays = [png.photo(h, w, 3 * h + w) for h, w in ((1, 1), (5, 7), (33, 17), (70, 341))] + [contents(33, 17)['random']]
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    plan = png.Plan(tensors)
    ih, sh = plan.host()
    old, new = _buffers(plan, dev), _buffers(plan, dev)
    assert L.dasr_png_filter(plan.images_dev, ih, plan.n_images, plan.strips_dev, sh, plan.n_strips, old[0].data_ptr(), plan.filt_bytes, old[1].data_ptr(), old[2].data_ptr(),
                             _stream()) == 0
    assert L.dasr_png_filter_fmt(plan.images_dev, ih, plan.n_images, plan.strips_dev, sh, plan.n_strips, new[0].data_ptr(), plan.filt_bytes, new[1].data_ptr(),
                                 new[2].data_ptr(), 0, _stream()) == 0
    torch.cuda.synchronize()
    assert plan.n_strips == 7 and int(old[1].sum()) == sum(int(n) for n in plan.strips['n']) + plan.n_strips    # (the old entry point ran: every byte and end-of-block counted)
    for a, b, what in zip(old, new, ('bytes', 'hist', 'adler')):
        assert torch.equal(a, b), what


# ---- 2. what the entry points refuse ---------------------------------------------------------------------------------------------------------
def _calls(plan, dev):
    """(filter_fmt(images, strips, fmt, filt_bytes), pack_fmt(images, strips, fmt), untouched()) on zeroed buffers of `plan`"""
    from dasr_amd import _lib
    L = _lib.lib()
    filt, hist, adler = _buffers(plan, dev)
    sizes = torch.zeros(plan.n_strips, dtype=torch.int32, device=dev)
    slots, out = torch.zeros(plan.slot_bytes, dtype=torch.uint8, device=dev), torch.zeros(plan.slot_bytes, dtype=torch.uint8, device=dev)
    ws, meta = torch.zeros(plan.n_strips, dtype=torch.int64, device=dev), torch.zeros(plan.n_images + 3, dtype=torch.int64, device=dev)

    def filt_call(images, strips, fmt, filt_bytes=plan.filt_bytes):
        return L.dasr_png_filter_fmt(plan.images_dev, images.ctypes.data, plan.n_images, plan.strips_dev, strips.ctypes.data, plan.n_strips, filt.data_ptr(), filt_bytes,
                                     hist.data_ptr(), adler.data_ptr(), fmt, _stream())

    def pack_call(images, strips, fmt, slot_bytes=plan.slot_bytes):
        return L.dasr_png_pack_fmt(plan.images_dev, images.ctypes.data, plan.n_images, plan.strips_dev, strips.ctypes.data, plan.n_strips, sizes.data_ptr(), slots.data_ptr(),
                                   slot_bytes, ws.data_ptr(), out.data_ptr(), plan.slot_bytes, meta.data_ptr(), fmt, _stream())

    def untouched():
        torch.cuda.synchronize()
        return all(int(t.count_nonzero()) == 0 for t in (filt, hist, adler, out, ws, meta))
    return filt_call, pack_call, untouched


@pytest.mark.parametrize('fmt', ['bgr', 'grey'])
def test_entry_points_refuse_bad_tables_and_formats(fmt):
    dev = _gpu()
    from dasr_amd import png
    code, bpp = png.FORMATS[fmt]
    x = torch.zeros((4, 5, 3) if bpp == 3 else (4, 5), dtype=torch.uint8, device=dev)
    plan = png.Plan([x], fmt)
    filt_call, pack_call, untouched = _calls(plan, dev)
    for call in (filt_call, pack_call):
        for bad_fmt in (3, -1):
            assert call(plan.images, plan.strips, bad_fmt) == EINVAL, bad_fmt
        assert call(plan.images, plan.strips, 2 if bpp == 3 else 0) == EINVAL            # n = rows (1 + bpp W) computed with the other bpp
        for field, value in (('W', png.max_width(fmt) + 1), ('W', 0), ('H', 0), ('pitch', bpp * 5 - 1), ('src', 0), ('n_strips', 2)):
            bad = plan.images.copy()
            bad[field][0] = value
            assert call(bad, plan.strips, code) == EINVAL, field
        for field, value in (('rows', 5), ('n', 4 * (1 + bpp * 5) - 1), ('row0', 1), ('image', 1)):
            bad = plan.strips.copy()
            bad[field][0] = value
            assert call(plan.images, bad, code) == EINVAL, field
    bad = plan.strips.copy()
    bad['filt_off'][0] = 8
    assert filt_call(plan.images, bad, code) == EINVAL
    assert filt_call(plan.images, plan.strips, code, filt_bytes=plan.filt_bytes - 16) == EINVAL
    bad = plan.strips.copy()
    bad['slot_off'][0] = 2
    assert pack_call(plan.images, bad, code) == EINVAL
    assert pack_call(plan.images, plan.strips, code, slot_bytes=plan.slot_bytes - 4) == EINVAL
    assert untouched()                                                                   # nothing was launched
    assert filt_call(plan.images, plan.strips, code) == 0 and pack_call(plan.images, plan.strips, code) == 0
    assert not untouched()


def test_grey_width_limit_of_the_entry_points():
    """W 65 535 is refused (a row of 65 536 filtered bytes), whatever n says; W 65 534 is the widest row"""
    dev = _gpu()
    from dasr_amd import png
    x = torch.zeros((1, 65534), dtype=torch.uint8, device=dev)
    plan = png.Plan([x], 'grey')
    assert plan.n_strips == 1 and plan.strips['n'][0] == 65535
    filt_call, pack_call, untouched = _calls(plan, dev)
    for call in (filt_call, pack_call):
        bad = plan.images.copy()
        bad['W'][0] = 65535
        assert call(bad, plan.strips, 2) == EINVAL
        strips = plan.strips.copy()
        strips['n'][0] = 65536
        assert call(bad, strips, 2) == EINVAL
        assert call(plan.images, plan.strips, 1) == EINVAL                               # three bytes per pixel at this width
    assert untouched()
    assert filt_call(plan.images, plan.strips, 2) == 0
    assert not untouched()
    a = (np.random.default_rng(3).integers(0, 8, (2, 65534)) + 100).astype(np.uint8)    # two strips of 65 535 bytes, the largest a slot holds
    check_file_fmt(png.encode_batch([torch.from_numpy(a).to(dev)], fmt='grey')[0], a, 'grey', a.shape)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['bgr', 'grey'])
def test_encode_batch_of_five_images(fmt):
    dev = _gpu()
    from dasr_amd import png
    from test_png_host import chunks
    tall = 2 * png.strip_rows(120, fmt) + 1
    arrays = [_image(1, 1, 11, fmt), _image(5, 7, 57, fmt), _image(33, 17, 3317, fmt), _image(tall, 120, 7, fmt), contents(33, 17)['random']]
    if fmt == 'grey':
        arrays[4] = arrays[4][:, :, 0].copy()
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    files = png.encode_batch(tensors, fmt=fmt)
    assert len(files) == 5 and all(isinstance(f, bytes) for f in files)
    for a, f in zip(arrays, files):
        check_file_fmt(f, a, fmt, (fmt, a.shape))
    stored = [chunks(f)[1][1][2] & 7 == 0 for f in files]                                      # a stored block for 1 x 1 and for random bytes, BTYPE 10 for the photos
    assert [stored[k] for k in (0, 2, 3, 4)] == [True, False, False, True] and (fmt == 'grey' or not stored[1])   # (5 x 7 grey is 40 bytes: smaller than a block header)
    assert png.encode_batch(tensors, fmt=fmt) == files                                         # the same inputs give the same bytes


def test_formats_refuse_the_other_layout():
    dev = _gpu()
    from dasr_amd import png
    grey, colour = torch.zeros((4, 4), dtype=torch.uint8, device=dev), torch.zeros((4, 4, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=r'images\[0\]'):
        png.encode_batch([grey])                                                               # the default fmt still takes [H, W, 3] only
    with pytest.raises(ValueError, match=r'images\[1\]'):
        png.encode_batch([colour, grey], fmt='bgr')
    with pytest.raises(ValueError, match=r'images\[1\]'):
        png.encode_batch([grey, colour], fmt='grey')
    with pytest.raises(ValueError, match=r'images\[0\]'):
        png.encode_batch([torch.zeros((4, 8), dtype=torch.uint8, device=dev)[:, ::2]], fmt='grey')   # stride(1) == 2
    with pytest.raises(ValueError, match='PIL'):
        png.encode_batch([torch.zeros((1, 65535), dtype=torch.uint8, device=dev)], fmt='grey')
    with pytest.raises(ValueError, match='PIL'):
        png.encode_batch([torch.zeros((1, 21845, 3), dtype=torch.uint8, device=dev)], fmt='bgr')
    with pytest.raises(ValueError, match='fmt'):
        png.encode_batch([colour], fmt='rgba')


# ---- 4. the writer ------------------------------------------------------------------------------------------------------------------------
def test_device_writer_writes_the_files_of_encode_batch(tmp_path):
    """one thread: two files may be outstanding, so the third write waits for the first"""
    dev = _gpu()
    from dasr_amd import png
    jobs = [(_image(40, 24, 1, 'bgr'), 'bgr'), (_image(16, 16, 2, 'grey'), 'grey'), (png.photo(37, 53, 3), 'rgb')]
    tensors = [torch.from_numpy(a).to(dev) for a, _ in jobs]
    paths = [str(tmp_path / ('%d.png' % k)) for k in range(3)]
    with png.DeviceWriter(1) as w:
        for t, p, (_, fmt) in zip(tensors, paths, jobs):
            w.write(t, p, fmt)
        assert len(w._pending) <= 2
    for t, p, (a, fmt) in zip(tensors, paths, jobs):
        data = open(p, 'rb').read()
        assert data == png.encode_batch([t], fmt=fmt)[0], p
        if fmt != 'rgb':
            check_file_fmt(data, a, fmt, p)


def test_device_writer_close_raises_the_first_failure(tmp_path):
    dev = _gpu()
    from dasr_amd import png
    t = torch.from_numpy(png.photo(8, 8, 1)).to(dev)
    w = png.DeviceWriter(2)
    w.write(t, str(tmp_path / 'ok.png'), 'bgr')
    w.write(t, str(tmp_path / 'missing' / 'a.png'), 'bgr')
    w.write(t, str(tmp_path / 'ok2.png'), 'bgr')
    with pytest.raises(OSError, match='missing'):
        w.close()
    assert (tmp_path / 'ok.png').read_bytes() == (tmp_path / 'ok2.png').read_bytes() == png.encode_batch([t], fmt='bgr')[0]   # the other files are complete
    with pytest.raises(OSError):
        with png.DeviceWriter(2) as w2:
            w2.write(t, str(tmp_path / 'missing' / 'b.png'), 'bgr')
