"""Host side of the one writer of the drivers that save 8-bit images (png.FileWriter, png.save_host) and of the checks the folder CLIs share (imgio.rgb8_header,
util.refuse_filled_folder, imgio.tick): the host mode of the writer with a saver the test controls, the bytes of the host saver against PIL, the bytes of
`prepare_data --sub_dir --mod_dir` (which opens no device).  No device."""
import io
import threading

import numpy as np
import pytest

SIZES = ((5, 7), (33, 20))


def _pil_bytes(pixels, level):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, 'PNG', compress_level=level)
    return buf.getvalue()


def test_host_mode_without_threads_writes_before_write_returns(tmp_path):
    from dasr_amd import png
    a = png.photo(5, 7, 1)
    with png.FileWriter(False, 0) as w:
        assert w.threads == 0 and w._pool is None
        w.write(a, str(tmp_path / 'a.png'))
        assert (tmp_path / 'a.png').read_bytes() == _pil_bytes(a, 6)           # complete here, not at close()
        w.write_many([a[:, :, 0], a[:, :, 1]], [str(tmp_path / 'g0.png'), str(tmp_path / 'g1.png')], 'grey')
        assert (tmp_path / 'g1.png').read_bytes() == _pil_bytes(np.ascontiguousarray(a[:, :, 1]), 6)
    assert w.paths == [str(tmp_path / n) for n in ('a.png', 'g0.png', 'g1.png')] and w.waited == 0.0
    with pytest.raises(ValueError, match='paths'):
        png.FileWriter(False, 0).write_many([a], [])


def test_host_mode_bounds_the_calls_in_flight_and_keeps_submission_order(tmp_path):
    """two threads, at most two calls outstanding: the third write() returns only after the first job is done"""
    from dasr_amd import png
    paths = [str(tmp_path / ('%d.png' % k)) for k in range(3)]
    gates = {p: threading.Event() for p in paths}
    done = []

    def saver(array, path, fmt, level):
        assert gates[path].wait(30)
        png.save_host(array, path, fmt, level)
        done.append(path)
        return path
    images = [png.photo(5, 7, k) for k in range(3)]
    times = {}
    w = png.FileWriter(False, 2, max_pending=2, compress_level=3, save=saver)
    w.times = times
    assert w.threads == 2 and w.max_pending == 2
    w.write(images[0], paths[0])
    w.write(images[1], paths[1])                                                # both return at once: their jobs are blocked
    returned = threading.Event()

    def third():
        w.write(images[2], paths[2])
        returned.set()
    t = threading.Thread(target=third)
    t.start()
    while len(w.paths) < 3 and t.is_alive():                                    # the third job is handed over ...
        pass
    assert not returned.wait(0.05) and not done                                 # ... and its call waits for the oldest
    gates[paths[0]].set()
    assert returned.wait(30) and done == [paths[0]]
    t.join()
    gates[paths[1]].set()
    gates[paths[2]].set()
    w.close()
    assert w.paths == paths and sorted(done) == paths
    assert [open(p, 'rb').read() for p in paths] == [_pil_bytes(a, 3) for a in images]
    assert w.waited > 0.0 and times['encode_wait'] == pytest.approx(w.waited) and times['submit'] >= 0.0 and 'device_png' not in times


def test_close_raises_the_first_failure_after_the_other_files_are_complete(tmp_path):
    from dasr_amd import png
    paths = [str(tmp_path / ('%d.png' % k)) for k in range(3)]

    def saver(array, path, fmt, level):
        if path == paths[1]:
            raise OSError('no room for ' + path)
        return png.save_host(array, path, fmt, level)
    a = png.photo(33, 20, 2)
    w = png.FileWriter(False, 2, max_pending=2, save=saver)
    for p in paths:
        w.write(a, p)
    with pytest.raises(OSError, match='no room for .*1.png'):
        w.close()
    assert open(paths[0], 'rb').read() == open(paths[2], 'rb').read() == _pil_bytes(a, 6) and not (tmp_path / '1.png').exists()
    w.close()                                                                   # (a second close is a no-op)
    with pytest.raises(ValueError, match='close'):
        w.write(a, paths[0])
    with pytest.raises(OSError):                                                # leaving the block raises it too
        with png.FileWriter(False, 2, save=saver) as w2:
            w2.write(a, paths[1])


@pytest.mark.parametrize('hw', SIZES)
@pytest.mark.parametrize('fmt', ['rgb', 'bgr', 'grey'])
def test_save_host_pixels_mode_and_bytes(tmp_path, fmt, hw):
    from PIL import Image
    from dasr_amd import png
    a = png.photo(hw[0], hw[1], 10 * hw[0] + hw[1])
    a = np.ascontiguousarray(a[:, :, 0]) if fmt == 'grey' else a
    want = np.ascontiguousarray(a[:, :, ::-1]) if fmt == 'bgr' else a
    for level in (3, 6):
        path = str(tmp_path / ('%s_%d.png' % (fmt, level)))
        assert png.save_host(a, path, fmt, level) == path
        with Image.open(path) as im:
            assert im.format == 'PNG' and im.mode == ('L' if fmt == 'grey' else 'RGB') and np.array_equal(np.array(im), want)
        assert open(path, 'rb').read() == _pil_bytes(want, level)
    assert open(png.save_host(a, str(tmp_path / 'd.png'), fmt), 'rb').read() == _pil_bytes(want, 6)      # the default level is PIL's
    view = np.concatenate([a, a], axis=1)[:, :hw[1]]                             # a window of a wider image: rows with a pitch
    assert not view.flags['C_CONTIGUOUS']
    assert open(png.save_host(view, str(tmp_path / 'v.png'), fmt, 3), 'rb').read() == _pil_bytes(want, 3)
    assert open(png.save_host(a, str(tmp_path / 'x.jpg'), fmt), 'rb').read()[:8] == png.SIGNATURE        # 'PNG' whatever the extension says


def test_save_host_refusals_and_save_img(tmp_path):
    from dasr_amd import png, util
    a = png.photo(5, 7, 3)
    for bad, fmt in ((a, 'grey'), (a[:, :, 0], 'rgb'), (a[:, :, 0], 'bgr'), (a.astype(np.float32), 'rgb')):
        with pytest.raises(ValueError, match='uint8'):
            png.save_host(bad, str(tmp_path / 'bad.png'), fmt)
    with pytest.raises(ValueError, match='fmt'):
        png.save_host(a, str(tmp_path / 'bad.png'), 'rgba')
    assert not (tmp_path / 'bad.png').exists()
    util.save_img(a, str(tmp_path / 'c.png'))                                    # BGR in, the RGB file of the reversed channels
    util.save_img(a[:, :, 0], str(tmp_path / 'g.png'))
    assert (tmp_path / 'c.png').read_bytes() == _pil_bytes(np.ascontiguousarray(a[:, :, ::-1]), 6)
    assert (tmp_path / 'g.png').read_bytes() == _pil_bytes(np.ascontiguousarray(a[:, :, 0]), 6)


def test_prepare_data_sub_and_mod_folders_are_pil_level_3_files_of_the_slices(tmp_path):
    """one 100 x 130 file, crop 48, step 24, threshold 8, scale 3: rows 0, 24, 48 (4 <= 8 remain), columns 0, 24, 48, 72 and 82 (10 > 8 remain); 48 is a multiple of 3, so
    a mod file holds the pixels of its sub file.  No device is opened for these two folders."""
    from PIL import Image
    from dasr_amd import prepare_data
    img = np.random.RandomState(3).randint(0, 256, (100, 130, 3)).astype(np.uint8)
    hr = tmp_path / 'HR'
    hr.mkdir()
    Image.fromarray(img).save(str(hr / 'a.png'))
    written = prepare_data.main(['--input_dir', str(hr), '--sub_dir', str(tmp_path / 'sub'), '--mod_dir', str(tmp_path / 'mod'), '--crop_sz', '48', '--step', '24',
                                 '--thres_sz', '8', '--scale', '3', '--num_workers', '2'])
    grid = [(y, x) for y in (0, 24, 48) for x in (0, 24, 48, 72, 82)]
    assert list(written) == ['sub', 'mod']
    for key in ('sub', 'mod'):
        assert written[key] == [str(tmp_path / key / ('a_s%03d.png' % (k + 1))) for k in range(15)]
        assert sorted(p.name for p in (tmp_path / key).iterdir()) == ['a_s%03d.png' % (k + 1) for k in range(15)]
        for path, (y, x) in zip(written[key], grid):
            assert open(path, 'rb').read() == _pil_bytes(np.ascontiguousarray(img[y:y + 48, x:x + 48]), 3), path


def _file(path, mode, size=(7, 5)):
    from PIL import Image
    shape = {'RGB': (size[1], size[0], 3), 'RGBA': (size[1], size[0], 4), 'L': (size[1], size[0]), 'P': (size[1], size[0])}[mode]
    im = Image.fromarray(np.random.RandomState(5).randint(0, 256, shape).astype(np.uint8), 'L' if mode == 'P' else mode)
    (im.convert('P') if mode == 'P' else im).save(str(path))
    return str(path)


@pytest.mark.parametrize('mode', ['L', 'P', 'RGBA'])
def test_rgb8_header_refuses_other_modes(tmp_path, mode):
    from dasr_amd import imgio
    path = _file(tmp_path / ('b_%s.png' % mode), mode)
    with pytest.raises(ValueError) as e:
        imgio.rgb8_header(path)
    assert path in str(e.value) and 'mode %s,' % mode in str(e.value) and 'RGB' in str(e.value)


def test_rgb8_header_refuses_a_side_above_65535(tmp_path):
    from PIL import Image
    from dasr_amd import imgio
    path = str(tmp_path / 'tall.png')
    Image.new('RGB', (1, 65536)).save(path)
    with pytest.raises(ValueError) as e:
        imgio.rgb8_header(path)
    assert path in str(e.value) and '65536 x 1' in str(e.value) and '65535' in str(e.value)


def test_rgb8_header_sizes_and_the_width_of_the_device_encoder(tmp_path):
    from dasr_amd import imgio, png
    path = _file(tmp_path / 'a.png', 'RGB')
    widest = png.max_width('rgb')
    assert imgio.rgb8_header(path) == imgio.rgb8_header(path, True) == imgio.rgb8_header(path, True, widest) == (5, 7)
    assert imgio.rgb8_header(path, False, widest + 1) == (5, 7)                  # (only the device encoder has a widest row)
    with pytest.raises(ValueError) as e:
        imgio.rgb8_header(path, True, widest + 1)
    assert path in str(e.value) and '--device_png' in str(e.value) and str(widest) in str(e.value) and 'a unit here has %d' % (widest + 1) in str(e.value)


def test_refuse_filled_folder_names_the_flag(tmp_path):
    from dasr_amd import util
    util.refuse_filled_folder(str(tmp_path / 'absent'), '--lr_dir')
    util.refuse_filled_folder(str(tmp_path), '--lr_dir')                          # an empty folder is fine
    (tmp_path / 'old.png').write_bytes(b'x')
    with pytest.raises(ValueError) as e:
        util.refuse_filled_folder(str(tmp_path), '--lr_dir')
    assert '--lr_dir %s' % tmp_path in str(e.value) and '--overwrite' in str(e.value)
    assert (tmp_path / 'old.png').read_bytes() == b'x'


def test_tick_measures_only_into_a_dict():
    import time
    from dasr_amd import imgio
    t0 = time.perf_counter()
    assert imgio.tick(None, 'a', t0, sync=True) >= t0                            # nothing measured: nothing synchronised, no device needed
    times = {'a': 1.0}
    t1 = imgio.tick(times, 'a', t0)
    assert 1.0 <= times['a'] <= 1.0 + (t1 - t0) and imgio.tick(times, 'b', t1) >= t1 and 0.0 <= times['b'] < 1.0
