"""Host side of the DSN corruption step (dasr_amd/corrupt.py, add_corruptions.py, csrc/corrupt.hip; reference: codes/DSN/add_corruptions.py, utils.py:20-22): the integer
restatement of the JPEG round trip against PIL's own outputs (tests/golden/jpeg_roundtrip.npz, written by scripts/gen_golden_jpeg.py) and against PIL live, the noise
generator against its published known answer and its statistics, the rounding margins the GPU tests rely on, the entry points in header, binding and library, and what
the CLI parses, pairs up and refuses before it writes.  No device."""
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_roundtrip.npz')
ENTRY_POINTS = {'dasr_jpeg_blocks': 7, 'dasr_jpeg_merge': 6, 'dasr_noise_u8': 8}

# the noise cases of tests/test_gpu_corrupt.py (the same table stands there): image shapes, standard deviations, seeds (the second has bits in both key words), indices
NOISE_SHAPES = ((1, 1, 3), (1, 3, 3), (7, 9, 3), (64, 48, 3))
NOISE_STDS = (0.5, 8.0, 40.0)
NOISE_SEEDS = (1, 0x9E3779B97F4A7C15)
NOISE_INDICES = (0, 5)
# the CLI cases of tests/test_gpu_corrupt.py: file sizes in sorted order, seed, noise
CLI_SIZES = ((16, 16), (40, 24), (37, 53))
CLI_SEED, CLI_STD = 11, 8.0


def _golden():
    """{name: uint8 [H, W, 3]}, version strings (the reader of scripts/gen_golden_jpeg.py)"""
    z = np.load(GOLDEN)
    ends = np.cumsum(z['shapes'].prod(axis=1))
    return {str(n): z['blob'][e - s[0] * s[1] * s[2]:e].reshape(s) for n, s, e in zip(z['names'], z['shapes'], ends)}, [str(v) for v in z['versions']]


def _cases(arrays):
    """[(name of the output, input, quality, PIL's output)]"""
    out = []
    for name, a in arrays.items():
        m = re.match(r'out_(\d+x\d+_\w+)_q(\d+)$', name)
        if m:
            out.append((name, arrays['in_' + m.group(1)], int(m.group(2)), a))
    return out


def test_fixture_holds_the_sizes_qualities_and_contents():
    arrays, versions = _golden()
    assert os.path.getsize(GOLDEN) < 300 * 1024
    assert len(versions) == 3 and versions[2] == 'libjpeg_turbo=True'
    cases = _cases(arrays)
    sizes = {(1, 1), (2, 2), (3, 5), (5, 4), (8, 8), (16, 16), (17, 33), (40, 24), (31, 6), (37, 53), (64, 48), (50, 130)}
    contents = {'random', 'constant', 'checker', 'primaries', 'gradient'}
    want = {'out_%dx%d_%s_q%d' % (h, w, c, q) for h, w in sizes for c in contents for q in ((30, 1, 5, 50, 75, 95, 100) if (h, w) in ((17, 33), (40, 24)) else (30,))}
    assert {c[0] for c in cases} == want
    for name, a, q, b in cases:
        h, w = (int(v) for v in name.split('_')[1].split('x'))
        assert a.shape == b.shape == (h, w, 3) and a.dtype == b.dtype == np.uint8, name


def test_jpeg_restatement_equals_the_fixture_bit_for_bit():
    from dasr_amd.corrupt import jpeg_roundtrip_ref
    arrays, _ = _golden()
    for name, a, q, want in _cases(arrays):
        got = jpeg_roundtrip_ref(a, q)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, int((got != want).sum()))


def test_jpeg_restatement_equals_pil_live():
    """PIL computed here on the same inputs and a few more sizes; only where this PIL is linked against libjpeg-turbo (another decoder may up-sample differently)"""
    from PIL import Image, features
    if not features.check('libjpeg_turbo'):
        pytest.skip('this PIL is not built on libjpeg-turbo')
    from dasr_amd.corrupt import jpeg_roundtrip_ref

    def pil(a, q):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, 'JPEG', quality=q)
        buf.seek(0)
        return np.array(Image.open(buf))
    arrays, _ = _golden()
    for name, a, q, _ in _cases(arrays):
        assert np.array_equal(jpeg_roundtrip_ref(a, q), pil(a, q)), name
    rng = np.random.RandomState(5)
    for k in range(60):
        h, w, q = rng.randint(1, 70), rng.randint(1, 70), rng.randint(1, 101)
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        if k % 3 == 1:
            a = (a // 128 * 255).astype(np.uint8)   # posterised: the range extremes
        assert np.array_equal(jpeg_roundtrip_ref(a, q), pil(a, q)), (h, w, q)


def test_jpeg_restatement_refuses_bad_arguments():
    from dasr_amd.corrupt import jpeg_roundtrip_ref, quant_tables
    a = np.zeros((4, 4, 3), np.uint8)
    for q in (0, 101, -3, 30.5):
        with pytest.raises(ValueError):
            jpeg_roundtrip_ref(a, q)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            jpeg_roundtrip_ref(bad, 30)
    qy, qc = quant_tables(30)   # s = 5000 // 30 = 166: (16 * 166 + 50) // 100 = 27, (17 * 166 + 50) // 100 = 28, 99 -> 164
    assert qy[0, 0] == 27 and qc[0, 0] == 28 and qc[7, 7] == 164
    assert quant_tables(100)[0].max() == 1 and quant_tables(1)[0].max() == 255


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: counter 0, key 0; and all ones"""
    from dasr_amd.corrupt import philox4x32
    assert [int(v) for v in philox4x32((0, 0, 0, 0), (0, 0))] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = 0xffffffff
    assert [int(v) for v in philox4x32((ones,) * 4, (ones, ones))] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_normal_samples_have_mean_0_and_deviation_1():
    from dasr_amd.corrupt import normal_ref
    z = normal_ref(10 ** 6, 3, 2)
    assert z.shape == (10 ** 6,) and np.isfinite(z).all()
    assert abs(z.mean()) < 0.005 and abs(z.std() - 1.0) < 0.005
    assert np.array_equal(normal_ref(9, 3, 2), z[:9])   # (a last group of one: a prefix of the same stream)


def test_noise_clamps_and_depends_on_seed_and_index_only():
    from dasr_amd.corrupt import gaussian_noise_ref
    img = np.zeros((32, 32, 3), np.uint8)
    img[16:] = 255
    out = gaussian_noise_ref(img, 40.0, 1, 0)
    assert out.dtype == np.uint8 and out.shape == img.shape
    assert (out[:16] == 0).mean() > 0.4 and (out[16:] == 255).mean() > 0.4 and out[:16].max() > 60 and out[16:].min() < 195   # half of the noise is cut off at either end
    assert np.array_equal(out, gaussian_noise_ref(img, 40.0, 1, 0))
    assert not np.array_equal(out, gaussian_noise_ref(img, 40.0, 1, 1)) and not np.array_equal(out, gaussian_noise_ref(img, 40.0, 2, 0))
    assert not np.array_equal(out, gaussian_noise_ref(img, 40.0, 1 + (1 << 32), 0))   # the high key word counts
    assert np.array_equal(gaussian_noise_ref(img, 0.0, 1, 0), img)
    grey = np.full((8, 8, 3), 128, np.uint8)
    d = gaussian_noise_ref(grey, 8.0, 1, 0).astype(int) - 128
    assert d.min() < -8 and d.max() > 8


def test_no_noise_sample_of_the_gpu_cases_lies_at_a_rounding_boundary():
    """the device computes log, sqrt, cos and sin in fp64 with its own library: std z may differ from the host's in the last bits, which changes rint only within a few
    ulp of a half-integer.  For every case the GPU tests compare bit for bit, no std z lies within 1e-9 of one (the seeds were chosen so)."""
    from dasr_amd.corrupt import normal_ref
    cases = [(int(np.prod(s)), std, seed, idx) for s in NOISE_SHAPES for std in NOISE_STDS for seed in NOISE_SEEDS for idx in NOISE_INDICES]
    cases += [(h * w * 3, CLI_STD, CLI_SEED, k) for k, (h, w) in enumerate(CLI_SIZES)]
    cases += [(17 * 33 * 3, 8.0, NOISE_SEEDS[0], k) for k in (2, 3, 4)]   # the batch case: images 2, 3, 4
    for n, std, seed, idx in cases:
        v = std * normal_ref(n, seed, idx)
        assert np.abs(v - np.floor(v) - 0.5).min() > 1e-9, (n, std, seed, idx)


def test_entry_points_in_header_binding_and_library():
    from dasr_amd import _lib, build, corrupt
    header = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert name in _lib._SIGS and len(_lib._SIGS[name]) == nargs, name
    assert re.search(r'^#define DASR_ABI_VERSION 22$', header, flags=re.M) and _lib.ABI_VERSION == 22   # additions only
    assert 'corrupt.hip' in build.SOURCES + build.MORE_SOURCES and os.path.exists(build.build())
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    data = open(_lib.LIB_PATH, 'rb').read()
    assert b'jpeg_blocks_kernel' in data and b'jpeg_merge_kernel' in data and b'noise_u8_kernel' in data
    # DASR_JPEG_PLANE_BYTES of the header: Y 40 x 24, chroma ceil8(20) x (ceil16(24) / 2) = 24 x 16
    assert corrupt.plane_bytes(40, 24) == 40 * 24 + 2 * 24 * 16 and corrupt.plane_bytes(1, 1) == 64 + 2 * 64 and corrupt.plane_bytes(17, 33) == 24 * 40 + 2 * 16 * 24


def test_device_functions_refuse_host_tensors():
    import torch
    from dasr_amd import corrupt
    for bad in (torch.zeros(4, 4, 3, dtype=torch.uint8), np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            corrupt.jpeg_roundtrip(bad, 30)
        with pytest.raises(ValueError):
            corrupt.gaussian_noise(bad, 8.0, 0, 0)
    with pytest.raises(ValueError):
        corrupt.jpeg_roundtrip(torch.zeros(4, 4, 3, dtype=torch.uint8), 0)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------
def _png(path, mode='RGB', size=(6, 5), seed=3):
    from PIL import Image
    rng = np.random.RandomState(seed)
    shape = {'RGB': (size[0], size[1], 3), 'RGBA': (size[0], size[1], 4), 'L': size, 'P': size}[mode]
    im = Image.fromarray(rng.randint(0, 256, shape).astype(np.uint8), 'L' if mode == 'P' else mode)
    (im.convert('P') if mode == 'P' else im).save(str(path))


def test_flags_have_the_reference_defaults_and_accept_none():
    from dasr_amd.add_corruptions import parse_args
    o = parse_args([])
    assert (o.noise_std_dev, o.blur_std_dev, o.jpg_quality, o.artifacts, o.dataset, o.resolution) == (8.0, None, 30, 'gaussian', 'df2k', 'hr')
    assert (o.seed, o.overwrite, o.input_dir, o.output_dir) == (0, False, None, None)
    o = parse_args(['--noise_std_dev', 'None', '--jpg_quality', 'none', '--blur_std_dev', '1.6', '--resolution', 'lr'])
    assert o.noise_std_dev is None and o.jpg_quality is None and o.blur_std_dev == 1.6 and o.resolution == 'lr'
    o = parse_args(['--noise_std_dev', 'NONE', '--jpg_quality', '75', '--blur_std_dev', 'None', '--seed', '9', '--input_dir', 'a', '--output_dir', 'b',
                    '--input_dir', 'c', '--output_dir', 'd'])
    assert o.noise_std_dev is None and o.jpg_quality == 75 and o.blur_std_dev is None and o.seed == 9 and o.input_dir == ['a', 'c'] and o.output_dir == ['b', 'd']
    with pytest.raises(SystemExit):
        parse_args(['--jpg_quality', 'thirty'])
    with pytest.raises(SystemExit):
        parse_args(['--resolution', 'mid'])


def test_folders_come_from_the_yaml_file_or_from_pairs(tmp_path):
    from dasr_amd.add_corruptions import folder_pairs, parse_args
    y = tmp_path / 'paths.yml'
    y.write_text('df2k:\n  clean:\n    hr: {train: /c/hr/t, valid: /c/hr/v}\n    lr: {train: /c/lr/t, valid: /c/lr/v}\n'
                 '  gaussian:\n    hr: {train: /g/hr/t, valid: /g/hr/v}\n  jpeg:\n    lr: {train: /j/lr/t, valid: /j/lr/v}\n')
    assert folder_pairs(parse_args(['--paths', str(y)])) == [('/c/hr/t', '/g/hr/t'), ('/c/hr/v', '/g/hr/v')]
    assert folder_pairs(parse_args(['--paths', str(y), '--artifacts', 'jpeg', '--resolution', 'lr'])) == [('/c/lr/t', '/j/lr/t'), ('/c/lr/v', '/j/lr/v')]
    with pytest.raises(KeyError):
        folder_pairs(parse_args(['--paths', str(y), '--artifacts', 'jpeg']))          # no ['jpeg']['hr']
    with pytest.raises(KeyError):
        folder_pairs(parse_args(['--paths', str(y), '--dataset', 'other']))
    assert folder_pairs(parse_args(['--paths', str(y), '--input_dir', 'a', '--output_dir', 'b'])) == [('a', 'b')]   # the pairs win
    with pytest.raises(ValueError):
        folder_pairs(parse_args(['--input_dir', 'a', '--input_dir', 'c', '--output_dir', 'b']))
    with pytest.raises(ValueError):
        folder_pairs(parse_args(['--input_dir', 'a']))


def test_plan_lists_the_files_in_sorted_order_with_their_indices(tmp_path):
    from dasr_amd.add_corruptions import parse_args, plan
    src, src2 = tmp_path / 'in', tmp_path / 'in2'
    src.mkdir()
    src2.mkdir()
    for k, name in enumerate(('b.png', 'a.png', 'c.PNG', 'notes.txt')):
        if name.endswith('.txt'):
            (src / name).write_text('x')
        else:
            _png(src / name, size=(5 + k, 7))
    _png(src2 / 'z.png')
    work = plan(parse_args(['--input_dir', str(src), '--output_dir', str(tmp_path / 'out'), '--input_dir', str(src2), '--output_dir', str(tmp_path / 'out2')]))
    assert [d for d, _ in work] == [str(tmp_path / 'out'), str(tmp_path / 'out2')]
    assert [(os.path.basename(f[0]), os.path.basename(f[1]), f[2], f[3], f[4]) for f in work[0][1]] == [('a.png', 'a.png', 0, 6, 7), ('b.png', 'b.png', 1, 5, 7), ('c.PNG', 'c.PNG', 2, 7, 7)]
    assert [(os.path.basename(f[0]), f[2]) for f in work[1][1]] == [('z.png', 0)]
    assert all(os.path.dirname(f[1]) == str(tmp_path / 'out') for f in work[0][1])
    assert not (tmp_path / 'out').exists()   # plan writes nothing


@pytest.mark.parametrize('mode', ['L', 'P', 'RGBA'])
def test_cli_refuses_grey_palette_and_alpha_files_before_it_writes(tmp_path, mode):
    from dasr_amd.add_corruptions import main
    src = tmp_path / 'in'
    src.mkdir()
    _png(src / 'a.png')
    _png(src / 'b.png', mode)
    with pytest.raises(ValueError, match='b.png'):
        main(['--input_dir', str(src), '--output_dir', str(tmp_path / 'out')])
    assert not (tmp_path / 'out').exists()


def test_cli_refuses_bad_flags_and_folders_before_it_writes(tmp_path):
    from dasr_amd.add_corruptions import main
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    _png(src / 'a.png')
    base = ['--input_dir', str(src), '--output_dir', str(out)]
    with pytest.raises(ValueError, match='no stage'):
        main(base + ['--noise_std_dev', 'None', '--jpg_quality', 'None'])
    for q in ('0', '101', '-5'):
        with pytest.raises(ValueError, match='jpg_quality'):
            main(base + ['--jpg_quality', q])
    with pytest.raises(ValueError, match='noise_std_dev'):
        main(base + ['--noise_std_dev', '-1'])
    with pytest.raises(ValueError, match='own input'):
        main(['--input_dir', str(src), '--output_dir', str(src)])
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(ValueError, match='no image files'):
        main(['--input_dir', str(empty), '--output_dir', str(out)])
    with pytest.raises(ValueError, match='does not exist'):
        main(['--input_dir', str(tmp_path / 'missing'), '--output_dir', str(out)])
    assert not out.exists()


def test_cli_refuses_a_filled_output_folder_without_overwrite(tmp_path):
    from dasr_amd.add_corruptions import main, parse_args, plan
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    out.mkdir()
    _png(src / 'a.png')
    base = ['--input_dir', str(src), '--output_dir', str(out)]
    assert len(plan(parse_args(base))[0][1]) == 1          # an empty folder is fine
    (out / 'a.png').write_bytes(b'kept')
    with pytest.raises(ValueError, match='--overwrite'):
        main(base)
    assert (out / 'a.png').read_bytes() == b'kept'
    assert len(plan(parse_args(base + ['--overwrite']))[0][1]) == 1
