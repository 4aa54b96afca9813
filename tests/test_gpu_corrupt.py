"""GPU: the DSN corruption step (dasr_amd/corrupt.py, csrc/corrupt.hip, `python -m dasr_amd.add_corruptions`; reference: codes/DSN/add_corruptions.py).  The JPEG round
trip against its integer restatement and against PIL's own outputs (tests/golden/jpeg_roundtrip.npz), the noise against its restatement, both bit for bit, what the
entry points refuse, and the CLI end to end.

The noise cases are those for which tests/test_corrupt_host.py shows that no std z lies within 1e-9 of a rounding boundary: the device's fp64 log / sqrt / cos / sin may
differ from the host's in the last bits, which cannot move rint there."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_roundtrip.npz')
EINVAL = -22

# (the same table stands in tests/test_corrupt_host.py, which checks the rounding margins of exactly these cases)
NOISE_SHAPES = ((1, 1, 3), (1, 3, 3), (7, 9, 3), (64, 48, 3))
NOISE_STDS = (0.5, 8.0, 40.0)
NOISE_SEEDS = (1, 0x9E3779B97F4A7C15)
NOISE_INDICES = (0, 5)
CLI_SIZES = ((16, 16), (40, 24), (37, 53))
CLI_SEED, CLI_STD = 11, 8.0


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def _stream():
    return torch.cuda.current_stream().cuda_stream


_CACHE = {}


def _golden_cases():
    """[(name, input, quality, PIL's output)] of the fixture, read once"""
    if 'cases' not in _CACHE:
        z = np.load(GOLDEN)
        ends = np.cumsum(z['shapes'].prod(axis=1))
        arrays = {str(n): z['blob'][e - s[0] * s[1] * s[2]:e].reshape(s) for n, s, e in zip(z['names'], z['shapes'], ends)}
        cases = []
        for name, a in arrays.items():
            m = re.match(r'out_(\d+x\d+_\w+)_q(\d+)$', name)
            if m:
                cases.append((name, arrays['in_' + m.group(1)], int(m.group(2)), a))
        _CACHE['cases'] = cases
    return _CACHE['cases']


# ---- 1. the JPEG round trip -------------------------------------------------------------------------------------------------------------------
def test_jpeg_roundtrip_equals_the_restatement_and_pil_bit_for_bit():
    """every size, quality and content of the fixture; the input is left as it was"""
    dev = _gpu()
    from dasr_amd.corrupt import jpeg_roundtrip, jpeg_roundtrip_ref
    cases = _golden_cases()
    assert len(cases) == 120
    inputs = [torch.from_numpy(a.copy()).to(dev) for _, a, _, _ in cases]
    outs = [jpeg_roundtrip(x, q) for x, (_, _, q, _) in zip(inputs, cases)]   # (all enqueued before the first read-back)
    for x, y, (name, a, q, want) in zip(inputs, outs, cases):
        got = y.cpu().numpy()
        assert y.dtype == torch.uint8 and y.shape == x.shape and y.data_ptr() != x.data_ptr(), name
        assert np.array_equal(got, want), (name, 'fixture', int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got, jpeg_roundtrip_ref(a, q)), (name, 'restatement')
        assert np.array_equal(x.cpu().numpy(), a), (name, 'input changed')


def test_jpeg_roundtrip_of_a_batch_equals_its_single_calls():
    dev = _gpu()
    from dasr_amd.corrupt import jpeg_roundtrip, jpeg_roundtrip_ref
    batch = np.random.RandomState(21).randint(0, 256, (3, 17, 33, 3)).astype(np.uint8)
    x = torch.from_numpy(batch).to(dev)
    y = jpeg_roundtrip(x, 30)
    assert y.shape == x.shape
    for k in range(3):
        assert torch.equal(y[k], jpeg_roundtrip(x[k], 30)), k
        assert np.array_equal(y[k].cpu().numpy(), jpeg_roundtrip_ref(batch[k], 30)), k
    assert np.array_equal(x.cpu().numpy(), batch)


def test_jpeg_roundtrip_on_views_and_unaligned_storage():
    """a non-contiguous view is made contiguous; an image at an odd byte offset of its storage goes through the byte path of loads and stores"""
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.corrupt import jpeg_roundtrip, jpeg_roundtrip_ref, plane_bytes
    a = np.random.RandomState(22).randint(0, 256, (24, 40, 3)).astype(np.uint8)
    x = torch.from_numpy(a).to(dev)
    assert np.array_equal(jpeg_roundtrip(x[3:20, 2:35], 50).cpu().numpy(), jpeg_roundtrip_ref(a[3:20, 2:35], 50))
    H, W = 17, 33
    src = torch.zeros(H * W * 3 + 8, dtype=torch.uint8, device=dev)
    dst = torch.zeros(H * W * 3 + 8, dtype=torch.uint8, device=dev)
    img = np.ascontiguousarray(a[:H, :W])
    src[1:1 + H * W * 3] = torch.from_numpy(img.reshape(-1)).to(dev)
    planes = torch.empty(plane_bytes(H, W), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    assert L.dasr_jpeg_blocks(src.data_ptr() + 1, 1, H, W, 30, planes.data_ptr(), _stream()) == 0
    assert L.dasr_jpeg_merge(planes.data_ptr(), 1, H, W, dst.data_ptr() + 3, _stream()) == 0
    got = dst.cpu().numpy()
    assert np.array_equal(got[3:3 + H * W * 3].reshape(H, W, 3), jpeg_roundtrip_ref(img, 30))
    assert not got[:3].any() and not got[3 + H * W * 3:].any()   # nothing written around the image


def test_jpeg_entry_points_refuse_bad_arguments():
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.corrupt import jpeg_roundtrip, plane_bytes
    L = _lib.lib()
    x = torch.zeros(8, 8, 3, dtype=torch.uint8, device=dev)
    p = torch.zeros(plane_bytes(8, 8) + 8, dtype=torch.uint8, device=dev)
    s = _stream()
    assert L.dasr_jpeg_blocks(None, 1, 8, 8, 30, p.data_ptr(), s) == EINVAL and L.dasr_jpeg_blocks(x.data_ptr(), 1, 8, 8, 30, None, s) == EINVAL
    for N, H, W, q in ((0, 8, 8, 30), (65536, 8, 8, 30), (1, 0, 8, 30), (1, 8, 0, 30), (1, 65536, 8, 30), (1, 8, 8, 0), (1, 8, 8, 101)):
        assert L.dasr_jpeg_blocks(x.data_ptr(), N, H, W, q, p.data_ptr(), s) == EINVAL, (N, H, W, q)
    assert L.dasr_jpeg_blocks(x.data_ptr(), 1, 8, 8, 30, p.data_ptr() + 4, s) == EINVAL   # planes not 8-byte aligned
    assert L.dasr_jpeg_merge(p.data_ptr(), 1, 8, 8, p.data_ptr(), s) == EINVAL and L.dasr_jpeg_merge(p.data_ptr(), 1, 8, 8, None, s) == EINVAL
    assert L.dasr_jpeg_merge(p.data_ptr() + 4, 1, 8, 8, x.data_ptr(), s) == EINVAL
    torch.cuda.synchronize()
    assert not x.cpu().numpy().any() and not p.cpu().numpy().any()   # nothing was launched
    for bad in (x.float(), x[..., :2], x.cpu()):
        with pytest.raises(ValueError):
            jpeg_roundtrip(bad, 30)
    with pytest.raises(ValueError):
        jpeg_roundtrip(x, 0)


# ---- 2. the noise -----------------------------------------------------------------------------------------------------------------------------
def test_gaussian_noise_equals_the_restatement_bit_for_bit():
    dev = _gpu()
    from dasr_amd.corrupt import gaussian_noise, gaussian_noise_ref
    jobs = []
    for k, shape in enumerate(NOISE_SHAPES):
        a = np.random.RandomState(40 + k).randint(0, 256, shape).astype(np.uint8)
        if shape[0] >= 7:
            a[0], a[-1] = 0, 255   # rows that the clamp cuts at either end
        x = torch.from_numpy(a).to(dev)
        for std in NOISE_STDS:
            for seed in NOISE_SEEDS:
                for idx in NOISE_INDICES:
                    jobs.append((a, x, std, seed, idx, gaussian_noise(x, std, seed, idx)))
    for a, x, std, seed, idx, y in jobs:
        want = gaussian_noise_ref(a, std, seed, idx)
        got = y.cpu().numpy()
        assert y.dtype == torch.uint8 and y.shape == x.shape and y.data_ptr() != x.data_ptr()
        assert np.array_equal(got, want), (a.shape, std, seed, idx, int((got != want).sum()))
        assert np.array_equal(x.cpu().numpy(), a)
    a = jobs[-1][0]
    assert torch.equal(gaussian_noise(jobs[-1][1], 0.0, 1, 0), jobs[-1][1])   # std 0 returns the input's bytes
    assert not np.array_equal(gaussian_noise_ref(a, 8.0, 1, 0), gaussian_noise_ref(a, 8.0, 1, 5))


def test_gaussian_noise_of_a_batch_counts_the_index_up():
    dev = _gpu()
    from dasr_amd.corrupt import gaussian_noise, gaussian_noise_ref
    batch = np.random.RandomState(45).randint(0, 256, (3, 17, 33, 3)).astype(np.uint8)   # 1683 bytes per image: images 1 and 2 start off a word boundary
    y = gaussian_noise(torch.from_numpy(batch).to(dev), 8.0, NOISE_SEEDS[0], 2).cpu().numpy()
    for k in range(3):
        assert np.array_equal(y[k], gaussian_noise_ref(batch[k], 8.0, NOISE_SEEDS[0], 2 + k)), k


def test_noise_entry_point_refuses_bad_arguments():
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.corrupt import gaussian_noise
    L = _lib.lib()
    x = torch.zeros(4, 4, 3, dtype=torch.uint8, device=dev)
    y = torch.zeros_like(x)
    s = _stream()
    assert L.dasr_noise_u8(None, y.data_ptr(), 1, 48, 8.0, 1, 0, s) == EINVAL and L.dasr_noise_u8(x.data_ptr(), None, 1, 48, 8.0, 1, 0, s) == EINVAL
    for N, per, std, idx in ((0, 48, 8.0, 0), (65536, 48, 8.0, 0), (1, 0, 8.0, 0), (1, 48, -1.0, 0), (1, 48, float('nan'), 0), (1, 48, float('inf'), 0), (1, 48, 8.0, -1),
                             (1, 48, 8.0, 1 << 32), (2, 24, 8.0, (1 << 32) - 1)):
        assert L.dasr_noise_u8(x.data_ptr(), y.data_ptr(), N, per, std, 1, idx, s) == EINVAL, (N, per, std, idx)
    torch.cuda.synchronize()
    assert not y.cpu().numpy().any()
    for std in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            gaussian_noise(x, std, 1, 0)
    with pytest.raises(ValueError):
        gaussian_noise(x, 8.0, 1, -1)


# ---- 3. the CLI end to end ---------------------------------------------------------------------------------------------------------------------
def _cli_folder(tmp_path):
    """the three fixture inputs with random content as PNG files; returns (folder, {file name: (index in the sorted list, input, PIL's round trip at quality 30)})"""
    from PIL import Image
    by_name = {name: (a, want) for name, a, q, want in _golden_cases() if q == 30 and '_random_' in name}
    src = tmp_path / 'clean'
    src.mkdir()
    files = {}
    for k, (h, w) in enumerate(CLI_SIZES):
        a, want = by_name['out_%dx%d_random_q30' % (h, w)]
        name = 'img_%d.png' % k
        Image.fromarray(a).save(str(src / name))
        files[name] = (k, a, want)
    return src, files


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.format == 'PNG' and im.mode == 'RGB', path
        return np.array(im)


def test_cli_jpeg_alone_writes_pils_round_trip(tmp_path):
    _gpu()
    from dasr_amd.add_corruptions import main
    src, files = _cli_folder(tmp_path)
    out = tmp_path / 'jpeg'
    written = main(['--input_dir', str(src), '--output_dir', str(out), '--noise_std_dev', 'None', '--jpg_quality', '30'])
    assert written == [str(out / n) for n in sorted(files)] and sorted(os.listdir(str(out))) == sorted(files)
    for name, (_, a, want) in files.items():
        assert np.array_equal(_read(str(out / name)), want), name
        assert np.array_equal(_read(str(src / name)), a), name


def test_cli_noise_then_jpeg_and_noise_alone(tmp_path):
    _gpu()
    from dasr_amd.add_corruptions import main
    from dasr_amd.corrupt import gaussian_noise_ref, jpeg_roundtrip_ref
    src, files = _cli_folder(tmp_path)
    both, noise = tmp_path / 'both', tmp_path / 'noise'
    base = ['--input_dir', str(src), '--seed', str(CLI_SEED), '--noise_std_dev', str(CLI_STD), '--num_workers', '2']
    assert len(main(base + ['--output_dir', str(both), '--jpg_quality', '30'])) == 3
    assert len(main(base + ['--output_dir', str(noise), '--jpg_quality', 'None'])) == 3
    for name, (k, a, _) in files.items():
        noisy = gaussian_noise_ref(a, CLI_STD, CLI_SEED, k)
        assert np.array_equal(_read(str(noise / name)), noisy), name
        assert np.array_equal(_read(str(both / name)), jpeg_roundtrip_ref(noisy, 30)), name
    assert not np.array_equal(_read(str(noise / 'img_0.png')), gaussian_noise_ref(files['img_0.png'][1], CLI_STD, CLI_SEED, 1))   # (the index matters)


def test_cli_blur_runs_between_noise_and_jpeg_as_pil_does_it(tmp_path, capsys):
    """--blur_std_dev is PIL's ImageFilter.GaussianBlur on the host, applied to the noisy image and before the JPEG round trip (add_corruptions.py:45-54), and logged"""
    _gpu()
    from PIL import Image, ImageFilter
    from dasr_amd.add_corruptions import main
    from dasr_amd.corrupt import gaussian_noise_ref, jpeg_roundtrip_ref
    src, files = _cli_folder(tmp_path)
    out, alone = tmp_path / 'all', tmp_path / 'blur'
    base = ['--input_dir', str(src), '--seed', str(CLI_SEED), '--blur_std_dev', '1.6']
    assert len(main(base + ['--output_dir', str(out), '--noise_std_dev', str(CLI_STD), '--jpg_quality', '30'])) == 3
    assert 'on the host' in capsys.readouterr().out
    assert len(main(base + ['--output_dir', str(alone), '--noise_std_dev', 'None', '--jpg_quality', 'None'])) == 3
    blur = lambda a: np.array(Image.fromarray(a).filter(ImageFilter.GaussianBlur(1.6)))
    for name, (k, a, _) in files.items():
        assert np.array_equal(_read(str(alone / name)), blur(a)), name
        assert np.array_equal(_read(str(out / name)), jpeg_roundtrip_ref(blur(gaussian_noise_ref(a, CLI_STD, CLI_SEED, k)), 30)), name


def test_cli_second_run_without_overwrite_raises_and_leaves_the_files(tmp_path):
    _gpu()
    from dasr_amd.add_corruptions import main
    src, files = _cli_folder(tmp_path)
    out = tmp_path / 'out'
    argv = ['--input_dir', str(src), '--output_dir', str(out), '--noise_std_dev', 'None']
    main(argv)
    before = {n: ((out / n).read_bytes(), os.stat(str(out / n)).st_mtime_ns) for n in files}
    with pytest.raises(ValueError, match='--overwrite'):
        main(argv)
    assert {n: ((out / n).read_bytes(), os.stat(str(out / n)).st_mtime_ns) for n in files} == before
    assert len(main(argv + ['--overwrite'])) == 3
    assert all((out / n).read_bytes() == before[n][0] for n in files)   # the same bytes again


def test_cli_reads_the_folders_from_the_yaml_file(tmp_path):
    _gpu()
    from PIL import Image
    from dasr_amd.add_corruptions import main
    from dasr_amd.corrupt import jpeg_roundtrip_ref
    rng = np.random.RandomState(50)
    imgs = {'train': rng.randint(0, 256, (9, 20, 3)).astype(np.uint8), 'valid': rng.randint(0, 256, (12, 7, 3)).astype(np.uint8)}
    for k, a in imgs.items():
        (tmp_path / 'clean' / k).mkdir(parents=True)
        Image.fromarray(a).save(str(tmp_path / 'clean' / k / 'x.png'))
    y = tmp_path / 'paths.yml'
    y.write_text('df2k:\n  clean:\n    lr: {train: %s, valid: %s}\n  jpeg:\n    lr: {train: %s, valid: %s}\n' % (
        tmp_path / 'clean' / 'train', tmp_path / 'clean' / 'valid', tmp_path / 'jpeg' / 'train', tmp_path / 'jpeg' / 'valid'))
    written = main(['--paths', str(y), '--artifacts', 'jpeg', '--resolution', 'lr', '--noise_std_dev', 'None', '--jpg_quality', '75'])
    assert written == [str(tmp_path / 'jpeg' / k / 'x.png') for k in ('train', 'valid')]
    for k, a in imgs.items():
        assert np.array_equal(_read(str(tmp_path / 'jpeg' / k / 'x.png')), jpeg_roundtrip_ref(a, 75)), k
