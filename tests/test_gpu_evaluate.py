"""GPU: the folder evaluator -- the 7 x 7 box SSIM and the channel sums of csrc/metrics.hip, metrics.pair_metrics_u8, the any-size LPIPS input stage
dasr_lpips_s2d_any, LPIPSAlexHIP.distance at sizes that are no multiple of 4, and the CLI dasr_amd.dsn_evaluate end to end -- against fp64 restatements of
codes/DSN/evaluate.py:44-52 written here (scikit-image's compare_ssim / compare_psnr restated from their algorithm; oracle.lpips for the network).

Bounds: device SSIM 1e-9 absolute (the project's bound for device SSIM; the integer form sits near 1e-15); PSNR from the exact integer sum bit-equal;
PSNR_col 1e-9 dB; the input stage 1e-6 relative with an identical zero pattern (fma against mul + add); LPIPS 1e-3 relative (ACT_TOL of test_gpu_lpips.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
SSIM_TOL, COL_TOL, ACT_TOL = 1e-9, 1e-9, 1e-3
ODD_SIZES = [(31, 31), (33, 46), (45, 38), (50, 35)]   # every residue mod 4 on both axes


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from dasr_amd import engine
    engine.ensure_runtime_ready()
    return torch.device('cuda')


def _pair(seed, n, c, h, w, kind='perturbed'):
    """two uint8 [n, c, h, w] arrays"""
    if kind == 'extremes':
        return np.full((n, c, h, w), 255, np.uint8), np.zeros((n, c, h, w), np.uint8)
    r = np.random.RandomState(seed)
    a = r.randint(0, 256, size=(n, c, h, w)).astype(np.uint8)
    if kind == 'identical':
        return a, a.copy()
    return a, np.clip(a.astype(np.int64) + r.randint(-20, 21, size=a.shape), 0, 255).astype(np.uint8)


def box_ssim_ref(a, b):
    """compare_ssim(X, Y, multichannel=True) on uint8 restated in fp64 in the uniform_filter form: per channel the filtered means ux, uy, uxx, uyy, uxy on the
    interior region (the window positions wholly inside the image), v = n / (n - 1) * (uxx - ux ux), the map S, its mean; then the mean of the channel means.
    a, b: uint8 [c, h, w]"""
    win = lambda x: np.lib.stride_tricks.sliding_window_view(x, (7, 7)).mean((-1, -2))
    cov_norm, C1, C2 = 49.0 / 48.0, (0.01 * 255) ** 2, (0.03 * 255) ** 2
    means = []
    for x, y in zip(a.astype(np.float64), b.astype(np.float64)):
        ux, uy, uxx, uyy, uxy = win(x), win(y), win(x * x), win(y * y), win(x * y)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        means.append(S.mean())
    return float(np.mean(means))


def _crop(x, c):
    return x[..., c:x.shape[-2] - c, c:x.shape[-1] - c]


def _device_box_ssim(dev, a, b, crop):
    from dasr_amd import _lib
    L = _lib.lib()
    n, c, h, w = a.shape
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    nbytes = L.dasr_img_ws_bytes(n, c, h, w, crop)
    assert nbytes > 0
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    out = torch.full((n,), float('nan'), dtype=torch.float64, device=dev)
    _lib.check(L.dasr_img_ssim_box(ta.data_ptr(), tb.data_ptr(), n, c, h, w, crop, out.data_ptr(), ws.data_ptr(), nbytes, None), 'dasr_img_ssim_box')
    torch.cuda.synchronize()
    return out.cpu()


BOX_CASES = [(1, 3, 7, 7, 0), (1, 3, 8, 13, 0), (1, 1, 8, 13, 0), (1, 3, 37, 53, 0), (1, 3, 45, 61, 4), (2, 3, 64, 96, 0)]


@pytest.mark.parametrize('kind', ['perturbed', 'extremes', 'identical'])
@pytest.mark.parametrize('n,c,h,w,crop', BOX_CASES, ids=['%dx%dx%dx%d-crop%d' % k for k in BOX_CASES])
def test_box_ssim_matches_the_fp64_uniform_filter_form(n, c, h, w, crop, kind, margins):
    dev = _gpu()
    a, b = _pair(h * w + crop, n, c, h, w, kind)
    got = _device_box_ssim(dev, a, b, crop)
    worst = 0.0
    for i in range(n):
        want = box_ssim_ref(_crop(a[i], crop), _crop(b[i], crop))
        worst = max(worst, abs(float(got[i]) - want))
        if kind == 'extremes':
            assert abs(want - 9.999000099989999e-05) < 1e-15 and abs(float(got[i]) - 9.999000099989999e-05) < SSIM_TOL
        if kind == 'identical':
            assert float(got[i]) == 1.0
    margins('box SSIM %s N %d C %d %d x %d crop %d: worst |device - fp64 uniform_filter form| %.2e (bound %.0e)' % (kind, n, c, h, w, crop, worst, SSIM_TOL))
    assert worst < SSIM_TOL


@pytest.mark.parametrize('n,c,h,w,crop', [(2, 3, 37, 53, 0), (2, 3, 37, 53, 5), (1, 1, 8, 300, 0), (1, 3, 600, 20, 3)])
def test_channel_sums_are_the_exact_integer_sums(n, c, h, w, crop):
    dev = _gpu()
    from dasr_amd import _lib
    L = _lib.lib()
    a, _ = _pair(7 + crop, n, c, h, w)
    ta = torch.from_numpy(a).to(dev)
    nbytes = L.dasr_img_ws_bytes(n, c, h, w, crop)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    out = torch.full((n * c,), -1, dtype=torch.int64, device=dev)
    _lib.check(L.dasr_img_channel_sums(ta.data_ptr(), n, c, h, w, crop, out.data_ptr(), ws.data_ptr(), nbytes, None), 'dasr_img_channel_sums')
    torch.cuda.synchronize()
    want = _crop(a, crop).astype(np.int64).sum((-1, -2)).reshape(-1)
    assert out.cpu().tolist() == want.tolist()


@pytest.mark.parametrize('h,w,border', [(40, 52, 0), (45, 61, 4)])
def test_pair_metrics_u8_against_the_double_formulas(h, w, border, margins):
    dev = _gpu()
    from dasr_amd import metrics
    r = np.random.RandomState(h + border)
    a = r.randint(30, 200, size=(3, h, w)).astype(np.uint8)
    b = (a.astype(np.int64) + r.randint(-20, 21, size=a.shape) + np.array([3, -2, 5]).reshape(3, 1, 1)).astype(np.uint8)   # channel means differ by >= 2 / 255
    m = metrics.pair_metrics_u8(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), border=border)
    ca, cb = _crop(a, border), _crop(b, border)
    d = ca.astype(np.int64) - cb.astype(np.int64)
    sse = int((d * d).sum())
    assert m['psnr'] == 10.0 * math.log10(255.0 ** 2 / (sse / ca.size))           # bit-equal: the sum is an exact integer
    hwc_a, hwc_b = ca.transpose(1, 2, 0), cb.transpose(1, 2, 0)                    # evaluate.py:45 on the HWC arrays
    va, vb = hwc_a.mean(1).mean(0) / 255., hwc_b.mean(1).mean(0) / 255.
    assert np.abs(va - vb).min() >= 1.0 / 255
    want_col = 10 * np.log10(1.0 / np.mean((va - vb) ** 2))
    want_ssim = box_ssim_ref(ca, cb)
    margins('pair_metrics_u8 %d x %d border %d: |psnr_col - numpy| %.2e dB (bound %.0e), |ssim - fp64 form| %.2e (bound %.0e)' % (
        h, w, border, abs(m['psnr_col'] - want_col), COL_TOL, abs(m['ssim'] - want_ssim), SSIM_TOL))
    assert abs(m['psnr_col'] - want_col) < COL_TOL and abs(m['ssim'] - want_ssim) < SSIM_TOL
    same = metrics.pair_metrics_u8(torch.from_numpy(a).to(dev), torch.from_numpy(a).to(dev), border=border)
    assert same['psnr'] == float('inf') and same['psnr_col'] == float('inf') and same['ssim'] == 1.0


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def to_blocked(x, dev):
    from dasr_amd.engine import BTensor
    N, Cc, H, W = x.shape
    b = BTensor(N, Cc, H, W, True, dev)
    xp = torch.zeros(N, b.planes * 16, H, W)
    xp[:, :Cc] = x
    b.t.copy_(xp.view(N, b.planes, 16, H, W).permute(0, 1, 3, 4, 2))
    return b


SC, SH = (2.1, 2.2, 2.3), (-1.0, -0.9, -0.8)


def _s2d_any(dev, x, entry='dasr_lpips_s2d_any'):
    from dasr_amd import _lib
    from dasr_amd.engine import BTensor
    from dasr_amd.lpips import s2d_grid
    n, _, H, W = x.shape
    sc, sh = (C.c_float * 4)(*SC, 0), (C.c_float * 4)(*SH, 0)
    y = BTensor(n, 48, s2d_grid(H), s2d_grid(W), True, dev)
    y.t.fill_(float('nan'))   # every slot of the three planes must be written
    args = (to_blocked(x, dev).view(), n, H, W, sc, sh, y.view()) + ((0, None) if entry == 'dasr_lpips_s2d' else (None,))
    _lib.check(getattr(_lib.lib(), entry)(*args), entry)
    torch.cuda.synchronize()
    return y.nchw().cpu()


@pytest.mark.parametrize('H,W', ODD_SIZES, ids=['%dx%d' % s for s in ODD_SIZES])
def test_s2d_any_is_the_padded_scaled_unfolded_image(H, W):
    dev = _gpu()
    from dasr_amd.lpips import s2d_grid
    n = 2
    x = torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(H * W)) + 0.5   # no zero inside the image: the zero pattern is the padding alone
    got = _s2d_any(dev, x)
    Hs, Ws = s2d_grid(H), s2d_grid(W)
    xs = x * torch.tensor(SC).view(1, 3, 1, 1) + torch.tensor(SH).view(1, 3, 1, 1)
    xp = F.pad(xs, (2, 4 * Ws - W - 2, 2, 4 * Hs - H - 2))   # zero padding of the SCALED image: 2 in front, what the grid needs behind
    want = xp.view(n, 3, Hs, 4, Ws, 4).permute(0, 1, 3, 5, 2, 4).reshape(n, 48, Hs, Ws)
    assert got.shape == want.shape and rel(got, want) < 1e-6
    assert torch.equal(got == 0, want == 0) and not torch.signbit(got[got == 0]).any()   # +0 bit for bit outside the image, on every side
    # and the 3 x 3 conv on this grid is the 11 x 11 / stride 4 / pad 2 conv of the image
    from dasr_amd.lpips import conv1_to_s2d
    w11 = torch.randn(4, 3, 11, 11, generator=torch.Generator().manual_seed(1))
    assert rel(F.conv2d(got, conv1_to_s2d(w11)), F.conv2d(xs, w11, stride=4, padding=2)) < 1e-5


def test_s2d_any_writes_the_bytes_of_s2d_at_multiples_of_4():
    dev = _gpu()
    x = torch.rand(2, 3, 32, 40, generator=torch.Generator().manual_seed(5))
    a, b = _s2d_any(dev, x), _s2d_any(dev, x, 'dasr_lpips_s2d')
    assert a.shape == b.shape == (2, 48, 9, 11) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _images(seed, n, H, W):
    """two batches of 8-bit images / 255, as the evaluator hands them to distance"""
    a, b = _pair(seed, n, 3, H, W)
    return torch.from_numpy(a).float() / 255.0, torch.from_numpy(b).float() / 255.0


@pytest.fixture(scope='module')
def lpips_pair(golden_dir):
    """(product network, oracle criterion) with the same weights: seeded AlexNet, the reference's linear heads from the golden fixture"""
    dev = _gpu()
    from oracle import lpips
    from dasr_amd.lpips import LPIPSAlexHIP
    crit, sd = lpips.golden_criterion(77, golden_dir)
    net = LPIPSAlexHIP(device=dev)
    net.load_state_dict(sd)
    return net, crit


@pytest.mark.parametrize('H,W', ODD_SIZES, ids=['%dx%d' % s for s in ODD_SIZES])
def test_distance_at_any_size_matches_the_oracle(H, W, lpips_pair, margins):
    dev = _gpu()
    net, crit = lpips_pair
    a, b = _images(H + W, 2, H, W)
    got = float(net.distance(a.to(dev), b.to(dev)))
    want = float(crit(a, b))
    margins('LPIPS distance %d x %d: rel err vs oracle %.2e (tol %.0e)' % (H, W, abs(got - want) / want, ACT_TOL))
    assert want > 0 and abs(got - want) < ACT_TOL * want


def test_distance_at_multiples_of_4_still_runs_the_old_entry_point(lpips_pair):
    """(32, 40): the recorded list holds dasr_lpips_s2d, not dasr_lpips_s2d_any, and the value has the bits of the same list built by hand around OP_LPIPS_S2D"""
    dev = _gpu()
    from dasr_amd import _lib
    from dasr_amd.engine import BTensor, OpList
    net, crit = lpips_pair
    n, H, W = 1, 32, 40
    a, b = _images(3, n, H, W)
    got = net.distance(a.to(dev), b.to(dev))
    kinds = [o.op for o in net._val_lru[('val', n, H, W)][0].ops]
    assert kinds.count(_lib.OP_LPIPS_S2D) == 1 and _lib.OP_LPIPS_S2D_ANY not in kinds
    p = net.plan(2 * n, n, H, W)
    assert not p.any_size and (p.x.H, p.x.W) == (H // 4 + 1, W // 4 + 1)
    img, acc = to_blocked(torch.cat([a, b]), dev), torch.zeros(1, device=dev)
    ops = OpList()
    ops.add(_lib.make_op(_lib.OP_LPIPS_S2D, x=img.view(), N=2 * n, H=H, W=W, y=p.x.view(), mode=0, scale4=p._sc, shift4=p._sh))
    ops.extend(p.fwd)
    for o in p.head_ops(acc.data_ptr(), 0.0):
        ops.add(o)
    ops.run()
    torch.cuda.synchronize()
    assert torch.equal(got.reshape(1).view(torch.int32).cpu(), acc.view(torch.int32).cpu())
    want = float(crit(a, b))
    assert abs(float(got) - want) < ACT_TOL * want
    # an odd size next to it takes the new op
    net.distance(a[..., :31, :39].to(dev), b[..., :31, :39].to(dev))
    kinds = [o.op for o in net._val_lru[('val', n, 31, 39)][0].ops]
    assert kinds.count(_lib.OP_LPIPS_S2D_ANY) == 1 and _lib.OP_LPIPS_S2D not in kinds


def test_distance_refuses_sizes_below_31(lpips_pair):
    dev = _gpu()
    net, _ = lpips_pair
    for H, W in ((30, 40), (40, 28), (30, 31)):
        x = torch.zeros(1, 3, H, W, device=dev)
        with pytest.raises(ValueError) as e:
            net.distance(x, x)
        assert '%d x %d' % (H, W) in str(e.value)


# ---- the CLI end to end ----------------------------------------------------------------------------------------------------------------------------------
CLI_BORDER = 4


def _write_folders(root):
    from PIL import Image
    res, gt = os.path.join(root, 'res'), os.path.join(root, 'gt')
    os.makedirs(res)
    os.makedirs(gt)
    arrays = []
    for i in range(3):
        r = np.random.RandomState(40 + i)
        g = r.randint(0, 256, size=(44, 56, 3)).astype(np.uint8)                                                   # RGB ground truth, larger
        a = np.clip(g[:40, :52].astype(np.int64) + r.randint(-20, 21, size=(40, 52, 3)), 0, 255).astype(np.uint8)
        rgba = np.concatenate([a, r.randint(0, 256, size=(40, 52, 1)).astype(np.uint8)], 2)                          # RGBA result
        Image.fromarray(rgba).save(os.path.join(res, 'img_%d.png' % i))
        Image.fromarray(g).save(os.path.join(gt, 'img_%d.png' % i))
        arrays.append((a, g))
    return res, gt, arrays


def _run_cli(res, gt, capsys):
    from dasr_amd import dsn_evaluate
    out = dsn_evaluate.main(['--dir', res, '--gt_dir', gt, '--border_crop', str(CLI_BORDER), '--allow_random_perceptual', '--num_workers', '2'])
    return out, capsys.readouterr().out


def _seeded_oracle():
    """the network --allow_random_perceptual seeds (lpips.load_lpips: lpips_random_state_dict(77)) as the oracle's criterion"""
    from oracle import lpips
    from dasr_amd.lpips import lpips_random_state_dict
    sd = lpips_random_state_dict(77)
    feats = lpips.alexnet_features()
    feats.load_state_dict({k[len('features.'):]: v for k, v in sd.items() if k.startswith('features.')})
    return lpips.PerceptualLossLPIPS(lpips.LPIPSAlex(feats, [sd['lin%d.model.1.weight' % i].reshape(-1) for i in range(5)]))


def test_cli_end_to_end_matches_the_host_restatement(tmp_path, capsys, margins):
    _gpu()
    res, gt, arrays = _write_folders(str(tmp_path))
    out, text = _run_cli(res, gt, capsys)
    crit = _seeded_oracle()
    c = CLI_BORDER
    want = {'psnr': [], 'psnr_col': [], 'ssim': [], 'lpips': []}
    for a, g in arrays:   # evaluate.py:35-52 in fp64 / on the oracle
        img, gti = a[c:-c, c:-c, :], g[:40, :52, :][c:-c, c:-c, :]
        d = img.astype(np.int64) - gti.astype(np.int64)
        want['psnr'].append(10.0 * math.log10(255.0 ** 2 / (int((d * d).sum()) / img.size)))   # the double formula on the exact sum: bit-equal
        va, vb = img.mean(1).mean(0) / 255., gti.mean(1).mean(0) / 255.
        want['psnr_col'].append(10 * np.log10(1.0 / np.mean((va - vb) ** 2)))
        want['ssim'].append(box_ssim_ref(img.transpose(2, 0, 1), gti.transpose(2, 0, 1)))
        ti, tg = (torch.from_numpy(np.ascontiguousarray(v)).permute(2, 0, 1)[None].float() / 255. for v in (img, gti))
        want['lpips'].append(float(crit(ti, tg)))
    assert out['lpips_label'] == 'LPIPS(random)' and len(out['files']) == 3
    assert [os.path.basename(r['file']) for r in out['files']] == ['img_0.png', 'img_1.png', 'img_2.png']
    assert [r['psnr'] for r in out['files']] == want['psnr'] and out['psnr'] == sum(want['psnr']) / 3
    tol = {'psnr_col': COL_TOL, 'ssim': SSIM_TOL}
    for k in ('psnr_col', 'ssim', 'lpips'):
        errs = [abs(r[k] - w) / (abs(w) if k == 'lpips' else 1.0) for r, w in zip(out['files'], want[k])]
        avg_err = abs(out[k] - float(np.mean(want[k]))) / (abs(float(np.mean(want[k]))) if k == 'lpips' else 1.0)
        margins('dsn_evaluate %s: worst per-file error %.2e, of the average %.2e (bound %.0e%s)' % (k, max(errs), avg_err, tol.get(k, ACT_TOL),
                                                                                                    ' relative' if k == 'lpips' else ''))
        assert max(errs) < tol.get(k, ACT_TOL) and avg_err < tol.get(k, ACT_TOL), k
    lines = text.splitlines()
    assert lines[-4:] == ['PSNR: ' + str(out['psnr']), 'PSNR_col: ' + str(out['psnr_col']), 'SSIM: ' + str(out['ssim']), 'LPIPS(random): ' + str(out['lpips'])]
    for r in out['files']:
        assert any(l.startswith(os.path.basename(r['file']) + ':') and str(r['ssim']) in l and 'LPIPS(random) ' + str(r['lpips']) in l for l in lines)
    assert not any('WARNING' in l for l in lines)


def test_box_ssim_and_cli_are_deterministic(tmp_path, capsys):
    dev = _gpu()
    a, b = _pair(9, 2, 3, 64, 96)
    r1, r2 = _device_box_ssim(dev, a, b, 0), _device_box_ssim(dev, a, b, 0)
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64))
    res, gt, _ = _write_folders(str(tmp_path))
    (o1, t1), (o2, t2) = _run_cli(res, gt, capsys), _run_cli(res, gt, capsys)
    assert t1 == t2 and o1 == o2
