"""Host side of the iterative back-projection (dasr_amd/backproject.py, dasr_amd/back_projection.py, csrc/imgio.hip; reference:
codes/SRN/scripts/back_projection/backprojection.m, main_bp.m): the entry points in header, binding and library; the up-sampling direction of
data.imresize_matlab against the reference's imresize_np; the separable form of the 5 x 5 kernel; the contraction of the fp64 restatement; the option values;
the pairing errors of the CLI.  No device."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('dasr_bp_residual', 'dasr_bp_update')


def test_entry_points_in_header_binding_and_library():
    from dasr_amd import _lib, backproject
    header = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    for name in ENTRY_POINTS:
        assert re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert name in _lib._SIGS and len(_lib._SIGS[name]) == 12, name
    assert re.search(r'^#define DASR_ABI_VERSION 22$', header, flags=re.M) and _lib.ABI_VERSION == 22
    # the tile sizes the GPU tests take their shapes from are the kernels'
    tiles = {k: int(v) for k, v in re.findall(r'^#define DASR_BP_(\w+) (\d+)$', header, flags=re.M)}
    assert (tiles['RES_TILE_H'], tiles['RES_TILE_W']) == backproject.RES_TILE and (tiles['UPD_TILE_H'], tiles['UPD_TILE_W']) == backproject.UPD_TILE
    from dasr_amd import build
    assert os.path.exists(build.build())
    L = _lib.lib()   # (binds every name of _SIGS: no device is touched)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    assert L.dasr_abi_version() == 22
    data = open(_lib.LIB_PATH, 'rb').read()
    assert b'bp_residual_kernel' in data and b'bp_update_kernel' in data


def test_upsampling_matches_the_reference(golden_dir):
    """data.imresize_matlab(x, s), s = 2, 3, 4 (float64 taps and sums) against the reference's imresize_np(x, s, True) (tests/golden/imresize_up.npz, written by
    scripts/gen_golden_imresize_up.py).  Bound 1e-6.  Measured on this fixture: at most 2.1e-7 at s = 2 and 4, 9.3e-7 at s = 3 -- the reference forms its weights and sums
    in float32 (torch.FloatTensor), where the sample offsets k / 3 are not exact; the fixture stores float32."""
    from dasr_amd.data import imresize_matlab
    z = np.load(os.path.join(golden_dir, 'imresize_up.npz'))
    n = len([k for k in z.files if k.startswith('in')])
    assert n >= 8
    seen, worst = set(), 0.0
    for i in range(n):
        x, s = torch.from_numpy(z['in%d' % i]).permute(2, 0, 1).double(), int(z['scale%d' % i])
        want = z['out%d' % i].astype(np.float64)
        got = imresize_matlab(x, float(s)).permute(1, 2, 0).numpy()
        assert got.shape == want.shape == (s * x.shape[1], s * x.shape[2], 3)
        err = float(np.abs(got - want).max())
        print('imresize up %s x%d: %.2e' % (tuple(x.shape[1:]), s, err))
        worst = max(worst, err)
        seen.add((s, tuple(x.shape[1:])))
    assert {s for s, _ in seen} == {2, 3, 4} and {(1, 3), (2, 2)} <= {hw for _, hw in seen}
    assert worst < 1e-6, worst


def test_kernel_is_separable():
    """p of backprojection.m:6-8 (fspecial('gaussian', 5, 1) squared and renormalised) = outer(u, u) with u_i = exp(-i^2) / sum_j exp(-j^2)"""
    from dasr_amd.backproject import gaussian_p, gaussian_u5
    u = torch.tensor(gaussian_u5(), dtype=torch.float64)
    p = gaussian_p()
    # MATLAB's fspecial written out independently of gaussian_p
    yy, xx = np.mgrid[-2:3, -2:3].astype(np.float64)
    h = np.exp(-(xx * xx + yy * yy) / (2.0 * 1.0 ** 2))
    h[h < np.finfo(np.float64).eps * h.max()] = 0
    h /= h.sum()
    q = h ** 2
    q /= q.sum()
    assert abs(float(u.sum()) - 1.0) < 1e-15 and tuple(p.shape) == (5, 5)
    assert float(np.abs(p.numpy() - q).max()) < 1e-15
    assert float((torch.outer(u, u) - p).abs().max()) < 1e-15


@pytest.mark.parametrize('s,hw', [(4, (48, 64)), (2, (12, 18)), (3, (12, 18))], ids=['x4_48x64', 'x2_12x18', 'x3_12x18'])
def test_restatement_contracts(s, hw):
    """max|lr - down(sr_k)| of back_project_fp64 does not increase over 20 iterations"""
    from dasr_amd.backproject import back_project_fp64
    from dasr_amd.data import imresize_matlab
    g = torch.Generator().manual_seed(100 * s + hw[0])
    hr = torch.rand((1, 3) + hw, generator=g, dtype=torch.float64)
    lr = imresize_matlab(hr[0], 1.0 / s)[None]
    sr = hr + 0.05 * torch.randn(hr.shape, generator=g, dtype=torch.float64)
    sr0, lr0, trace = sr.clone(), lr.clone(), []
    out = back_project_fp64(sr, lr, 20, trace)
    assert out.dtype == torch.float64 and out.shape == sr.shape
    assert torch.equal(sr, sr0) and torch.equal(lr, lr0)
    assert len(trace) == 21 and all(b <= a for a, b in zip(trace, trace[1:])), trace
    assert trace[-1] < 0.1 * trace[0], trace
    assert torch.equal(back_project_fp64(sr, lr, 0), sr)


def test_option_values(tmp_path):
    import json
    from dasr_amd import options
    it = options.back_projection_iters
    assert it(True) == 20 and it(7) == 7
    assert it(None) == 0 and it(False) == 0 and it(0) == 0
    for bad in (-1, 1.5, 'x'):
        with pytest.raises(ValueError, match='back_projection'):
            it(bad)
    # the check is part of options.parse: a bad value stops the run before a model is built; a good one is left in the file's own form
    base = {'name': 'bp', 'model': 'sr', 'scale': 4, 'gpu_ids': [0], 'datasets': {}, 'path': {'root': str(tmp_path)}, 'network_G': {'which_model_G': 'RRDB_net'}}
    def parse(**extra):
        p = tmp_path / 'o.json'
        p.write_text(json.dumps(dict(base, **extra)))
        return options.parse(str(p), is_train=False)
    assert 'back_projection' not in parse()
    assert parse(back_projection=True)['back_projection'] is True and parse(back_projection=3)['back_projection'] == 3
    for bad in (-1, 1.5, 'x'):
        with pytest.raises(ValueError, match='back_projection'):
            parse(back_projection=bad)


def test_scale_of_names_the_shapes():
    from dasr_amd.backproject import scale_of
    assert scale_of((1, 3, 48, 64), (1, 3, 12, 16)) == 4 and scale_of((1, 1, 6, 4), (1, 1, 3, 2)) == 2 and scale_of((1, 3, 3, 9), (1, 3, 1, 3)) == 3
    for sr, lr in (((2, 3, 8, 8), (2, 3, 2, 2)), ((1, 3, 8, 8), (1, 1, 2, 2)), ((1, 3, 8, 12), (1, 3, 2, 4)), ((1, 3, 10, 10), (1, 3, 2, 2)), ((1, 3, 9, 8), (1, 3, 2, 2)),
                   ((1, 3, 2, 2), (1, 3, 2, 2))):
        with pytest.raises(ValueError) as e:
            scale_of(sr, lr)
        assert str(sr) in str(e.value) and str(lr) in str(e.value)


def test_cli_pairing_errors(tmp_path):
    from PIL import Image
    from dasr_amd import back_projection as cli
    lr_dir, sr_dir = tmp_path / 'LR', tmp_path / 'SR'
    lr_dir.mkdir()
    sr_dir.mkdir()
    g = np.random.RandomState(0)
    save = lambda p, h, w: Image.fromarray(g.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(str(p))
    save(sr_dir / 'a.png', 48, 64)
    save(lr_dir / 'a.png', 12, 16)
    save(sr_dir / 'b.png', 48, 64)
    with pytest.raises(ValueError) as e:   # no partner
        cli.list_pairs(str(sr_dir), str(lr_dir))
    assert str(sr_dir / 'b.png') in str(e.value) and str(lr_dir / 'b.png') in str(e.value)
    save(lr_dir / 'b.png', 12, 17)
    with pytest.raises(ValueError) as e:   # not s x the LR size
        cli.list_pairs(str(sr_dir), str(lr_dir))
    assert str(sr_dir / 'b.png') in str(e.value) and str(lr_dir / 'b.png') in str(e.value)
    with pytest.raises(ValueError) as e:   # the same through main(): raised before a device is looked for
        cli.main(['--lr_dir', str(lr_dir), '--sr_dir', str(sr_dir), '--out_dir', str(tmp_path / 'out')])
    assert str(sr_dir / 'b.png') in str(e.value) and str(lr_dir / 'b.png') in str(e.value)
    assert not (tmp_path / 'out').exists()
    save(lr_dir / 'b.png', 24, 32)
    assert cli.list_pairs(str(sr_dir), str(lr_dir)) == [(str(sr_dir / 'a.png'), str(lr_dir / 'a.png'), 4), (str(sr_dir / 'b.png'), str(lr_dir / 'b.png'), 2)]
