"""CPU: bench.py --dump-outputs writes every output of the timed step as float32 / float64 .npy files, 64 MB at most in all, and samples an
oversized array at the same positions on every run."""
import os
import types

import numpy as np
import torch

import bench


def _model(n_weights):
    net = types.SimpleNamespace(params=types.SimpleNamespace(flat=torch.arange(n_weights, dtype=torch.float32)))
    return types.SimpleNamespace(netG=net, netD_target=None, get_current_log=lambda: {'loss/l_g_pix': 0.25, 'l_pix': 1.5})


def test_dump_outputs_names_dtypes_and_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 1 << 20)   # a small budget exercises the sampling of the weights without a 64 MB array
    images = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(5))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), _model(1 << 20), images)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['images.npy', 'log_l_pix.npy', 'log_loss_l_g_pix.npy', 'weights_netG.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / n) for n in names) <= bench.DUMP_BYTES
    out = {n: np.load(tmp_path / 'a' / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert np.array_equal(out['images.npy'], images.numpy())                   # under its share: written whole, shape kept
    assert out['log_l_pix.npy'].dtype == np.float64 and out['log_l_pix.npy'][0] == 1.5
    w = out['weights_netG.npy']                                                # over its share: a sorted sample of distinct positions
    assert 0 < w.size < 1 << 20 and np.all(np.diff(w) > 0)
    for n in names:                                                            # the same positions on every run
        assert np.array_equal(out[n], np.load(tmp_path / 'b' / n))
