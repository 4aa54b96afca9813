"""CPU: the host parts of the x8 self-ensemble (`"self_ensemble": true`, BaseModel.test_x8): the two entry points of csrc/imgio.hip, the index table of
dasr_amd/util.py against a literal restatement of the reference's loops (codes/SRN/models/SR_model.py:102-140), the argument checks in front of the first HIP call
and the refusal of a batch above 1."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def test_symbols_are_declared_bound_and_exported_and_the_abi_number_stays():
    from dasr_amd import build, _lib
    hdr = open(os.path.join(ROOT, 'include', 'dasr_hip.h')).read()
    declared = set(re.findall(r'^\s*int\s+(dasr_\w+)\s*\(', hdr, flags=re.M))
    build.build()
    L = _lib.lib()
    for name in ('dasr_dihedral8', 'dasr_dihedral8_mean'):
        assert name in declared and name in _lib._SIGS and hasattr(L, name), name
    assert _lib.ABI_VERSION == 22 and '#define DASR_ABI_VERSION 22' in hdr and L.dasr_abi_version() == 22


def _reference_loops(x, net):
    """SR_model.py:102-140 restated literally on numpy: lr_list grows by 'v', 'h', 't'; `net` stands for netG; the inverse by i > 3 / i % 4 > 1 / i % 2 == 1.
    Returns (the eight transformed inputs, the eight inverse-transformed outputs)."""
    def _transform(v, op):
        if op == 'v':
            return v[:, :, :, ::-1].copy()
        if op == 'h':
            return v[:, :, ::-1, :].copy()
        return v.transpose((0, 1, 3, 2)).copy()
    lr_list = [x]
    for tf in 'v', 'h', 't':
        lr_list.extend([_transform(t, tf) for t in lr_list])
    sr_list = [net(aug) for aug in lr_list]
    for i in range(len(sr_list)):
        if i > 3:
            sr_list[i] = _transform(sr_list[i], 't')
        if i % 4 > 1:
            sr_list[i] = _transform(sr_list[i], 'h')
        if (i % 4) % 2 == 1:
            sr_list[i] = _transform(sr_list[i], 'v')
    return lr_list, sr_list


@pytest.mark.parametrize('hw', [(1, 1), (5, 3), (37, 70)], ids=lambda s: '%dx%d' % s)
def test_index_table_equals_the_reference_loops(hw):
    from dasr_amd import util
    H, W = hw
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W))
    # a stand-in generator that is NOT equivariant (every sample is weighted by its position), so that a wrong inverse cannot cancel
    net = lambda a: a * (1.0 + np.arange(a.shape[2] * a.shape[3], dtype=np.float32).reshape(1, 1, a.shape[2], a.shape[3]))
    lr_ref, sr_ref = _reference_loops(x.numpy(), net)
    members = util.dihedral8_reference(x)
    assert len(members) == 8
    for i in range(8):
        assert tuple(members[i].shape) == lr_ref[i].shape and np.array_equal(members[i].numpy(), lr_ref[i]), i
    # the inverse, member by member: all members but i zeroed, the mean times 8 is member i's inverse-transformed output
    srs = [torch.from_numpy(net(m.numpy())) for m in members]
    for i in range(8):
        only = [s if k == i else torch.zeros_like(s) for k, s in enumerate(srs)]
        assert np.array_equal((util.dihedral8_mean_reference(only) * 8).numpy(), sr_ref[i]), i
    # and the sum: sequential in fp32, within the last bits of the reference's torch.cat(...).mean(dim=0) (which has no defined order)
    got = util.dihedral8_mean_reference(srs)
    seq = sr_ref[0].copy()
    for s in sr_ref[1:]:
        seq = seq + s
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), seq * np.float32(0.125))
    want = torch.cat([torch.from_numpy(s) for s in sr_ref], 0).double().mean(dim=0, keepdim=True)
    bound = 7 * 2.0 ** -24 * torch.stack([torch.from_numpy(s).double().abs() for s in sr_ref]).mean(0)
    assert bool(((got.double() - want).abs() <= bound).all())


def test_entry_points_reject_bad_arguments_before_any_launch():
    """every DASR_EINVAL clause, in front of the first HIP call (the non-null pointers stand for device addresses and are never dereferenced)"""
    from dasr_amd import _lib
    L = _lib.lib()
    x, a, b = 0x1000, 0x2000, 0x3000
    assert L.dasr_dihedral8(None, 3, 4, 4, a, b, None) == EINVAL
    assert L.dasr_dihedral8(x, 3, 4, 4, None, b, None) == EINVAL
    assert L.dasr_dihedral8(x, 3, 4, 4, a, None, None) == EINVAL
    for chw in ((0, 4, 4), (3, 0, 4), (3, 4, 0), (-1, 4, 4), (3, -4, 4), (3, 4, -4), (65536, 4, 4)):
        assert L.dasr_dihedral8(x, *chw, a, b, None) == EINVAL, chw
        assert L.dasr_dihedral8_mean(x, a, *chw, b, None) == EINVAL, chw
    assert L.dasr_dihedral8(x, 3, 4, 4, x, b, None) == EINVAL
    assert L.dasr_dihedral8(x, 3, 4, 4, a, x, None) == EINVAL
    assert L.dasr_dihedral8(x, 3, 4, 4, a, a, None) == EINVAL
    assert L.dasr_dihedral8_mean(None, a, 3, 4, 4, b, None) == EINVAL
    assert L.dasr_dihedral8_mean(x, None, 3, 4, 4, b, None) == EINVAL
    assert L.dasr_dihedral8_mean(x, a, 3, 4, 4, None, None) == EINVAL
    assert L.dasr_dihedral8_mean(x, a, 3, 4, 4, x, None) == EINVAL
    assert L.dasr_dihedral8_mean(x, a, 3, 4, 4, a, None) == EINVAL


@pytest.mark.parametrize('cls', ['SRModel', 'DASR_Model'])
def test_test_x8_refuses_a_batch_above_one(cls):
    """the reference's mean(dim=0) over the concatenated list would average different images into one: ValueError, in front of any device work (the
    generator is a stand-in that must not be reached)"""
    from dasr_amd import models, dasr_model, options
    klass = getattr(models, cls, None) or getattr(dasr_model, cls)
    m = klass.__new__(klass)
    m.opt = options.dict_to_nonedict({'scale': 4, 'chop': False, 'val_lpips': False})

    class _NetG:
        def forward(self, x):
            raise AssertionError('the generator must not run on a refused batch')
    m.netG = _NetG()
    m.var_L = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match='batch of 1'):
        m.test_x8()

