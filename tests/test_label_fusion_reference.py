"""CPU: multi-atlas label fusion, everything that needs no GPU -- the two C entries exist in the header and the library and refuse bad
arguments before touching a device; the oracles of tests/fusion_cases.py are self-consistent; and on exactly the inputs of
test_gpu_label_fusion.py the exclusion rule leaves out less than its cap, so a GPU test cannot hide a failure behind its mask."""
import os

import numpy as np
import pytest
import torch

import fusion_cases as fc
import regeval_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fusion_entries_are_declared_and_built():
    import __graft_entry__ as ge
    ge.build()
    from deepatlas_amd import _native
    L = _native.lib()
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    for name in ('da_label_fusion_vote', 'da_local_msd_weights', 'da_local_msd_weights_ws_bytes'):
        assert name + '(' in header, name
        assert name in _native.SIGNATURES and hasattr(L, name), name
    blob = open(ge.LIB, 'rb').read()
    assert b'label_fusion_vote_kernel' in blob and b'msd_axis_kernel' in blob


def test_fusion_c_abi_rejects_bad_arguments_before_touching_the_device():
    from ctypes import c_void_p
    from deepatlas_amd import _native
    L = _native.lib()
    fake = c_void_p(0x1000)          # never dereferenced on the host
    BAD, SMALL, UNSUPPORTED = -1, -2, -3
    vote = L.da_label_fusion_vote
    assert vote(fake, 1, 0, fake, None, None, 1, 0, 8, 8, 8, fake, None, None) == BAD               # K = 0
    assert vote(fake, 1, 0, fake, None, None, 1, 33, 8, 8, 8, fake, None, None) == UNSUPPORTED      # K = 33
    assert vote(fake, 1, 0, None, None, None, 1, 3, 8, 8, 8, fake, None, None) == BAD               # null fields
    assert vote(None, 1, 0, fake, None, None, 1, 3, 8, 8, 8, fake, None, None) == BAD               # null atlas maps
    assert vote(fake, 1, 0, fake, None, None, 1, 3, 8, 8, 8, None, fake, None) == BAD               # null output
    assert vote(fake, 1, 0, fake, fake, fake, 1, 3, 8, 8, 8, fake, None, None) == BAD               # both weight forms at once
    assert vote(fake, 4, 0, fake, None, None, 1, 3, 8, 8, 8, fake, None, None) == BAD               # label_bytes 4
    assert vote(fake, 1, 100, fake, None, None, 2, 3, 8, 8, 8, fake, None, None) == BAD             # per-target blocks that overlap
    assert vote(fake, 1, 0, fake, None, None, 1, 3, 1024, 1024, 1024, fake, None, None) == UNSUPPORTED      # 2^30 voxels
    for dims in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0)):
        assert vote(fake, 1, 0, fake, None, None, dims[0], 3, dims[1], dims[2], dims[3], fake, None, None) == BAD
    msd = L.da_local_msd_weights
    need = L.da_local_msd_weights_ws_bytes(2, 3, 8, 8, 8)
    assert need >= 2 * 3 * 512 * 4
    assert msd(fake, fake, 2, 3, 8, 8, 8, 0, 1.0, fake, fake, need, None) == BAD                    # r = 0
    assert msd(fake, fake, 2, 3, 8, 8, 8, 5, 1.0, fake, fake, need, None) == BAD                    # r = 5
    assert msd(None, fake, 2, 3, 8, 8, 8, 2, 1.0, fake, fake, need, None) == BAD                    # null warped images
    assert msd(fake, None, 2, 3, 8, 8, 8, 2, 1.0, fake, fake, need, None) == BAD                    # null target
    assert msd(fake, fake, 2, 3, 8, 8, 8, 2, 1.0, None, fake, need, None) == BAD                    # null output
    assert msd(fake, fake, 2, 3, 8, 8, 8, 2, -1.0, fake, fake, need, None) == BAD                   # beta < 0
    assert msd(fake, fake, 2, 0, 8, 8, 8, 2, 1.0, fake, fake, need, None) == BAD                    # K = 0
    assert msd(fake, fake, 2, 3, 8, 8, 8, 2, 1.0, fake, fake, need - 1, None) == SMALL


def test_fusion_ops_fail_loudly_on_cpu_tensors_and_wrong_shapes():
    from deepatlas_amd import ops, _native
    lab = torch.zeros((3, 4, 4, 4), dtype=torch.uint8)
    disp = torch.zeros((3, 3, 4, 4, 4))
    with pytest.raises(_native.NativeError):
        ops.label_fusion(lab, disp)
    with pytest.raises(_native.NativeError):
        ops.local_msd_weights(torch.zeros((1, 3, 4, 4, 4)), torch.zeros((1, 4, 4, 4)))


def test_train_scripts_take_the_atlas_fusion_flag():
    import argparse
    import train_joint
    import train_reg
    base = dict(device='0', debug=False, num_samples=4, num_epochs=3, lr=1e-3, test_only=False, data_root='./data', log_root='./logs', shape=[16, 16, 32])
    for mod in (train_reg, train_joint):
        assert 'atlas_fusion' not in mod.build_config(argparse.Namespace(**base))
        assert 'atlas_fusion' not in mod.build_config(argparse.Namespace(atlas_fusion=None, **base))
        c = mod.build_config(argparse.Namespace(atlas_fusion='local', **base))
        assert c['atlas_fusion'] == 'local'
    args = train_reg.add_common_arguments(argparse.ArgumentParser()).parse_args(['--atlas-fusion', 'majority'])
    assert args.atlas_fusion == 'majority'
    assert train_reg.add_common_arguments(argparse.ArgumentParser()).parse_args([]).atlas_fusion is None
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    from deepatlas_amd.models.registration import RegistrationExperiment
    c0 = train_joint.build_config(argparse.Namespace(**base))
    c1 = train_joint.build_config(argparse.Namespace(atlas_fusion='majority', **base))
    assert DeepAtlasExperiment.experiment_name(c0) == DeepAtlasExperiment.experiment_name(c1)       # the key does not enter the name
    r0 = train_reg.build_config(argparse.Namespace(**base))
    r1 = train_reg.build_config(argparse.Namespace(atlas_fusion='local', **base))
    assert RegistrationExperiment.experiment_name(r0) == RegistrationExperiment.experiment_name(r1)
    with pytest.raises(ValueError):
        RegistrationExperiment(dict(r0, atlas_fusion='median'))


# ---- the oracles of fusion_cases.py are self-consistent -----------------------------------------------------------------------------
def test_vote_oracle_on_hand_made_votes():
    shape = (2, 2, 3)
    zero = torch.zeros((4, 3) + shape)
    lab = torch.zeros((4,) + shape, dtype=torch.int64)
    lab[:, 0, 0, 0] = torch.tensor([5, 3, 5, 3])              # 2 : 2 tie -> the smaller label
    lab[:, 0, 0, 1] = torch.tensor([7, 7, 2, 7])              # majority
    lab[:, 0, 0, 2] = torch.tensor([1, 2, 3, 4])              # four-way tie -> 1
    o = fc.vote_oracle(lab, zero, 1, 4)
    assert not bool(o['excluded'].any())
    assert o['fused'][0, 0, 0].tolist() == [3, 7, 1] and o['conf'][0, 0, 0].tolist() == [0.5, 0.75, 0.25]
    assert o['gap'][0, 0, 0].tolist() == [0.0, 0.5, 0.0]
    w = torch.tensor([[0.0, 1.0, 0.5, 0.25]])
    o = fc.vote_oracle(lab, zero, 1, 4, w)
    assert o['fused'][0, 0, 0].tolist() == [3, 7, 2] and o['conf'][0, 0, 0].tolist() == [1.25 / 1.75, 1.25 / 1.75, 1.0 / 1.75]
    o = fc.vote_oracle(lab, zero, 1, 4, torch.zeros((1, 4)))
    assert int(o['fused'].max()) == 0 and float(o['conf'].max()) == 0.0
    # two targets sharing the atlas maps: the batch is N x K with the atlas index fastest
    o2 = fc.vote_oracle(lab[:2], torch.zeros((4, 3) + shape), 2, 2)
    assert torch.equal(o2['fused'][0], o2['fused'][1]) and o2['fused'][0, 0, 0].tolist() == [3, 7, 1]


def test_exact_weights_sum_exactly_in_fp32():
    w = fc.exact_weights((5, 32), seed=1)
    assert float(w.min()) >= 0.0 and float(w.max()) <= 4.0 and torch.equal(w * 64, (w * 64).round())
    s32 = torch.zeros(5)
    for k in range(32):
        s32 = s32 + w[:, k]
    assert torch.equal(s32.double(), w.double().sum(1))


@pytest.mark.parametrize('case', fc.VOTE_CASES, ids=fc.VOTE_IDS)
def test_gpu_vote_inputs_are_conditioned_as_the_exclusion_rule_assumes(case):
    """On the very inputs test_gpu_label_fusion.py uses: the share of voxels where some atlas is within 1e-4 voxels of a rounding
    boundary stays under K x 1e-3; torch's own fp32 grid_sample vote differs from the fp64 vote only inside that band; and the
    unweighted vote has exact ties for the top count on a large share of the voxels whenever K > 1, so the tie rule is exercised."""
    shape, n, k, sigma, per, dtype, kind = case
    labels, disp = fc.vote_inputs(case)
    o = fc.vote_oracle(labels, disp, n, k)
    share = float(o['excluded'].double().mean())
    ties = float((o['gap'] == 0).double().mean())
    print('K = %d: excluded share %.3e (cap %.1e), exact ties for the top count on %.1f %% of the voxels' % (k, share, k * fc.MAX_EXCLUDED_PER_ATLAS, 100 * ties))
    assert share <= k * fc.MAX_EXCLUDED_PER_ATLAS
    if k > 1 and kind == 'blocky':
        assert ties > 0.02
    full = labels.repeat(n, 1, 1, 1) if (labels.shape[0] == k and n > 1) else labels
    w32, _ = rc.nearest_oracle(full, disp, dtype=torch.float32)
    w32 = (w32 % 256).view((n, k) + tuple(shape))
    scores = torch.zeros((n, o['warped'].max().item() + 2) + tuple(shape), dtype=torch.float64)
    for a in range(k):
        scores.scatter_add_(1, w32[:, a:a + 1], torch.ones((n, 1) + tuple(shape), dtype=torch.float64))
    differ = scores.argmax(1) != o['fused']
    print('fp32 grid_sample vote differs on %d voxels' % int(differ.sum()))
    assert not bool((differ & ~o['excluded']).any())


@pytest.mark.parametrize('case', fc.LOCAL_CASES, ids=fc.LOCAL_IDS)
def test_near_ties_of_a_smoothly_weighted_vote_are_rare(case):
    """The locally weighted vote leaves out voxels whose float64 top-two scores are within 1e-5 of the total: with smooth positive
    weights (exp of a smooth field here) that share stays far below its 1e-3 cap."""
    shape, n, k, sigma, per, dtype, kind = case
    labels, disp = fc.vote_inputs(case)
    g = torch.Generator().manual_seed(9)
    w = torch.exp(-torch.rand((n, k) + tuple(shape), generator=g, dtype=torch.float64) * 3.0).float()
    o = fc.vote_oracle(labels, disp, n, k, w)
    share = float((o['gap'] < fc.NEAR_TIE).double().mean())
    print('near-tie share %.3e' % share)
    assert share <= fc.MAX_NEAR_TIE


@pytest.mark.parametrize('case', fc.MSD_CASES, ids=fc.MSD_IDS)
def test_msd_weight_yardstick_is_small_and_not_zero(case):
    shape, n, k, r, sigma = case
    warped, target = fc.msd_inputs(case)
    w64, bound, yard = fc.msd_bound(warped, target, r, sigma)
    print('r = %d sigma = %g: weights in [%.3g, %.3g], fp32 numpy yardstick %.3e' % (r, sigma, w64.min(), w64.max(), yard))
    assert w64.shape == (n, k) + tuple(shape)
    assert 0.0 < yard < 1e-5 and bound == 4 * yard
    assert w64.max() <= 1.0 and w64.min() >= 0.0 and w64.max() - w64.min() > 0.01          # the weights really differ


def test_msd_oracle_closed_forms():
    shape = (9, 10, 11)
    t = torch.rand((1,) + shape, dtype=torch.float64)
    # equal images: exactly 1
    assert np.all(fc.msd_weights_np(t[:, None].repeat(1, 2, 1, 1, 1), t, 2, 0.1) == 1.0)
    # a constant difference c: m = c^2 at interior voxels, c^2 x (the share of the window inside the volume) elsewhere
    c, r, sigma = 0.25, 2, 0.2
    w = fc.msd_weights_np((t + c)[:, None], t, r, sigma)
    want = np.exp(-c * c / (2 * sigma * sigma))
    assert np.abs(w[0, 0, r:-r, r:-r, r:-r] - want).max() < 1e-12
    corner = np.exp(-c * c * (3.0 / 5.0) ** 3 / (2 * sigma * sigma))
    assert abs(w[0, 0, 0, 0, 0] - corner) < 1e-12
    # a direct triple loop at a few voxels
    rng = np.random.default_rng(0)
    a = rng.random((1, 1) + (4, 5, 6)); b = rng.random((1,) + (4, 5, 6))
    w = fc.msd_weights_np(a, b, 1, 0.1)
    for (z, y, x) in ((0, 0, 0), (2, 3, 4), (3, 4, 5), (1, 0, 5)):
        s = 0.0
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    zz, yy, xx = z + dz, y + dy, x + dx
                    if 0 <= zz < 4 and 0 <= yy < 5 and 0 <= xx < 6:
                        s += (a[0, 0, zz, yy, xx] - b[0, zz, yy, xx]) ** 2
        assert abs(w[0, 0, z, y, x] - np.exp(-s / 27.0 / (2 * 0.01))) < 1e-12
