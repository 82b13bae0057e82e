"""GPU: multi-atlas label fusion (csrc/regeval.hip da_label_fusion_vote / da_local_msd_weights, ops.label_fusion /
ops.local_msd_weights, lib/evalMetrics.py atlas_segmentation, the experiments' atlas_fusion key) against oracles that are not the code
under test (tests/fusion_cases.py: torch-CPU grid_sample in float64 + a float64 vote; numpy window sums), plus constructed cases with
exact answers, device-versus-device identities and determinism.

Measured on an MI355X (printed by the tests): the vote equals the float64 oracle on every voxel outside the exclusion band in every case
(excluded share 4.5e-4 at K = 1 to 1.9e-2 at K = 32, always under K x 1e-3); conf is within 6e-8 relative with exactly summable weights.
local_msd_weights: the fp32 numpy yardstick is 0.78 - 1.56e-7 and the device error 0.33 - 0.73 of the yardstick (bound: 4 x).  Locally
weighted vote: near-tie share 0 - 3.7e-5 (cap 1e-3), no mismatch outside the excluded voxels."""
import argparse
import functools

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import fusion_cases as fc
import regeval_cases as rc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CONF_REL = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def _case(i):
    """(labels, disp, unweighted oracle) of VOTE_CASES[i]: computed once, shared, never modified."""
    labels, disp = fc.vote_inputs(fc.VOTE_CASES[i])
    _, n, k = fc.VOTE_CASES[i][:3]
    return labels, disp, fc.vote_oracle(labels, disp, n, k)


def _index(case):
    return fc.VOTE_CASES.index(case)


def _check_vote(got, conf, oracle, k, tag, extra_excluded=None, cap_extra=None):
    """fused equal outside the excluded voxels, the excluded share under its cap, conf within 2^-22 relative of the float64 value there."""
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(oracle['fused'].shape)
    got = got.cpu().to(torch.int64)
    excluded = oracle['excluded']
    share = float(excluded.double().mean())
    assert share <= k * fc.MAX_EXCLUDED_PER_ATLAS
    if extra_excluded is not None:
        extra = float((extra_excluded & ~excluded).double().mean())
        assert extra <= cap_extra
        excluded = excluded | extra_excluded
    else:
        extra = 0.0
    wrong = (got != oracle['fused']) & ~excluded
    msg = '%s: excluded share %.3e (cap %.1e), near-tie share %.3e, mismatches inside %d, outside %d' % (
        tag, share, k * fc.MAX_EXCLUDED_PER_ATLAS, extra, int(((got != oracle['fused']) & excluded).sum()), int(wrong.sum()))
    if conf is not None:
        assert conf.dtype == torch.float32 and tuple(conf.shape) == tuple(got.shape)
        c = conf.cpu().double()
        err = ((c - oracle['conf']).abs() / oracle['conf'].clamp_min(1e-300))[~excluded & (oracle['conf'] > 0)]
        zero_ok = bool((c[~excluded & (oracle['conf'] == 0)] == 0).all())
        msg += ', conf max relative error %.3e' % (float(err.max()) if err.numel() else 0.0)
        print(msg)
        assert zero_ok and (err.numel() == 0 or float(err.max()) <= CONF_REL)
    else:
        print(msg)
    assert not bool(wrong.any())


# ---- majority vote -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fc.VOTE_CASES, ids=fc.VOTE_IDS)
def test_majority_vote_matches_the_fp64_oracle_per_voxel(case):
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics as metrics
    shape, n, k = case[:3]
    labels, disp, oracle = _case(_index(case))
    lab_d, u = labels.to(DEV), disp.to(DEV)
    fused, conf = ops.label_fusion(lab_d, u, return_confidence=True, n_targets=n)
    fused_b, conf_b = ops.label_fusion(lab_d, u, return_confidence=True, n_targets=n)
    only = ops.label_fusion(lab_d, u, n_targets=n)
    assert torch.equal(fused, fused_b) and torch.equal(conf, conf_b) and torch.equal(only, fused)          # two runs are bit-identical
    assert torch.equal(metrics.atlas_label_fusion(lab_d, u, n_targets=n), fused)                           # the library entry, per-target maps included
    _check_vote(fused, conf, oracle, k, 'majority K = %d' % k)
    # conf = 1 exactly where all atlases agree
    agree = (oracle['warped'] == oracle['warped'][:, :1]).all(1) & ~oracle['excluded']
    assert bool((conf.cpu()[agree] == 1.0).all())                  # (K copies of one atlas, in the constructed cases, agree everywhere)
    if k > 1:
        assert float((oracle['gap'] == 0).double().mean()) > 0.02          # the tie rule is exercised


EXACT = [((24, 40, 56), 5), ((33, 47, 61), 9), ((9, 5, 7), 17), ((16, 12, 20), 32), ((33, 47, 61), 2)]


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64], ids=['u8', 'i64'])
@pytest.mark.parametrize('shape,k', EXACT, ids=['%dx%dx%d-k%d' % (s + (k,)) for s, k in EXACT])
def test_constructed_votes_are_exact_everywhere(shape, k, dtype):
    from deepatlas_amd import ops
    D, H, W = shape
    labels = fc.atlas_labels(shape, k, dtype, 'blocky', seed=40)
    lab_d = labels.to(DEV)
    zero = torch.zeros((k, 3) + shape)

    def device_vote(disp, lab=lab_d, w=None):
        f, c = ops.label_fusion(lab, disp.to(DEV), w, return_confidence=True, n_targets=1)
        return f.cpu().to(torch.int64), c.cpu().double()

    def check(warped, disp, tag):
        want = fc.vote_from_warped((warped.to(torch.int64) % 256)[None])
        f, c = device_vote(disp)
        assert torch.equal(f, want['fused']), tag
        assert float((c - want['conf']).abs().max()) <= CONF_REL, tag
    # zero displacement: the per-voxel mode of the atlas maps
    check(labels, zero, 'zero')
    # integer translations that differ per atlas
    u = torch.zeros((k, 3) + shape, dtype=torch.float64)
    shifts = [((3 * a) % 5 - 2, (2 * a) % 3 - 1, (a % 4) - 1) for a in range(k)]
    warped = torch.stack([fc.shifted(labels[a], *shifts[a]) for a in range(k)])
    for a, (tx, ty, tz) in enumerate(shifts):
        u[a, 0] = tx; u[a, 1] = ty; u[a, 2] = tz
    check(warped, rc.to_normalised(u).float(), 'translations')
    # fields pointing far outside: every vote is 0
    for far in (5.0, -7.0, 1e6):
        f, c = device_vote(torch.full((k, 3) + shape, far))
        assert int(f.max()) == 0 and bool((c == 1.0).all())
    # non-finite displacements in some atlases: those atlases vote 0 there, the others are untouched
    u = torch.zeros((k, 3) + shape)
    warped = labels.clone()
    u[0, 0, 1, 2, 3] = float('nan'); warped[0, 1, 2, 3] = 0
    u[k - 1, 1, 2, 1, 0] = float('inf'); warped[k - 1, 2, 1, 0] = 0
    u[k // 2, 2, 0, 0, 1] = float('-inf'); warped[k // 2, 0, 0, 1] = 0
    u[k // 2, :, 3] = float('nan'); warped[k // 2, 3] = 0
    check(warped, u, 'non-finite')
    # K = 1 is the nearest-neighbour label warp, bit for bit; atlas 0 repeated K times is K = 1; a permutation changes nothing
    smooth = rc.smooth_field(shape, k, 2.0, seed=41).to(DEV)
    one = ops.label_fusion(lab_d[:1], smooth[:1])
    assert torch.equal(one, ops.warp_labels_nearest(lab_d[:1], smooth[:1]))
    rep, rep_c = ops.label_fusion(lab_d[:1].repeat(k, 1, 1, 1), smooth[:1].repeat(k, 1, 1, 1, 1), return_confidence=True)
    assert torch.equal(rep, one) and bool((rep_c == 1.0).all())
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(5)).to(DEV)
    a, ac = ops.label_fusion(lab_d, smooth, return_confidence=True)
    b, bc = ops.label_fusion(lab_d[perm], smooth[perm], return_confidence=True)
    assert torch.equal(a, b) and torch.equal(ac, bc)


def test_label_fusion_rejects_wrong_shapes_and_dtypes():
    from deepatlas_amd import ops, _native
    shape = (4, 6, 8)
    lab = torch.zeros((3,) + shape, dtype=torch.uint8, device=DEV)
    disp = torch.zeros((6, 3) + shape, device=DEV)
    assert tuple(ops.label_fusion(lab, disp).shape) == (2,) + shape                      # K x D x H x W labels: N = batch / K
    assert tuple(ops.label_fusion(lab.repeat(2, 1, 1, 1), disp).shape) == (1,) + shape   # (N K) maps, no other hint: one target
    assert tuple(ops.label_fusion(lab.repeat(2, 1, 1, 1), disp, n_targets=2).shape) == (2,) + shape
    with pytest.raises(ValueError):
        ops.label_fusion(lab, disp[:5])                                                  # 5 fields are not N x 3
    with pytest.raises(ValueError):
        ops.label_fusion(lab, disp[:, :2])
    with pytest.raises(ValueError):
        ops.label_fusion(lab.float(), disp)
    with pytest.raises(ValueError):
        ops.label_fusion(lab[:, :3], disp)
    with pytest.raises(ValueError):
        ops.label_fusion(lab, disp, torch.ones((2, 4), device=DEV))                      # weights say K = 4
    with pytest.raises(ValueError):
        ops.label_fusion(lab, disp, torch.ones((2, 3), device=DEV).double())
    with pytest.raises(ValueError):
        ops.label_fusion(lab, disp, torch.ones((2, 3, 4, 6, 7), device=DEV))
    with pytest.raises(ValueError):
        ops.label_fusion(torch.zeros((33,) + shape, dtype=torch.uint8, device=DEV), torch.zeros((33, 3) + shape, device=DEV))
    with pytest.raises(ValueError):
        ops.local_msd_weights(torch.zeros((1, 2) + shape, device=DEV), torch.zeros((1,) + shape, device=DEV), radius=5)
    with pytest.raises(ValueError):
        ops.local_msd_weights(torch.zeros((1, 2) + shape, device=DEV), torch.zeros((2,) + shape, device=DEV))
    with pytest.raises(ValueError):
        ops.local_msd_weights(torch.zeros((1, 2) + shape, device=DEV), torch.zeros((1,) + shape, device=DEV), sigma=0.0)
    with pytest.raises(_native.NativeError):
        ops.label_fusion(lab.cpu(), disp)


# ---- weights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['atlas', 'voxel'])
@pytest.mark.parametrize('case', fc.WEIGHT_CASES, ids=fc.WEIGHT_IDS)
def test_weighted_vote_with_exactly_summable_weights(case, form):
    from deepatlas_amd import ops
    shape, n, k = case[:3]
    labels, disp, plain = _case(_index(case))
    w = fc.exact_weights((n, k) if form == 'atlas' else (n, k) + tuple(shape), seed=60 + k)
    oracle = dict(fc.vote_from_warped(plain['warped'], w), excluded=plain['excluded'])
    lab_d, u, w_d = labels.to(DEV), disp.to(DEV), w.to(DEV)
    fused, conf = ops.label_fusion(lab_d, u, w_d, return_confidence=True)
    fused_b, conf_b = ops.label_fusion(lab_d, u, w_d, return_confidence=True)
    assert torch.equal(fused, fused_b) and torch.equal(conf, conf_b)
    _check_vote(fused, conf, oracle, k, '%s weights K = %d' % (form, k))
    # an atlas of weight 0 never changes the result: the vote without it is the same vote
    drop = k // 2
    w0 = w.clone(); w0[:, drop] = 0
    keep = [a for a in range(k) if a != drop]
    with_zero = ops.label_fusion(lab_d, u, w0.to(DEV), return_confidence=True)
    if k > 1:
        lab_k = labels.view((n, k) + tuple(shape))[:, keep].reshape((n * (k - 1),) + tuple(shape)) if labels.shape[0] == n * k else labels[keep]
        u_k = disp.view((n, k, 3) + tuple(shape))[:, keep].reshape((n * (k - 1), 3) + tuple(shape))
        without = ops.label_fusion(lab_k.to(DEV), u_k.to(DEV), w0[:, keep].contiguous().to(DEV), return_confidence=True)
        assert torch.equal(with_zero[0], without[0]) and torch.equal(with_zero[1], without[1])
    # all-zero weights: fused 0, conf 0
    z = ops.label_fusion(lab_d, u, torch.zeros_like(w_d), return_confidence=True)
    assert int(z[0].max()) == 0 and float(z[1].abs().max()) == 0.0
    # conf = 1 exactly where all atlases agree (and carry some weight)
    agree = (plain['warped'] == plain['warped'][:, :1]).all(1) & ~plain['excluded'] & (oracle['total'] > 0)
    assert bool((conf.cpu()[agree] == 1.0).all())
    # unit weights are the majority vote
    ones = ops.label_fusion(lab_d, u, torch.ones_like(w_d), return_confidence=True)
    maj = ops.label_fusion(lab_d, u, return_confidence=True, n_targets=n)
    assert torch.equal(ones[0], maj[0]) and torch.equal(ones[1], maj[1])


def test_per_voxel_weights_at_an_unaligned_address_take_the_element_path():
    """A voxel count that is a multiple of 4 with a weight field that starts 4 bytes past a 16-byte boundary: the kernel may not use its
    16-byte accesses; the result is the aligned call's, bit for bit, and the oracle's."""
    from deepatlas_amd import ops
    case = fc.VOTE_CASES[3]
    shape, n, k = case[:3]
    assert (shape[0] * shape[1] * shape[2]) % 4 == 0
    labels, disp, plain = _case(3)
    w = fc.exact_weights((n, k) + tuple(shape), seed=61)
    lab_d, u, w_d = labels.to(DEV), disp.to(DEV), w.to(DEV)
    shifted = torch.empty(w.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(w.shape)
    shifted.copy_(w_d)
    assert shifted.is_contiguous() and w_d.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    want = ops.label_fusion(lab_d, u, w_d, return_confidence=True)
    got = ops.label_fusion(lab_d, u, shifted, return_confidence=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    _check_vote(got[0], got[1], dict(fc.vote_from_warped(plain['warped'], w), excluded=plain['excluded']), k, 'unaligned per-voxel weights')


# ---- weights of locally weighted voting ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fc.MSD_CASES, ids=fc.MSD_IDS)
def test_local_msd_weights_against_numpy_fp64(case):
    from deepatlas_amd import ops
    shape, n, k, r, sigma = case
    warped, target = fc.msd_inputs(case)
    w64, bound, yard = fc.msd_bound(warped, target, r, sigma)
    a, b = warped.to(DEV), target.to(DEV)
    got = ops.local_msd_weights(a, b, radius=r, sigma=sigma)
    again = ops.local_msd_weights(a, b[:, None], radius=r, sigma=sigma)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, k) + tuple(shape) and torch.equal(got, again)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - w64).max())
    print('local_msd_weights r = %d sigma = %g %s: fp32 numpy yardstick %.3e, bound %.3e, device error %.3e = %.2f of the yardstick'
          % (r, sigma, 'x'.join(str(s) for s in shape), yard, bound, err, err / yard))
    assert err <= bound


@pytest.mark.parametrize('r,sigma', [(1, 0.05), (2, 0.2), (4, 0.2)])
def test_local_msd_weights_closed_forms(r, sigma):
    from deepatlas_amd import ops
    shape = (11, 13, 12)
    g = torch.Generator().manual_seed(7)
    t = torch.rand((2,) + shape, generator=g)
    same = ops.local_msd_weights(t[:, None].repeat(1, 3, 1, 1, 1).to(DEV), t.to(DEV), radius=r, sigma=sigma)
    assert bool((same == 1.0).all())                                                    # equal images: exactly 1
    # a constant difference c between exactly representable images: m = c^2 at interior voxels
    c = 0.25
    t = (torch.randint(0, 64, (1,) + shape, generator=g).float() / 128.0)
    got = ops.local_msd_weights((t + c)[:, None].to(DEV), t.to(DEV), radius=r, sigma=sigma).cpu().double()
    want = np.exp(-c * c / (2 * sigma * sigma))
    inner = got[0, 0, r:shape[0] - r, r:shape[1] - r, r:shape[2] - r]
    assert inner.numel() > 0
    # the window sum of (2 r + 1)^3 equal terms c^2 = 1 / 16 is exact, so is the division: one fp32 product and one expf remain
    assert float((inner - want).abs().max()) <= 4 * 2.0 ** -24 * max(1.0, c * c / (2 * sigma * sigma)) * want + 2.0 ** -24
    corner = np.exp(-c * c * ((r + 1.0) / (2 * r + 1.0)) ** 3 / (2 * sigma * sigma))
    # (the corner's (r + 1)^3 equal terms sum exactly too; the division by (2 r + 1)^3 rounds, which adds one more relative 2^-24 x the exponent)
    xc = c * c * ((r + 1.0) / (2 * r + 1.0)) ** 3 / (2 * sigma * sigma)
    assert abs(float(got[0, 0, 0, 0, 0]) - corner) <= 6 * 2.0 ** -24 * max(1.0, xc) * corner + 2.0 ** -24


# ---- locally weighted vote end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fc.LOCAL_CASES, ids=fc.LOCAL_IDS)
def test_locally_weighted_vote_end_to_end(case):
    from deepatlas_amd import ops
    shape, n, k = case[:3]
    labels, disp, plain = _case(_index(case))
    g = torch.Generator().manual_seed(70 + k)
    full = labels if labels.shape[0] == n * k else labels.repeat(n, 1, 1, 1)
    atlas_img = (full.float() / (fc.N_CLASS_BLOCKY - 1) + 0.1 * torch.rand(full.shape, generator=g)).clamp_(0, 1)
    target_lab = fc.atlas_labels(shape, n, torch.uint8, 'blocky', seed=90)
    target_img = (target_lab.float() / (fc.N_CLASS_BLOCKY - 1) + 0.1 * torch.rand(target_lab.shape, generator=g)).clamp_(0, 1)
    u = disp.to(DEV)
    warped_img = ops.WarpFn.apply(atlas_img[:, None].to(DEV), u)[0].reshape((n, k) + tuple(shape))
    w = ops.local_msd_weights(warped_img, target_img.to(DEV), radius=2, sigma=0.1)
    fused, conf = ops.label_fusion(labels.to(DEV), u, w, return_confidence=True)
    fused_b, conf_b = ops.label_fusion(labels.to(DEV), u, w, return_confidence=True)
    assert torch.equal(fused, fused_b) and torch.equal(conf, conf_b)
    w_host = w.cpu()
    assert float(w_host.min()) >= 0.0 and float(w_host.max()) <= 1.0 and float(w_host.max() - w_host.min()) > 0.05
    oracle = dict(fc.vote_from_warped(plain['warped'], w_host), excluded=plain['excluded'])
    near_tie = oracle['gap'] < fc.NEAR_TIE
    _check_vote(fused, None, oracle, k, 'local K = %d' % k, extra_excluded=near_tie, cap_extra=fc.MAX_NEAR_TIE)
    c = conf.cpu().double()
    ok = ~(plain['excluded'] | near_tie) & (oracle['conf'] > 0)
    rel = float(((c - oracle['conf']).abs() / oracle['conf'].clamp_min(1e-300))[ok].max())
    print('local K = %d: conf max relative error %.3e (fp32 sums of %d arbitrary weights)' % (k, rel, k))
    assert rel <= 2 * k * 2.0 ** -24              # k - 1 fp32 additions of positive terms in each of the two sums and one division, half an ulp each


# ---- library and experiments -----------------------------------------------------------------------------------------------------
LIB_SHAPE = (16, 16, 32)


def _reg_net(zero_flow, seed=3):
    from deepatlas_amd import ops
    from deepatlas_amd.lib.network_factory import get_network
    torch.manual_seed(seed)
    net = get_network('voxel_morph_cvpr')()
    net.weights_init()
    if zero_flow:
        net.flow.weight.data.zero_()
        net.flow.bias.data.zero_()
    else:
        net.flow.bias.data.copy_(torch.tensor([0.05, -0.04, 0.03]))
    ops.bump_weights_epoch()
    return net.to(DEV)


def _volumes(n, seed):
    from deepatlas_amd.lib.datasets import SyntheticSegDataset
    ds = SyntheticSegDataset(n, LIB_SHAPE, 32, seed=seed)
    return torch.stack([ds[i][0] for i in range(n)]), torch.stack([ds[i][1] for i in range(n)])


def test_atlas_segmentation_with_a_zero_field_is_the_mode_of_the_atlas_labels():
    from deepatlas_amd.lib import evalMetrics as metrics
    net = _reg_net(zero_flow=True)
    ims, labs = _volumes(6, seed=11)
    for mode in ('majority', 'local'):
        fused, conf = metrics.atlas_segmentation(net, ims[:5].to(DEV), labs[:5].to(DEV), ims[5].to(DEV), mode=mode, chunk=2)
        assert fused.dtype == torch.uint8 and tuple(fused.shape) == (1,) + LIB_SHAPE and tuple(conf.shape) == (1,) + LIB_SHAPE
        if mode == 'majority':
            want = fc.vote_from_warped(labs[:5].to(torch.int64)[None])
            assert torch.equal(fused.cpu().to(torch.int64), want['fused'])
            assert float((conf.cpu().double() - want['conf']).abs().max()) <= CONF_REL
            assert torch.equal(metrics.atlas_label_fusion(labs[:5].to(DEV), torch.zeros((5, 3) + LIB_SHAPE, device=DEV)), fused)


def test_atlas_segmentation_composes_the_ops_and_k1_dice_is_the_registration_dice():
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics as metrics
    net = _reg_net(zero_flow=False)
    ims, labs = _volumes(5, seed=21)
    ims_d, labs_d = ims.to(DEV), labs.to(DEV)
    target, truth = ims_d[4:5], labs_d[4:5]
    with torch.no_grad():
        net.eval()
        disp = torch.cat([net(ims_d[a:a + 1], target)[0] for a in range(4)], 0)
        assert float(disp.abs().max()) > 0
        # K = 1: the Dice of the fused map = registration_dice of that pair, bit for bit
        fused1, conf1 = metrics.atlas_segmentation(net, ims_d[:1], labs_d[:1], target, chunk=4)
        d1 = metrics.dice_from_counts(ops.label_overlap_counts(fused1, truth, 32))[:, 1:]
        assert np.array_equal(d1, metrics.registration_dice(labs_d[:1], truth, disp[:1], 32), equal_nan=True)
        assert bool((conf1 == 1.0).all())
        # K = 4: majority and local modes equal the composition of the ops on the net's own fields, whatever the chunking
        for chunk in (1, 3, 4):
            fused, conf = metrics.atlas_segmentation(net, ims_d[:4], labs_d[:4], target, mode='majority', chunk=chunk)
            want = ops.label_fusion(labs_d[:4], disp, return_confidence=True)
            assert torch.equal(fused, want[0]) and torch.equal(conf, want[1])
        warped = ops.WarpFn.apply(ims_d[:4], disp)[0]
        w = ops.local_msd_weights(warped.reshape((1, 4) + LIB_SHAPE), target[:, 0], radius=1, sigma=0.2)
        fused, conf = metrics.atlas_segmentation(net, ims_d[:4], labs_d[:4], target, mode='local', radius=1, sigma=0.2, chunk=2)
        want = ops.label_fusion(labs_d[:4], disp, w, return_confidence=True)
        assert torch.equal(fused, want[0]) and torch.equal(conf, want[1])
    with pytest.raises(ValueError):
        metrics.atlas_segmentation(net, ims_d[:4], labs_d[:4], target, mode='median')


JOINT_KEYS = {'dice_per_class', 'dice_avg', 'identity_dice_per_class', 'identity_dice_avg', 'nonpos_frac', 'det_mean', 'det_std', 'n_pairs',
              'n_dice_pairs', 'seg_dice_per_class', 'seg_dice_avg'}


def _joint_experiment(tmp, **extra):
    import train_joint
    from deepatlas_amd.lib.datasets import SyntheticRegDataset, SyntheticSegDataset
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    ns = argparse.Namespace(device='0', debug=False, num_samples=3, num_epochs=1, lr=1e-3, test_only=False, data_root='./data', log_root=tmp,
                            shape=list(LIB_SHAPE), num_labeled=2)
    cfg = train_joint.build_config(ns)
    labeled = DeepAtlasExperiment.labeled_subset(3, 2, cfg['random_seed'])
    data = SyntheticRegDataset(3, LIB_SHAPE, 32, seed=230, labeled=labeled)
    cfg.update(lr_mode='const', samples_per_epoch=len(data), print_batch_period=2, **extra)
    cfg['training_data_loader'] = DataLoader(data, batch_size=1, shuffle=False)
    cfg['validation_data_loader'] = DataLoader(SyntheticSegDataset(2, LIB_SHAPE, 32, seed=1230), batch_size=1, shuffle=False)
    cfg['validation_pair_loader'] = DataLoader(SyntheticRegDataset(2, LIB_SHAPE, 32, seed=1230), batch_size=1, shuffle=False)
    return DeepAtlasExperiment(cfg), labeled


def _same(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=True)
    if torch.is_tensor(a):
        return torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
    return a == b or (a != a and b != b)


def test_deepatlas_experiment_reports_the_atlas_fusion_dice(tmp_path, monkeypatch, capsys):
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics as metrics
    from deepatlas_amd.models.registration import _nanmean
    monkeypatch.chdir(tmp_path)
    ops.set_deterministic(True)
    exp, labeled = _joint_experiment('fusion', atlas_fusion='majority')
    assert 'atlas' not in exp.exp_name
    exp.train()
    res = exp.last_validation
    assert set(res) == JOINT_KEYS | {'atlas_dice_per_class', 'atlas_dice_avg'}
    assert 'atlas-fusion Dice Avg: %.4f' % res['atlas_dice_avg'] in capsys.readouterr().out
    # recomputation from the run's own fields: per validation volume the fused map on the device, held to the float64 oracle on every voxel
    # outside the band (excluded share under K x 1e-3, _check_vote); the Dice of that device map, aggregated as the experiment aggregates
    # it, is what the run must report bit for bit
    train = exp.training_data_loader.dataset.seg
    atl_im = torch.stack([train[i][0] for i in labeled]).to(DEV)
    atl_lab = torch.stack([train[i][1] for i in labeled])
    k_atl = len(labeled)
    rows, n_excl = [], 0
    with torch.no_grad():
        exp.reg_model.eval()
        valid = exp.validation_data_loader.dataset
        for im, seg, name in (valid[i] for i in range(len(valid))):      # (by index: the synthetic datasets generate a volume for any index)
            disp = exp.reg_model(atl_im, im.to(DEV)[None].expand(k_atl, -1, -1, -1, -1).contiguous())[0]
            fused = ops.label_fusion(atl_lab.to(DEV), disp, n_targets=1)
            o = fc.vote_oracle(atl_lab, disp.cpu(), 1, k_atl)
            _check_vote(fused, None, o, k_atl, 'experiment, %s' % name)
            k = int(o['excluded'].sum())
            n_excl += k
            dev = metrics.dice_from_counts(ops.label_overlap_counts(fused, seg.to(DEV)[None], 32))[:, 1:]
            c = rc.counts_np(o['fused'].numpy(), seg[None].numpy(), 32).astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                d = (2.0 * c[..., 2] / (c[..., 0] + c[..., 1]))[:, 1:]
            # at most k voxels differ: |P & T| and |P| move by at most k each, so Dice = 2 I / (P + T) moves by at most 4 k / (P + T - k)
            denom = (c[..., 0] + c[..., 1])[:, 1:]
            tol = np.where(denom > k, 4.0 * k / np.maximum(denom - k, 1), np.inf)
            both = np.isfinite(d) & np.isfinite(dev)
            assert both.any() and np.all(np.abs(d - dev)[both] <= tol[both])
            if k == 0:
                assert np.array_equal(d, dev, equal_nan=True)
            rows.append(dev)
    per = _nanmean(np.concatenate(rows, 0), axis=0)
    print('atlas_dice_avg %.6f, recomputed %.6f, %d voxels in the exclusion band' % (res['atlas_dice_avg'], float(np.nanmean(per)), n_excl))
    assert np.array_equal(res['atlas_dice_per_class'], per, equal_nan=True)           # mean over the volumes that have the class
    assert res['atlas_dice_avg'] == float(np.nanmean(per))                            # mean over the classes that occur
    assert 0.0 <= res['atlas_dice_avg'] <= 1.0
    tested = exp.test()
    assert set(tested) == set(res)
    assert 'atlas-fusion Dice Avg: %.4f' % tested['atlas_dice_avg'] in capsys.readouterr().out     # (and what the fusion run printed ends here)

    # the same run without the key: today's result keys, and bit-equal to a second run
    ops.set_deterministic(True)
    a, _ = _joint_experiment('plain_a')
    a.train()
    out = capsys.readouterr().out
    assert 'atlas' not in out
    ops.set_deterministic(True)
    b, _ = _joint_experiment('plain_b')
    b.train()
    assert set(a.last_validation) == JOINT_KEYS == set(b.last_validation)
    for key in JOINT_KEYS:
        assert _same(a.last_validation[key], b.last_validation[key]), key
    for (ka, va), (kb, vb) in zip(a.reg_model.state_dict().items(), b.reg_model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    # the key adds numbers, it does not change the others or the training
    for key in JOINT_KEYS:
        assert _same(a.last_validation[key], res[key]), key
    for (ka, va), (kb, vb) in zip(a.seg_model.state_dict().items(), exp.seg_model.state_dict().items()):
        assert torch.equal(va, vb), ka


def test_train_reg_command_line_with_local_atlas_fusion(tmp_path, monkeypatch):
    import train_reg
    monkeypatch.chdir(tmp_path)
    res = train_reg.main(['--num-samples', '3', '--num-epochs', '1', '--device', '0', '--shape'] + [str(s) for s in LIB_SHAPE] +
                         ['--log-root', 'reg', '--atlas-fusion', 'local'])
    assert {'atlas_dice_per_class', 'atlas_dice_avg', 'dice_avg', 'nonpos_frac'} <= set(res)
    assert res['atlas_dice_per_class'].shape == (31,) and 0.0 <= res['atlas_dice_avg'] <= 1.0
