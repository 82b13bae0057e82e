"""GPU: the registration-evaluation kernels (csrc/regeval.hip) against references that are not the code under test -- torch-CPU
grid_sample(mode='nearest') in float64 and numpy.gradient in float64 (tests/regeval_cases.py) -- plus constructed cases with exact
answers, the device-versus-device identity of the fused counts, determinism, and one case at the size users run (160 x 192 x 160)."""
import numpy as np
import pytest
import torch

import regeval_cases as rc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
C = rc.N_CLASS


def _check_warp_against_oracle(lab, disp, tag):
    """Per voxel: exact outside the exclusion band, the band capped at 0.2 %.  Returns (device map on the host, oracle, excluded)."""
    from deepatlas_amd import ops
    got = ops.warp_labels_nearest(lab.to(DEV), disp.to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(lab.shape)
    got = got.cpu().to(torch.int64)
    want, excluded = rc.nearest_oracle(lab, disp)
    share = float(excluded.double().mean())
    wrong = (got != want) & ~excluded
    print('%s: excluded share %.3e, mismatches inside the band %d, outside %d' % (tag, share, int(((got != want) & excluded).sum()), int(wrong.sum())))
    assert share <= rc.MAX_EXCLUDED
    assert not bool(wrong.any())
    return got, want, excluded


@pytest.mark.parametrize('shape,n,sigma,dtype', rc.WARP_CASES, ids=rc.WARP_IDS)
def test_nearest_warp_matches_the_fp64_oracle_per_voxel(shape, n, sigma, dtype):
    disp = rc.smooth_field(shape, n, sigma, seed=11)
    lab = rc.random_labels(shape, n, dtype, seed=12)
    _check_warp_against_oracle(lab, disp, 'warp')


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64], ids=['u8', 'i64'])
@pytest.mark.parametrize('shape,n', [((24, 40, 56), 3), ((33, 47, 61), 1), ((9, 5, 7), 2)], ids=['24x40x56', '33x47x61', '9x5x7'])
def test_nearest_warp_constructed_cases_are_exact(shape, n, dtype):
    from deepatlas_amd import ops
    D, H, W = shape
    lab = rc.random_labels(shape, n, dtype, seed=5)
    lab_d = lab.to(DEV)
    zero = torch.zeros((n, 3) + shape, device=DEV)
    # zero displacement: the input, bit for bit
    assert torch.equal(ops.warp_labels_nearest(lab_d, zero).cpu(), lab.to(torch.uint8))
    # integer-voxel translations: an exact shift with zero fill
    for tx, ty, tz in ((2, -1, 3), (-3, 2, 0), (0, 0, -2), (W - 1, 0, 0)):
        u = torch.zeros((n, 3) + shape, dtype=torch.float64)
        u[:, 0] = tx; u[:, 1] = ty; u[:, 2] = tz
        got = ops.warp_labels_nearest(lab_d, rc.to_normalised(u).float().to(DEV)).cpu()
        want = torch.zeros_like(lab)
        d0, d1 = max(0, -tz), min(D, D - tz)
        h0, h1 = max(0, -ty), min(H, H - ty)
        w0, w1 = max(0, -tx), min(W, W - tx)
        want[:, d0:d1, h0:h1, w0:w1] = lab[:, d0 + tz:d1 + tz, h0 + ty:h1 + ty, w0 + tx:w1 + tx]
        assert torch.equal(got, want.to(torch.uint8)), (tx, ty, tz)
    # a field pointing far outside: all zeros
    for far in (5.0, -7.0, 1e6):
        assert int(ops.warp_labels_nearest(lab_d, torch.full((n, 3) + shape, far, device=DEV)).max()) == 0
    # non-finite displacement gives 0 there and leaves the other voxels alone
    u = torch.zeros((n, 3) + shape)
    u[:, 0, 1, 2, 3] = float('nan'); u[:, 1, 2, 1, 0] = float('inf'); u[:, 2, 0, 0, 1] = float('-inf')
    got = ops.warp_labels_nearest(lab_d, u.to(DEV)).cpu()
    want = lab.to(torch.uint8).clone()
    want[:, 1, 2, 3] = 0; want[:, 2, 1, 0] = 0; want[:, 0, 0, 1] = 0
    assert torch.equal(got, want)
    assert int(ops.warp_labels_nearest(lab_d, torch.full((n, 3) + shape, float('nan'), device=DEV)).max()) == 0


def _check_counts(lab_m, lab_t, disp, n_class, tag):
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics as metrics
    m, t, u = lab_m.to(DEV), lab_t.to(DEV), disp.to(DEV)
    warped = ops.warp_labels_nearest(m, u)
    composed = ops.label_overlap_counts(warped, t, n_class)
    fused = ops.reg_label_counts(m, t, u, n_class)
    fused2, warped2 = ops.reg_label_counts(m, t, u, n_class, return_warped=True)
    assert fused.dtype == torch.int64 and tuple(fused.shape) == (lab_m.shape[0], n_class, 3)
    assert torch.equal(fused, composed) and torch.equal(fused2, composed) and torch.equal(warped2, warped)      # integers: no tolerance
    # against the fp64 oracle
    want, excluded = rc.nearest_oracle(lab_m, disp)
    n_excl = int(excluded.sum())
    assert n_excl <= rc.MAX_EXCLUDED * excluded.numel()
    oc = rc.counts_np(want.numpy() % 256, lab_t.numpy(), n_class)          # (the warped map is uint8)
    got = fused.cpu().numpy()
    d0, d2 = int(np.abs(got[:, :, 0] - oc[:, :, 0]).sum()), int(np.abs(got[:, :, 2] - oc[:, :, 2]).sum())
    print('%s: excluded voxels %d, count differences |warped| %d, |both| %d' % (tag, n_excl, d0, d2))
    assert np.array_equal(got[:, :, 1], oc[:, :, 1])
    assert d0 <= 2 * n_excl and d2 <= 2 * n_excl
    # registration_dice = dice_from_counts of those counts, NaN convention included
    dice = metrics.registration_dice(m, t, u, n_class)
    ref = metrics.dice_from_counts(composed)[:, 1:]
    assert dice.dtype == np.float64 and dice.shape == (lab_m.shape[0], n_class - 1)
    assert np.array_equal(dice, ref, equal_nan=True)
    c = got.astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        by_hand = (2.0 * c[:, 1:, 2] / (c[:, 1:, 0] + c[:, 1:, 1]))
    assert np.array_equal(dice, by_hand, equal_nan=True)
    return dice


@pytest.mark.parametrize('shape,n,sigma,dtype', rc.WARP_CASES, ids=rc.WARP_IDS)
def test_fused_counts_equal_the_composition_and_the_oracle(shape, n, sigma, dtype):
    disp = rc.smooth_field(shape, n, sigma, seed=21)
    lab_m = rc.random_labels(shape, n, dtype, seed=22)
    lab_t = rc.random_labels(shape, n, torch.uint8 if dtype == torch.int64 else torch.int64, seed=23)
    _check_counts(lab_m, lab_t, disp, C, 'counts')


def test_fused_counts_ignore_labels_outside_the_class_range_and_keep_the_nan_convention():
    shape, n = (24, 40, 56), 2
    disp = rc.smooth_field(shape, n, 1.5, seed=31)
    lab_m = rc.random_labels(shape, n, torch.int64, seed=32, n_class=40)          # labels 32..39 are outside [0, 32)
    lab_t = rc.random_labels(shape, n, torch.uint8, seed=33, n_class=40)
    lab_t[0][lab_t[0] == 40 - 1] = 255
    _check_counts(lab_m, lab_t, disp, C, 'out-of-range')
    # classes absent from both maps give NaN, as metricEval('dice', ...) does
    lab_m2, lab_t2 = lab_m % 5, (lab_t % 5).to(torch.uint8)
    dice = _check_counts(lab_m2, lab_t2, disp, C, 'absent classes')
    assert np.isnan(dice[:, 4:]).all() and np.isfinite(dice[:, :4]).all()
    # blocky anatomical maps (long runs of equal pairs: the in-register merging path)
    from deepatlas_amd.lib.datasets import structured_labels
    sm = torch.stack([structured_labels(shape, C, seed=i) for i in range(n)])
    st_ = torch.stack([structured_labels(shape, C, seed=i + 3) for i in range(n)])
    _check_counts(sm, st_, disp, C, 'structured')


def test_full_size_warp_and_counts():
    """160 x 192 x 160, N = 1: device-versus-device exact, and against the fp64 oracle under the exclusion rule."""
    shape = rc.FULL_SHAPE
    disp = rc.smooth_field(shape, 1, 4.0, seed=41)
    lab_m = rc.random_labels(shape, 1, torch.uint8, seed=42)
    lab_t = rc.random_labels(shape, 1, torch.uint8, seed=43)
    _check_warp_against_oracle(lab_m, disp, 'full-size warp')
    _check_counts(lab_m, lab_t, disp, C, 'full-size counts')


# ---- Jacobian determinant ----------------------------------------------------------------------------------------------------------
def _check_jacobian(disp, tag):
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics as metrics
    det64, bound, yard = rc.jacobian_bound(disp)
    u = disp.to(DEV)
    stats, det = ops.jacobian_det(u, return_map=True)
    stats_b, det_b = ops.jacobian_det(u, return_map=True)
    stats_only = ops.jacobian_det(u)
    torch.cuda.synchronize()
    assert det.dtype == torch.float32 and tuple(det.shape) == det64.shape
    assert torch.equal(det, det_b) and torch.equal(stats, stats_b)                 # two runs are bit-identical
    assert torch.equal(stats_only, stats)                                           # statistics-only call = statistics of the call with a map
    got = det.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - det64).max())
    print('%s: max|det| %.4g, fp32 numpy yardstick %.3e (%.2e of max|det|), bound %.3e, device error %.3e' %
          (tag, np.abs(det64).max(), yard, yard / np.abs(det64).max(), bound, err))
    assert err <= bound
    js = metrics.jacobian_stats(u)
    N = det64.shape[0]
    flat = det64.reshape(N, -1)
    assert set(js) == {'mean', 'std', 'min', 'max', 'n_nonpos', 'nonpos_frac'}
    for k in js:
        assert js[k].dtype == np.float64 and js[k].shape == (N,), k
    assert np.abs(js['mean'] - flat.mean(1)).max() <= bound
    assert np.abs(js['std'] - flat.std(1)).max() <= 2 * bound                      # population form; absolute (a zero field has std 0)
    assert np.abs(js['min'] - flat.min(1)).max() <= bound and np.abs(js['max'] - flat.max(1)).max() <= bound
    lo, hi = (flat <= -bound).sum(1), (flat <= bound).sum(1)
    print('%s: folding count device %s, oracle interval [%s, %s], fraction %s' % (tag, js['n_nonpos'], lo, hi, js['nonpos_frac']))
    assert np.all(js['n_nonpos'] >= lo) and np.all(js['n_nonpos'] <= hi)
    assert np.array_equal(js['nonpos_frac'], js['n_nonpos'] / flat.shape[1])
    # the raw sums the C entry returns
    s = stats.cpu().numpy()
    assert np.all(np.abs(s[:, 0] - got.reshape(N, -1).sum(1)) <= 1e-12 * np.abs(got.reshape(N, -1)).sum(1))        # double accumulation of the fp32 map
    assert np.array_equal(s[:, 4], (got.reshape(N, -1) <= 0).sum(1))
    assert np.array_equal(s[:, 2], got.reshape(N, -1).min(1)) and np.array_equal(s[:, 3], got.reshape(N, -1).max(1))
    return js


@pytest.mark.parametrize('shape,n,sigma', rc.JAC_CASES, ids=rc.JAC_IDS)
def test_jacobian_matches_numpy_gradient_fp64(shape, n, sigma):
    disp = rc.smooth_field(shape, n, sigma, seed=51)
    if sigma >= 4.0:
        assert float((rc.jacobian_np(disp) <= 0).mean()) > 0.04            # (oracle) these fields fold: the folding regime is covered
    _check_jacobian(disp, 'jacobian')


def test_jacobian_of_a_rough_field():
    _check_jacobian(rc.noise_field((17, 30, 22), 2, 0.7, seed=52), 'noise field')


@pytest.mark.parametrize('shape', [(24, 40, 56), (33, 47, 61), (2, 2, 2), (2, 9, 3)], ids=['24x40x56', '33x47x61', '2x2x2', '2x9x3'])
def test_jacobian_of_affine_and_zero_fields_is_exact_everywhere(shape):
    from deepatlas_amd import ops
    js = _check_jacobian(torch.zeros((2, 3) + shape), 'zero field')              # the yardstick is 0 here: exactly 1 everywhere
    assert np.all(js['mean'] == 1.0) and np.all(js['std'] == 0.0) and np.all(js['n_nonpos'] == 0)
    rng = np.random.default_rng(3)
    for k in range(3):
        A = rng.standard_normal((3, 3)) * (0.15 if k < 2 else 0.9)
        disp = rc.affine_field(shape, A, n=2)
        _check_jacobian(disp, 'affine field %d' % k)
        det = ops.jacobian_det(disp.to(DEV), return_map=True)[1].cpu().numpy()
        want = np.linalg.det(np.eye(3) + A)
        # faces, edges and corners included.  The field is stored in fp32: a displacement of up to |A| size voxels carries 6e-8 of itself,
        # a difference of two of them twice that, and the determinant a few such terms -- 2e-5 of that scale is two orders above it
        assert np.abs(det - want).max() < 2e-5 * max(1.0, abs(want), np.abs(A).max() * max(shape))


def test_jacobian_full_size():
    _check_jacobian(rc.smooth_field(rc.FULL_SHAPE, 1, 4.0, seed=61), 'full-size jacobian')


def test_jacobian_rejects_thin_volumes():
    from deepatlas_amd import ops, _native
    with pytest.raises(_native.NativeError):
        ops.jacobian_det(torch.zeros((1, 3, 1, 8, 8), device=DEV))
    with pytest.raises(ValueError):
        ops.jacobian_det(torch.zeros((1, 2, 8, 8, 8), device=DEV))
