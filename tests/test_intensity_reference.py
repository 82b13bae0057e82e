"""CPU companion of test_gpu_intensity.py: the host side of the intensity augmentation (discrete_gaussian_taps, the draw order of the three
classes, make_augmentation, train_seg.py's flags) and the float64 references of tests/intensity_cases.py against independent restatements
(scipy.special.ive, scipy.ndimage.convolve1d, a per-voxel Python loop, a basis-matrix einsum, oracle/datapath.py's hash), plus the
guard-band facts asserted on the exact case lists the GPU file uses."""
import argparse

import numpy as np
import pytest
import torch
from scipy import ndimage, special

import intensity_cases as ic
from deepatlas_amd import ops
from deepatlas_amd.lib import transforms as T
from oracle import datapath as oracle_datapath


# ---- discrete_gaussian_taps ----------------------------------------------------------------------------------------------------------
def _taps_ive(variance, width, error):
    """ITK's GaussianOperator with scipy's exponentially scaled Bessel function; returns (taps, which exit ended the loop)"""
    c = [special.ive(0, variance), special.ive(1, variance)]
    total, i, why = c[0] + 2 * c[1], 2, 'sum'
    while total < 1 - error:
        c.append(special.ive(i, variance))
        total += 2 * c[i]
        if c[i] < total * np.finfo(float).eps:
            why = 'eps'
            break
        if len(c) > width:
            why = 'width'
            break
        i += 1
    c = np.array(c) / total
    return np.concatenate([c[:0:-1], c]), why


@pytest.mark.parametrize('variance', [0.0, 0.5, 2.0, 9.0])
@pytest.mark.parametrize('width,error,exit_', [(32, 0.01, 'sum'), (3, 1e-6, 'width'), (64, -1e-3, 'eps')])      # (a cap above 1 is never reached: the term-size exit ends the loop)
def test_discrete_gaussian_taps_against_scipy_ive(variance, width, error, exit_):
    want, why = _taps_ive(variance, width, error)
    if variance == 9.0 or exit_ == 'eps':
        assert why == exit_                                       # at this variance each combination ends the loop by the exit it is named for
    got = T.discrete_gaussian_taps(variance, width, error)
    assert got.dtype == np.float64 and got.shape == want.shape and len(got) % 2 == 1
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-300)
    assert abs(got.sum() - 1) < 1e-14
    np.testing.assert_array_equal(got, got[::-1])


def test_reference_default_is_three_taps_and_variance_zero_is_the_identity():
    t = T.discrete_gaussian_taps(0.5, 1, 0.9)
    assert len(t) == 3
    np.testing.assert_allclose(t, [0.163, 0.673, 0.163], atol=1e-3)
    np.testing.assert_array_equal(T.discrete_gaussian_taps(0, 1, 0.9), [0.0, 1.0, 0.0])
    np.testing.assert_allclose(ic.blur_taps()['default'][0], t, atol=1e-8)          # the GPU file's 'default' taps are these
    assert T.GaussianBlur().taps()[0].shape == (3,)
    assert len(T.discrete_gaussian_taps(4.0, 32, 0.01)) // 2 <= ops.BLUR_MAX_RADIUS       # what --aug-blur asks for fits the kernel
    assert max(len(t) for t in ic.blur_taps()['rmax']) // 2 == ops.BLUR_MAX_RADIUS


# ---- references against independent restatements ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('tname', sorted(ic.blur_taps()))
def test_blur_reference_equals_convolve1d_nearest(tname):
    taps = ic.blur_taps()[tname]
    tp, _ = ic.padded_taps(taps)
    for shape in ((1, 1, 5, 6, 7), (1, 2, 1, 3, 40), (1, 1, 2, 9, 4)):
        img = ic.rand_image(shape, 3).numpy()
        want = img.astype(np.float64)
        for axis, t in ((4, tp[0]), (3, tp[1]), (2, tp[2])):
            want = ndimage.convolve1d(want, t.astype(np.float64)[::-1], axis=axis, mode='nearest')   # (convolution flips: hand it the flipped taps)
        np.testing.assert_allclose(ic.blur_reference(img, taps), want, rtol=0, atol=1e-14)
        assert ic.tolerance(want, ic.blur_torch32(torch.from_numpy(img), taps))[1] < 1e-6


def _bilateral_loop(img, sigma_d, sigma_r, S, spacing):
    D, H, W = img.shape
    r = [int(np.ceil(2.5 * sigma_d / s)) for s in spacing]
    c = 4 * sigma_r
    out = np.zeros((D, H, W))
    for z in range(D):
        for y in range(H):
            for x in range(W):
                a, num, den = float(img[z, y, x]), 0.0, 0.0
                for oz in range(-r[2], r[2] + 1):
                    for oy in range(-r[1], r[1] + 1):
                        for ox in range(-r[0], r[0] + 1):
                            b = float(img[min(max(z + oz, 0), D - 1), min(max(y + oy, 0), H - 1), min(max(x + ox, 0), W - 1)])
                            delta = abs(b - a)
                            if delta < c:
                                i = int(np.floor(delta * (S / c)))
                                w = np.exp(-((ox * spacing[0]) ** 2 + (oy * spacing[1]) ** 2 + (oz * spacing[2]) ** 2) / (2 * sigma_d ** 2)) \
                                    * np.exp(-0.5 * (i * c / S) ** 2 / sigma_r ** 2)
                                num += w * b
                                den += w
                out[z, y, x] = num / den
    return out


@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), (1.0, 0.7, 2.5)])
def test_bilateral_reference_equals_a_per_voxel_loop(spacing):
    img = ic.lattice_image((4, 5, 6), 11).numpy()
    ref, guarded = ic.bilateral_reference(img[None, None], 0.6, 0.06, 50, spacing)
    np.testing.assert_allclose(ref[0, 0], _bilateral_loop(img, 0.6, 0.06, 50, spacing), rtol=0, atol=1e-14)
    assert not guarded.any()
    rr, wd, cutoff, table, scale = ops.bilateral_tables(0.6, 0.06, 50, spacing)      # the host helper builds what the definition says
    r2, wd2, c2, t2, s2 = ic.bilateral_setup(0.6, 0.06, 50, spacing)
    assert list(rr) == r2 and cutoff == c2 and scale == s2
    np.testing.assert_allclose(wd, wd2, rtol=1e-13)
    np.testing.assert_allclose(table, t2, rtol=1e-13)


@pytest.mark.parametrize('order', [1, 2, 3])
def test_bias_reference_equals_the_basis_matrix_einsum(order):
    D, H, W = 5, 7, 9
    mesh = (3, 2, 1)
    coef = ic.bias_coefficients(1, (D, H, W), mesh, order, 4)[0].astype(np.float64)
    Bz, By, Bx = (ic.bspline_basis(s, m, order) for s, m in ((D, mesh[2]), (H, mesh[1]), (W, mesh[0])))
    want = np.einsum('da,hb,wc,abc->dhw', Bz, By, Bx, coef)
    np.testing.assert_allclose(ic.bias_field_reference(coef, (D, H, W), order), want, rtol=0, atol=1e-15)
    np.testing.assert_allclose(Bz.sum(1), 1, atol=1e-15)                            # partition of unity
    start, w = T.bspline_support(np.arange(W), W, mesh[0], order)                   # ... and the package's support rule is the same one
    for i in range(W):
        np.testing.assert_allclose(Bx[i, start[i]:start[i] + order + 1], w[i], atol=1e-15)


def test_noise_reference_reproduces_the_hash_bit_for_bit():
    V = 4 * 5 * 6
    img, _ = oracle_datapath.synth_volume(2, (4, 5, 6), 4, 0, 0.0, seed=9, sample0=3)      # u = (bits >> 8) 2^-24 of stream 0
    for n in range(2):
        bits = ic.noise_bits(9, 3 + n, V, 0)
        np.testing.assert_array_equal((bits >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), img[n].reshape(-1))
    z = ic.noise_reference(9, 0, 1 << 16)
    assert np.isfinite(z).all() and abs(z.mean()) < 5 / 256 and abs(z.var() - 1) < 5 * np.sqrt(2.0 / (1 << 16))
    assert not np.array_equal(ic.noise_bits(9, 0, 64, ops.INTENSITY_STREAMS[0]), ic.noise_bits(9, 0, 64, ops.INTENSITY_STREAMS[1]))


def test_intensity_params_table():
    tab = ops.intensity_params([None, dict(gamma=1.5, invert=True, clamp=True), dict(gain=1.1, noise_std=0.02, seed=0xFFFFFFFF), {}], 4, seed=7, bias=True)
    F = ops.INTENSITY_FLAGS
    assert tab.dtype == np.uint32 and tab.shape == (4, 8)
    assert list(tab[:, 0]) == [0, F['bias'] | F['gamma'] | F['invert'] | F['clamp'], F['bias'] | F['linear'] | F['noise'], F['bias']]
    f = tab.view(np.float32)
    assert f[1, 1] == np.float32(1.5) and f[2, 2] == np.float32(1.1) and f[2, 3] == 0 and f[2, 4] == np.float32(0.02)
    assert tab[2, 5] == 0xFFFFFFFF and tab[1, 5] == 7
    assert not tab[0].any()
    with pytest.raises(ValueError):
        ops.intensity_params([{}], 2)


# ---- draw order and counts ---------------------------------------------------------------------------------------------------------------
def _state_after(fn):
    np.random.seed(123)
    fn()
    return np.random.get_state()[1].copy(), np.random.get_state()[2]


def _same_state(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0])


def test_filter_classes_draw_one_coin_per_sample():
    for cls in (T.GaussianBlur, T.BilateralFilter):
        np.random.seed(5)
        coins = cls(ratio=0.5).draw(6)
        np.random.seed(5)
        assert coins == [bool(np.random.rand(1)[0] < 0.5) for _ in range(6)] and True in coins and False in coins
        assert _same_state(_state_after(lambda: cls(ratio=0.5).draw(3)), _state_after(lambda: [np.random.rand(1) for _ in range(3)]))


def test_random_intensity_draw_order_counts_and_disabled_stages():
    size = (9, 8, 7)
    t = T.RandomIntensityTransform(gamma_invert_prob=0.5, offset=(-0.1, 0.1), bias_scale=0.4, bias_mesh=(2, 3, 1), bias_order=3)
    np.random.seed(42)
    got = t.draw(2, size)
    np.random.seed(42)
    for p in got:
        assert np.random.rand(1)[0] < 1.0
        assert p['gamma'] == np.random.uniform(0.7, 1.5)
        assert p['invert'] == bool(np.random.rand(1)[0] < 0.5)
        assert p['gain'] == np.random.uniform(0.75, 1.25)
        assert p['offset'] == np.random.uniform(-0.1, 0.1)
        assert p['noise_std'] == np.random.uniform(0.0, 0.05)
        np.testing.assert_array_equal(p['bias_coef'], np.random.normal(0, 0.2, 5 * 6 * 4).reshape(4, 6, 5))      # (gz, gy, gx), x fastest
        assert p['seed'] == int(np.random.randint(0, 2 ** 32, dtype=np.int64)) and 0 <= p['seed'] < 2 ** 32
        assert p['clamp'] is True
    # disabled stages draw nothing: everything off leaves the coin alone
    off = T.RandomIntensityTransform(gamma=None, gain=None, offset=None, noise_std=None, bias_scale=None)
    assert _same_state(_state_after(lambda: off.draw(3, size)), _state_after(lambda: [np.random.rand(1) for _ in range(3)]))
    np.random.seed(1)
    assert off.draw(1, size) == [{'clamp': True}]
    # the invert coin is drawn only when its probability is positive; no noise, no seed
    only_gamma = T.RandomIntensityTransform(gain=None, noise_std=None)
    assert _same_state(_state_after(lambda: only_gamma.draw(2, size)),
                       _state_after(lambda: [(np.random.rand(1), np.random.uniform(0.7, 1.5)) for _ in range(2)]))
    np.random.seed(3)
    assert set(only_gamma.draw(1, size)[0]) == {'clamp', 'gamma'}
    # a failed coin draws nothing more
    never = T.RandomIntensityTransform(ratio=0.0, bias_scale=0.3)
    assert _same_state(_state_after(lambda: never.draw(4, size)), _state_after(lambda: [np.random.rand(1) for _ in range(4)]))
    np.random.seed(0)
    assert never.draw(2, size) == [None, None]
    with pytest.raises(ValueError):
        T.RandomIntensityTransform(bias_order=4)


def test_all_coins_failing_returns_the_sample_object_without_touching_the_device():
    img = torch.zeros(2, 1, 3, 4, 5)                                                # a CPU tensor: any device call would raise
    for t in (T.GaussianBlur(ratio=0.0), T.BilateralFilter(ratio=0.0), T.RandomIntensityTransform(ratio=0.0)):
        sample = {'image': img, 'segmentation': torch.zeros(2, 3, 4, 5, dtype=torch.uint8)}
        out = t(sample)
        assert out is sample and out['image'] is img


def test_make_augmentation_accepts_the_new_names_and_rejects_unknown_ones():
    ts = T.make_augmentation([['intensity', {'bias_scale': 0.3}], ['blur', {}], ['bilateral', {'rangeSigma': 0.1}], ['rigid', {}]])
    assert [type(t) for t in ts] == [T.RandomIntensityTransform, T.GaussianBlur, T.BilateralFilter, T.RandomRigidTransform]
    assert ts[0].bias_scale == 0.3 and ts[2].rangeSigma == 0.1 and ts[2].domainSigma == 0.5 and ts[2].numberOfRangeGaussianSamples == 50
    assert (ts[1].variance, ts[1].maximumKernelWidth, ts[1].maximumError, ts[1].ratio) == (0.5, 1, 0.9, 1.0)
    assert set(T.AUGMENTATIONS) == {'rigid', 'bspline', 'blur', 'bilateral', 'intensity'}
    with pytest.raises(ValueError):
        T.make_augmentation([['contrast', {}]])


# ---- train_seg.py ------------------------------------------------------------------------------------------------------------------------
def test_train_seg_parses_the_intensity_flags(monkeypatch):
    import train_seg
    seen = []

    class Stop(Exception):
        pass

    def fake_experiment(cfg):
        seen.append(cfg)
        raise Stop()
    monkeypatch.setattr(train_seg, 'SegmentationExperiment', fake_experiment)
    argvs = ([], ['--aug-blur', '0.5'], ['--aug-bilateral', '0.5', '0.06'], ['--aug-intensity'], ['--aug-bias', '0.3', '--aug-noise', '0.1'],
             ['--aug-intensity', '--aug-blur', '2', '--aug-bspline', '4', '--aug-bilateral', '1', '0.1'])
    for argv in argvs:
        with pytest.raises(Stop):
            train_seg.main(argv)
    assert 'augment' not in seen[0]
    assert seen[1]['augment'] == [['blur', {'variance': 0.5, 'maximumKernelWidth': 32, 'maximumError': 0.01}]]
    assert seen[2]['augment'] == [['bilateral', {'domainSigma': 0.5, 'rangeSigma': 0.06}]]
    assert seen[3]['augment'] == [['intensity', {}]]
    assert seen[4]['augment'] == [['intensity', {'bias_scale': 0.3, 'noise_std': [0.0, 0.1]}]]
    assert [a[0] for a in seen[5]['augment']] == ['bspline', 'blur', 'bilateral', 'intensity']          # spatial first, then this order
    for cfg in seen:
        assert not any(k.startswith('aug_') for k in cfg)
        assert {k: v for k, v in cfg.items() if k != 'augment'} == seen[0]
        T.make_augmentation(cfg.get('augment'))                                     # every spelling constructs


def test_build_config_without_the_new_attributes_is_unchanged():
    import train_seg
    base = dict(device='0', debug=False, preload=False, num_samples=21, num_epochs=100, lr=1e-3, test_only=False,
                data_root='./data', log_root='./logs', shape=[64, 64, 64])
    c = train_seg.build_config(argparse.Namespace(**base))
    c2 = train_seg.build_config(argparse.Namespace(aug_blur=None, aug_bilateral=None, aug_intensity=False, aug_bias=None, aug_noise=None, **base))
    assert c2 == c and 'augment' not in c


# ---- guard-band facts, on the case lists the GPU file uses ---------------------------------------------------------------------------------
def test_lattice_cases_sit_away_from_every_bin_edge_and_from_the_cutoff():
    used = {case['pair'] for case in ic.bilateral_cases().values()}
    assert used == {0, 1}                                                            # at least a second (sigma_r, S) pair
    for k in used:
        sigma_r, S = ic.RANGE_PAIRS[k]
        d_int, d_cut = ic.lattice_min_distance(sigma_r, S)
        assert d_int >= 1.0 / 768 - 1e-12 and d_cut > 1e-3
        assert d_int > 100 * 4 * ic.U32 * S                                          # far outside the guard band: nothing is left out
    sigma_r, S = ic.RANGE_PAIRS[0]
    m = np.arange(0, 62)
    pos = m * 625.0 / 768.0                                                           # delta S / c = m / 256 * 50 / 0.24
    np.testing.assert_allclose(m / 256.0 * (S / (4 * sigma_r)), pos, rtol=1e-14)
    assert 61 / 256.0 < 4 * sigma_r < 62 / 256.0


@pytest.mark.parametrize('name', sorted(ic.bilateral_cases()))
def test_bilateral_cases_guard_share_and_radii(name):
    case = ic.bilateral_cases()[name]
    sigma_r, S = ic.RANGE_PAIRS[case['pair']]
    img, ref, guarded, tol, d32 = ic.bilateral_expected(name)
    r = ic.bilateral_setup(case['sigma_d'], sigma_r, S, case['spacing'])[0]
    assert max(r) <= ops.BILATERAL_MAX_RADIUS and S <= ops.BILATERAL_MAX_SAMPLES
    assert np.isfinite(ref).all() and tol < 4e-6
    if case['kind'] == 'lattice':
        assert not guarded.any()                                                     # on lattice cases no voxel is left out
        assert np.array_equal(img.numpy() * 256, np.round(img.numpy() * 256))
    else:
        assert 0 < guarded.mean() <= ic.GUARD_CAP                                    # the float64 reference's own count stays within the cap
    if name == 'aniso':
        assert len(set(r)) == 3
    if name == 'radius4':
        assert r == [4, 4, 4]
    if name == 'ragged':
        td, th, tw = ops.BILATERAL_TILE
        D, H, W = case['shape'][2:]
        assert D > td and H > th and W > tw and D % td and H % th and W % 64


def test_blur_and_pointwise_case_lists_cover_the_paths():
    b = ic.blur_shapes()
    assert b['ragged'][4] % 64 and b['ragged'][2] * b['ragged'][3] * b['ragged'][4] > 8 * ops.BLUR_BLOCK and b['long_w'][4] > ops.BLUR_BLOCK
    assert {s[k] for s in b.values() for k in (2, 3, 4)} >= {1, 2}
    p = ic.pointwise_shapes()
    assert p['ragged'][4] % 4 and p['vector'][4] % 4 == 0 and p['long_w'][4] > 4 * 256
    for order in (1, 2, 3):
        gx, gy, gz = (m + order for m in ic.max_grid_mesh(order))
        assert gx * gy * gz == 2048
