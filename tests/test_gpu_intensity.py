"""Intensity augmentation on the device (da_gauss_blur3d, da_bilateral3d, da_intensity_augment; lib/transforms.py:293-320 and the project's
own RandomIntensityTransform) against the float64 references of tests/intensity_cases.py, which restate the definitions of
include/deepatlas_hip.h independently of the host helpers.  ITK / SimpleITK are not available: agreement with ITK itself is not tested.
Tolerances: intensity_cases.tolerance (4 x the float32-torch distance, floor 4 float32 ulps of the data range); the bilateral filter's
continuous case leaves out the voxels inside the derived guard band (at most 2 %).

Mutants (each kernel broken once in a scratch copy of intensity.hip and run against this file on the device; the tests that then failed):
  * blur: the W and H passes read each other's taps                   -> 11: test_blur_matches_reference[axes-*] (all 10), the mixed-apply batch
  * blur: the upper clamp is len - 2 instead of len - 1 (wrong face)  -> 44: test_blur_matches_reference (all 40), the mixed-apply batch, the identity
                                                                         taps, both NaN-box cases
  * bilateral: table index + 1                                        -> 15: test_bilateral_matches_reference (all 13), the mixed-apply batch, the NaN test
  * bilateral: the `delta < cutoff` test dropped                      -> 9: test_bilateral_matches_reference (the 6 cases whose deltas reach the cutoff), the
                                                                         mixed-apply batch, constant volume / step edge, the NaN test
  * pointwise: the linear stage runs before gamma                     -> 12: test_pointwise_stages[all-*] (all 11), the mixed batch
"""
import argparse

import numpy as np
import pytest
import torch

import intensity_cases as ic
from deepatlas_amd import _native as nat
from deepatlas_amd import ops
from deepatlas_amd.lib import transforms as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _close(got, ref, tol, keep=None):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    if keep is not None:
        err = err[keep]
    worst = float(err.max()) if err.size else 0.0
    print('max |device - float64| %.3e, bound %.3e' % (worst, tol))
    assert np.isfinite(got[keep] if keep is not None else got).all()
    assert worst <= tol, (worst, tol)


# ---- Gaussian blur ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sname', sorted(ic.blur_shapes()))
@pytest.mark.parametrize('tname', sorted(ic.blur_taps()))
def test_blur_matches_reference(tname, sname):
    taps, shape = ic.blur_taps()[tname], ic.blur_shapes()[sname]
    img = ic.rand_image(shape, 1)
    ref = ic.blur_reference(img.numpy(), taps)
    tol, _ = ic.tolerance(ref, ic.blur_torch32(img, taps))
    out = ops.gaussian_blur(img.to(DEV), taps)
    assert out.shape == img.shape and out.dtype == torch.float32
    _close(out, ref, tol)
    single = ops.gaussian_blur(img[0].to(DEV), taps)                                    # C x D x H x W in, C x D x H x W out
    assert single.dim() == 4 and torch.equal(single, out[0])


def test_blur_batch_with_mixed_apply_flags_and_repeats():
    taps = ic.blur_taps()['axes']
    img = ic.rand_image((3, 1, 5, 9, 33), 2)
    ref = ic.blur_reference(img.numpy(), taps)
    tol, _ = ic.tolerance(ref, ic.blur_torch32(img, taps))
    dimg = img.to(DEV)
    out = ops.gaussian_blur(dimg, taps, apply=[True, False, True])
    assert torch.equal(out[1], dimg[1])                                                 # copied through bit for bit
    _close(out[[0, 2]], ref[[0, 2]], tol)
    assert out.data_ptr() != dimg.data_ptr() and torch.equal(dimg.cpu(), img)           # a fresh tensor, the input untouched
    for _ in range(2):
        assert torch.equal(ops.gaussian_blur(dimg, taps, apply=[True, False, True]), out)


def test_blur_identity_taps_reproduce_the_input_bit_for_bit():
    img = ic.rand_image(ic.blur_shapes()['ragged'], 3).to(DEV)
    assert torch.equal(ops.gaussian_blur(img, [0.0, 1.0, 0.0]), img)
    assert torch.equal(ops.gaussian_blur(img, T.discrete_gaussian_taps(0, 1, 0.9)), img)


@pytest.mark.parametrize('radius', [1, 3])
def test_blur_nan_poisons_exactly_its_box(radius):
    shape = ic.blur_shapes()['ragged']
    img = ic.rand_image(shape, 4)
    D, H, W = shape[2:]
    spots = [(4, 5, 30), (0, 0, 0), (D - 1, H - 2, W - 1)]
    want = np.zeros(shape, dtype=bool)
    for (z, y, x) in spots:
        img[0, 0, z, y, x] = float('nan')
        want[0, 0, max(z - radius, 0):z + radius + 1, max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1] = True
    out = ops.gaussian_blur(img.to(DEV), ic.gauss_taps(1.0, radius))
    assert np.array_equal(torch.isnan(out).cpu().numpy(), want)


def test_blur_declines():
    img = torch.zeros(1, 1, 2, 2, 2, device=DEV)
    with pytest.raises(nat.NativeError, match='DA_ERR_UNSUPPORTED'):
        ops.gaussian_blur(img, np.ones(2 * ops.BLUR_MAX_RADIUS + 3) / (2 * ops.BLUR_MAX_RADIUS + 3))
    flags = torch.ones(1, dtype=torch.int32, device=DEV)
    taps = torch.ones(3, 3, device=DEV)
    a, b, c = (torch.zeros(8, device=DEV) for _ in range(3))
    with pytest.raises(nat.NativeError, match='DA_ERR_UNSUPPORTED'):                    # >= 2^31 voxels per sample: declined before any launch
        nat.call('da_gauss_blur3d', nat.ptr(a), nat.ptr(b), nat.ptr(c), nat.ptr(taps), 1, nat.ptr(flags), 1, 1, 2048, 1024, 1024, nat.stream())
    with pytest.raises(ValueError):
        ops.gaussian_blur(img, [0.5, 0.5])


# ---- bilateral filter --------------------------------------------------------------------------------------------------------------------
def _bilateral(img, case, **kw):
    sigma_r, S = ic.RANGE_PAIRS[case['pair']]
    return ops.bilateral_filter(img, case['sigma_d'], sigma_r, S, case['spacing'], **kw)


@pytest.mark.parametrize('name', sorted(ic.bilateral_cases()))
def test_bilateral_matches_reference(name):
    case = ic.bilateral_cases()[name]
    img, ref, guarded, tol, _ = ic.bilateral_expected(name)
    out = _bilateral(img.to(DEV), case)
    assert out.shape == img.shape
    if case['kind'] == 'lattice':
        assert not guarded.any()
        _close(out, ref, tol)
    else:
        assert guarded.mean() <= ic.GUARD_CAP
        print('left out %.4f of the voxels' % guarded.mean())
        _close(out, ref, tol, keep=~guarded)
    assert torch.equal(_bilateral(img.to(DEV), case), out)                              # bit-identical repeat


def test_bilateral_batch_with_mixed_apply_flags():
    case = dict(sigma_d=0.5, pair=0, spacing=(1.0, 1.0, 1.0))
    img = ic.lattice_image((3, 1, 5, 9, 33), 7)
    sigma_r, S = ic.RANGE_PAIRS[0]
    ref, guarded = ic.bilateral_reference(img.numpy(), 0.5, sigma_r, S)
    tol, _ = ic.tolerance(ref, ic.bilateral_torch32(img, 0.5, sigma_r, S))
    assert not guarded.any()
    dimg = img.to(DEV)
    out = _bilateral(dimg, case, apply=[False, True, True])
    assert torch.equal(out[0], dimg[0])
    _close(out[1:], ref[1:], tol)
    assert torch.equal(_bilateral(dimg[1], case), out[1])                               # C x D x H x W in and out


def test_bilateral_constant_volume_and_step_edge_are_exact():
    case = dict(sigma_d=0.5, pair=0, spacing=(1.0, 1.0, 1.0))
    td, th, tw = ops.BILATERAL_TILE
    const = torch.full((1, 1, td + 1, th + 1, tw + 3), 0.3137, device=DEV)
    assert torch.equal(_bilateral(const, case), const)                                  # exact (the sums run over b - a = 0), not merely to 1 ulp
    step = torch.full((1, 1, td + 1, th + 1, tw + 3), 0.2, device=DEV)
    step[..., (tw + 3) // 2:] = 0.7                                                     # height 0.5 > cutoff 0.24: nothing crosses the edge
    step[:, :, td // 2:, :, :3] = 0.95
    assert torch.equal(_bilateral(step, case), step)


def test_bilateral_nan_centre_and_nan_neighbour():
    case = dict(sigma_d=0.5, pair=0, spacing=(1.0, 1.0, 1.0))
    img = ic.lattice_image((1, 1, 6, 9, 35), 8)
    img[0, 0, 2, 4, 17] = float('nan')
    img[0, 0, 0, 0, 0] = float('nan')
    sigma_r, S = ic.RANGE_PAIRS[0]
    ref, _ = ic.bilateral_reference(img.numpy(), 0.5, sigma_r, S)
    out = _bilateral(img.to(DEV), case)
    nan = torch.isnan(out).cpu().numpy()
    assert np.array_equal(nan, np.isnan(img.numpy())) and nan.sum() == 2                # NaN for those voxels alone
    tol, _ = ic.tolerance(ref[~nan], ic.bilateral_torch32(img, 0.5, sigma_r, S)[~nan])
    _close(out, ref, tol, keep=~nan)                                                    # the NaN neighbour is ignored


def test_bilateral_declines():
    img = torch.zeros(1, 1, 4, 4, 4, device=DEV)
    with pytest.raises(nat.NativeError, match='DA_ERR_UNSUPPORTED'):
        ops.bilateral_filter(img, 1.7, 0.06)                                            # radius 5
    with pytest.raises(nat.NativeError, match='DA_ERR_UNSUPPORTED'):
        ops.bilateral_filter(img, 0.5, 0.06, spacing=(1.0, 1.0, 0.2))                   # radius 7 along z alone
    with pytest.raises(nat.NativeError, match='DA_ERR_UNSUPPORTED'):
        ops.bilateral_filter(img, 0.5, 0.06, n_samples=ops.BILATERAL_MAX_SAMPLES + 1)
    assert ops.bilateral_filter(img, 1.5, 0.06, n_samples=ops.BILATERAL_MAX_SAMPLES).shape == img.shape       # the limits themselves work


# ---- fused pointwise pass ------------------------------------------------------------------------------------------------------------------
def _pointwise_case(stage, shape, seed=5, sample0=0, order=2):
    p = dict(ic.STAGES[stage])
    img = ic.rand_image(shape, seed) * 1.2 - 0.1                                        # a little outside [0, 1]: the clamps matter
    with_bias = p.get('bias') and min(shape[2:]) >= 2
    coef = ic.bias_coefficients(shape[0], shape[2:], (2, 3, 1), order, seed) if with_bias else None
    params = [p] * shape[0]
    ref = ic.intensity_reference(img.numpy(), params, coef, order, sample0)
    tol, _ = ic.tolerance(ref, ic.intensity_torch32(img, params, coef, order, sample0))
    return img, params, coef, ref, tol


@pytest.mark.parametrize('stage,sname', [(st, sn) for st in sorted(ic.STAGES) for sn in (['ragged', 'vector'] if st != 'all' else sorted(ic.pointwise_shapes()))])
def test_pointwise_stages(stage, sname):
    shape = ic.pointwise_shapes()[sname]
    img, params, coef, ref, tol = _pointwise_case(stage, shape)
    out = ops.intensity_augment(img.to(DEV), params, coef, 2)
    assert out.shape == img.shape
    _close(out, ref, tol)
    if stage == 'clamp':
        assert float(out.min()) == 0.0 and float(out.max()) == 1.0
    if stage == 'all':
        assert torch.equal(ops.intensity_augment(img.to(DEV), params, coef, 2), out)    # the same (seed, sample0) repeats bit for bit
        assert torch.equal(ops.intensity_augment(img[0].to(DEV), params[0], None if coef is None else coef[0], 2), out[0])


def test_pointwise_all_off_copies_bit_for_bit_and_mixed_batch():
    shape = (3, 2, 4, 6, 10)
    img = ic.rand_image(shape, 6) * 1.2 - 0.1
    dimg = img.to(DEV)
    for params in ([{}] * 3, [None] * 3, {}):
        out = ops.intensity_augment(dimg, params)
        assert torch.equal(out, dimg) and out.data_ptr() != dimg.data_ptr()
    coef = ic.bias_coefficients(3, shape[2:], (1, 2, 3), 3, 1)
    params = [ic.STAGES['all'], None, dict(ic.STAGES['noise'], bias=False)]
    ref = ic.intensity_reference(img.numpy(), params, coef, 3, sample0=4)
    tol, _ = ic.tolerance(ref, ic.intensity_torch32(img, params, coef, 3, sample0=4))
    out = ops.intensity_augment(dimg, params, coef, 3, sample0=4)
    assert torch.equal(out[1], dimg[1])
    _close(out, ref, tol)


def test_pointwise_noise_statistics_seeds_and_sample0():
    img = torch.zeros(1, 1, 32, 32, 64, device=DEV)
    E = img.numel()
    z = ops.intensity_augment(img, dict(noise_std=1.0), seed=9)
    assert torch.isfinite(z).all()
    mean, var = float(z.double().mean()), float(z.double().var())
    print('noise mean %.5f var %.5f over %d' % (mean, var, E))
    assert abs(mean) < 5 / np.sqrt(E) and abs(var - 1) < 5 * np.sqrt(2.0 / E)           # 5 standard errors
    np.testing.assert_allclose(z.cpu().numpy().reshape(-1), ic.noise_reference(9, 0, E), atol=2e-5)
    assert torch.equal(ops.intensity_augment(img, dict(noise_std=1.0), seed=9), z)
    other = ops.intensity_augment(img, dict(noise_std=1.0), seed=9, sample0=1)
    assert not torch.equal(other, z)
    two = ops.intensity_augment(torch.zeros(2, 1, 32, 32, 64, device=DEV), dict(noise_std=1.0), seed=9)
    assert torch.equal(two[0], z[0]) and torch.equal(two[1], other[0])                  # sample n of a batch = sample0 + n
    assert not torch.equal(ops.intensity_augment(img, dict(noise_std=1.0, seed=99), seed=9), z)       # a per-sample seed overrides


@pytest.mark.parametrize('order', [1, 2, 3])
def test_pointwise_bias_orders_at_the_largest_grid(order):
    shape = (1, 1, 6, 7, 9)
    mesh = ic.max_grid_mesh(order)
    img = ic.rand_image(shape, 9)
    coef = ic.bias_coefficients(1, shape[2:], mesh, order, 10)
    assert coef[0].size == 2048
    params = [dict(bias=True)]
    ref = ic.intensity_reference(img.numpy(), params, coef, order)
    tol, _ = ic.tolerance(ref, ic.intensity_torch32(img, params, coef, order))
    _close(ops.intensity_augment(img.to(DEV), params, coef, order), ref, tol)
    beyond = ic.bias_coefficients(1, shape[2:], (mesh[0] + 1, mesh[1], mesh[2]), order, 10)
    with pytest.raises(nat.NativeError, match='DA_ERR_UNSUPPORTED'):
        ops.intensity_augment(img.to(DEV), params, beyond, order)


# ---- classes and experiment ------------------------------------------------------------------------------------------------------------------
def _batch(seed=0, N=3, shape=(6, 9, 20)):
    img = ic.rand_image((N, 1) + shape, seed).to(DEV)
    seg = torch.randint(0, 4, (N,) + shape, generator=torch.Generator().manual_seed(seed)).to(torch.uint8).to(DEV)
    return img, seg


def test_classes_equal_the_ops_called_with_their_own_draws():
    img, seg = _batch()
    D, H, W = img.shape[-3:]
    blur = T.GaussianBlur(variance=1.5, maximumKernelWidth=32, maximumError=0.01, ratio=0.6)
    bil = T.BilateralFilter(domainSigma=0.5, rangeSigma=0.1, numberOfRangeGaussianSamples=40, ratio=0.6)
    inten = T.RandomIntensityTransform(ratio=0.7, gamma_invert_prob=0.5, offset=(-0.05, 0.05), bias_scale=0.4)
    for seed in (0, 1, 2, 3):                                                           # (several seeds: both coin outcomes occur)
        np.random.seed(seed)
        coins = blur.draw(3)
        np.random.seed(seed)
        sample = {'image': img, 'segmentation': seg}
        out = blur(sample)
        assert out['segmentation'] is seg
        assert torch.equal(out['image'], ops.gaussian_blur(img, blur.taps(), apply=coins) if any(coins) else img)

        np.random.seed(seed)
        coins = bil.draw(3)
        np.random.seed(seed)
        out = bil({'image': img, 'segmentation': seg, 'spacing': (1.0, 0.8, 1.2)})
        assert out['segmentation'] is seg
        assert torch.equal(out['image'], ops.bilateral_filter(img, 0.5, 0.1, 40, (1.0, 0.8, 1.2), apply=coins) if any(coins) else img)

        np.random.seed(seed)
        params = inten.draw(3, (W, H, D))
        np.random.seed(seed)
        out = inten({'image': img, 'segmentation': seg})
        assert out['segmentation'] is seg
        coef = np.stack([np.zeros((4, 4, 4)) if p is None else p['bias_coef'] for p in params])
        assert torch.equal(out['image'], ops.intensity_augment(img, params, coef, 2) if any(p is not None for p in params) else img)
    np.random.seed(0)
    single = inten({'image': img[0], 'segmentation': seg[0]})                           # a single sample: C x D x H x W
    assert single['image'].shape == img[0].shape and single['segmentation'] is not None


def test_all_coins_failing_makes_no_device_call():
    img, seg = _batch()
    prev, nat.profiler = nat.profiler, nat.CallProfiler()
    try:
        before = nat.n_calls
        for t in (T.GaussianBlur(ratio=0.0), T.BilateralFilter(ratio=0.0), T.RandomIntensityTransform(ratio=0.0, bias_scale=0.3)):
            sample = {'image': img, 'segmentation': seg}
            out = t(sample)
            assert out is sample and out['image'] is img and out['segmentation'] is seg
        assert nat.n_calls == before and not nat.profiler.records
        T.GaussianBlur()({'image': img, 'segmentation': seg})
        assert [k[0] for k in nat.profiler.records] == ['da_gauss_blur3d']              # (the profiler does see a call when one is made)
    finally:
        nat.profiler = prev


def _first_epoch(tmp_path, **extra):
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                            data_root='./data', log_root=str(tmp_path), shape=[16, 24, 32])
    cfg = train_seg.build_config(ns)
    cfg.update(extra)
    exp = SegmentationExperiment(cfg)
    exp.setup_train()
    exp.initialize_model(exp.model, exp.optimizer, '')
    losses = []
    step = exp.train_step

    def recording_step(images, truths):
        loss, out = step(images, truths)
        losses.append(loss.item())
        return loss, out
    exp.train_step = recording_step
    exp.current_epoch = 1
    exp.train_one_epoch()
    return losses


def test_segmentation_experiment_with_and_without_the_intensity_transforms(tmp_path):
    plain = _first_epoch(tmp_path / 'a')
    none = _first_epoch(tmp_path / 'b', augment=None)
    aug = _first_epoch(tmp_path / 'c', augment=[['intensity', {}], ['blur', {}], ['bilateral', {}]])
    assert len(plain) == len(none) == len(aug) == 2 and all(np.isfinite(aug))
    assert plain[0] == none[0]                                                          # without the key: the first step's loss, bit for bit
    assert aug[0] != plain[0]
