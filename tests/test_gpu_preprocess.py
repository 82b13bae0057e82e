"""GPU: the preprocessing kernels (csrc/preprocess.hip) against numpy on the same tables / values, the transforms on a sample dict, and the
three experiments end to end on tiny NIfTI files written at test time."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NP_OF = {'f32': np.float32, 'u8': np.uint8, 'i16': np.int16, 'i32': np.int32, 'f64': np.float64}


def volume(shape, kind, seed):
    rng = np.random.RandomState(seed)
    if kind in ('f32', 'f64'):
        return (rng.standard_normal(shape) * 100).astype(NP_OF[kind])
    hi = {'u8': 255, 'i16': 32767, 'i32': 2 ** 31 - 1}[kind]
    lo = 0 if kind == 'u8' else -hi
    return rng.randint(lo, hi, size=shape, dtype=np.int64).astype(NP_OF[kind])


def tables(ops, shape_in, shape_out, scale, offset, interpolator):
    return [ops.resample_axis_table(n, m, s, o, interpolator) for n, m, s, o in zip(shape_in, shape_out, scale, offset)]


def ref_nearest(x, tabs, default):
    (ld, _, _, ind), (lh, _, _, inh), (lw, _, _, inw) = tabs
    out = x[:, ld][:, :, lh][:, :, :, lw].copy()
    inside = ind[:, None, None] & inh[None, :, None] & inw[None, None, :]
    out[:, ~inside] = default
    return out


def ref_linear(x, tabs, default, dtype):
    (ld, hd, fd, ind), (lh, hh, fh, inh), (lw, hw, fw, inw) = tabs
    X = x.astype(dtype)
    a, b = X[..., lw], X[..., hw]
    X = fw.astype(dtype) * (b - a) + a
    a, b = X[:, :, lh], X[:, :, hh]
    X = fh.astype(dtype)[:, None] * (b - a) + a
    a, b = X[:, ld], X[:, hd]
    X = fd.astype(dtype)[:, None, None] * (b - a) + a
    inside = ind[:, None, None] & inh[None, :, None] & inw[None, None, :]
    X[:, ~inside] = default
    return X


def out_size(n, scale):
    return max(1, int(math.ceil(n / abs(scale)))) + (2 if abs(scale) < 1 else 0)          # (+2: some outputs of an up-sampling fall outside)


RESAMPLE_CASES = [((1, 1, 1), (1.0, 1.0, 1.0)), ((1, 1, 1), (0.5, 0.25, 1.5)), ((5, 6, 7), (0.5, 1.5, 2.0 / 3.0)), ((5, 6, 7), (0.25, 1.0, -1.0)),
                  ((5, 6, 7), (-1.0, 2.0 / 3.0, 0.5)), ((3, 4, 63), (1.0, 1.0, 1.5)), ((3, 4, 64), (1.5, 0.5, 2.0 / 3.0)), ((3, 4, 65), (1.0, -1.0, 0.25)),
                  ((3, 4, 130), (2.0 / 3.0, 1.0, 0.5))]


def geometry(shape, scale):
    size = tuple(out_size(n, s) for n, s in zip(shape, scale))
    offset = tuple(float(n - 1) if s < 0 else 0.0 for n, s in zip(shape, scale))
    return size, offset


@pytest.mark.parametrize('shape,scale', RESAMPLE_CASES)
def test_resample_nearest_equals_numpy_indexing(shape, scale):
    from deepatlas_amd import ops
    size, offset = geometry(shape, scale)
    tabs = tables(ops, shape, size, scale, offset, 'nearest')
    for k, (kind, C, default) in enumerate((('f32', 1, 0), ('u8', 2, 7), ('i16', 1, -3), ('i32', 2, 123456), ('f64', 1, 0.5))):
        x = volume((C,) + shape, kind, seed=k)
        got = ops.resample_volume(torch.from_numpy(x).to(DEV), size, scale, offset, 'nearest', default)
        assert got.dtype == torch.from_numpy(x).dtype and tuple(got.shape) == (C,) + size
        want = ref_nearest(x, tabs, default)
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8)), (kind, shape, scale)
    x = volume(shape, 'i16', seed=9)                                                           # D x H x W in, D x H x W out
    got = ops.resample_volume(torch.from_numpy(x).to(DEV), size, scale, offset, 'nearest', 0)
    assert np.array_equal(got.cpu().numpy(), ref_nearest(x[None], tabs, 0)[0])


def test_resample_identity_and_double_flip_restore_the_bits():
    from deepatlas_amd import ops
    for kind in ('f32', 'u8', 'i16', 'i32'):
        x = volume((2, 5, 6, 67), kind, seed=3)
        if kind == 'f32':
            x.reshape(-1)[:4] = [np.nan, -0.0, np.inf, 1e-42]
        t = torch.from_numpy(x).to(DEV)
        same = ops.resample_volume(t, (5, 6, 67), (1, 1, 1), (0, 0, 0), 'nearest')
        assert np.array_equal(same.cpu().numpy().view(np.uint8), x.view(np.uint8))
        flip = ops.resample_volume(t, (5, 6, 67), (-1, -1, -1), (4, 5, 66), 'nearest')
        assert np.array_equal(flip.cpu().numpy().view(np.uint8), np.ascontiguousarray(x[:, ::-1, ::-1, ::-1]).view(np.uint8))
        back = ops.resample_volume(flip, (5, 6, 67), (-1, -1, -1), (4, 5, 66), 'nearest')
        assert np.array_equal(back.cpu().numpy().view(np.uint8), x.view(np.uint8))
    x = volume((1, 5, 6, 67), 'f32', seed=4)
    lin = ops.resample_volume(torch.from_numpy(x).to(DEV), (5, 6, 67), (1, 1, 1), (0, 0, 0), 'linear')          # every fraction 0: exact
    assert np.array_equal(lin.cpu().numpy(), x)
    lin = ops.resample_volume(torch.from_numpy(x).to(DEV), (5, 6, 67), (1, -1, 1), (0, 5, 0), 'linear')
    assert np.array_equal(lin.cpu().numpy(), x[:, :, ::-1])
    x16 = volume((1, 5, 6, 67), 'i16', seed=5)
    lin = ops.resample_volume(torch.from_numpy(x16).to(DEV), (3, 3, 34), (2, 2, 2), (0, 0, 0), 'linear')        # integer positions of an i16 source
    assert lin.dtype == torch.float32 and np.array_equal(lin.cpu().numpy(), x16[:, ::2, ::2, ::2].astype(np.float32))


@pytest.mark.parametrize('shape,scale', RESAMPLE_CASES)
def test_resample_linear_against_float64(shape, scale):
    """Against the float64 evaluation of the same taps and fractions; tolerance 4 x the distance of numpy's float32 evaluation of the formula from the
    float64 one on the case, never below 2^-24 max|x|."""
    from deepatlas_amd import ops
    size, offset = geometry(shape, scale)
    tabs = tables(ops, shape, size, scale, offset, 'linear')
    for k, (kind, C, default) in enumerate((('f32', 2, 0.25), ('i16', 1, -1), ('u8', 1, 0), ('f64', 1, 0), ('i32', 1, 0))):
        x = volume((C,) + shape, kind, seed=10 + k)
        if kind == 'i32':
            x = (x % 100000).astype(np.int32)                                                      # (integers a float32 holds exactly)
        xf = x.astype(np.float32)                                                                  # the kernel converts to float32 first
        got = ops.resample_volume(torch.from_numpy(x).to(DEV), size, scale, offset, 'linear', default).cpu().numpy().astype(np.float64)
        r64, r32 = ref_linear(xf, tabs, default, np.float64), ref_linear(xf, tabs, default, np.float32)
        floor = float(np.abs(r32.astype(np.float64) - r64).max())
        tol = max(4 * floor, 2.0 ** -24 * float(np.abs(xf).max()))
        err = float(np.abs(got - r64).max())
        print('linear %s %s %s: err %.3g, float32 numpy %.3g, tol %.3g' % (kind, shape, scale, err, floor, tol))
        assert err <= tol, (kind, shape, scale)


# ---- moments ---------------------------------------------------------------------------------------------------------------------------
def fsum_moments(x):
    vals = [float(v) for v in np.asarray(x, dtype=np.float64).reshape(-1) if math.isfinite(v)]
    n = len(vals)
    mean = math.fsum(vals) / n if n else 0.0
    var = math.fsum((v - mean) ** 2 for v in vals) / (n - 1) if n > 1 else 0.0
    return n, mean, var


def moment_cases():
    rng = np.random.RandomState(5)
    cases = [('n%d' % n, (rng.standard_normal(n) * 50 + 10).astype(np.float32)) for n in (1, 2, 255, 256, 257)]
    cases.append(('ragged', (rng.standard_normal((7, 33, 129)) * 3).astype(np.float32)))
    cases.append(('mean1000', (1000.0 + 0.01 * rng.standard_normal((6, 31, 65))).astype(np.float32)))
    x = (rng.standard_normal((5, 9, 70)) * 2).astype(np.float32)
    x.reshape(-1)[::13] = np.nan
    x.reshape(-1)[5] = np.inf
    cases.append(('nan', x))
    cases.append(('i16', volume((4, 9, 70), 'i16', 6)))
    cases.append(('u8', volume((4, 9, 70), 'u8', 7)))
    cases.append(('f64', (1e6 + rng.standard_normal((3, 9, 70))).astype(np.float64)))
    return cases


@pytest.mark.parametrize('name,x', moment_cases(), ids=[c[0] for c in moment_cases()])
def test_volume_moments_against_fsum(name, x):
    from deepatlas_amd import ops
    t = torch.from_numpy(x).to(DEV)
    t = t if t.dim() >= 3 else t.reshape(1, 1, -1)
    c, m, v = ops.volume_moments(t)
    n, mean, var = fsum_moments(x)
    print('%s: count %d, mean %.17g (fsum %.17g), var %.17g (fsum %.17g)' % (name, c, m, mean, v, var))
    assert c == n
    assert abs(m - mean) <= 1e-12 * abs(mean) and abs(v - var) <= 1e-12 * abs(var)
    assert ops.volume_moments(t) == (c, m, v)                                                     # bit-identical from run to run
    if name == 'mean1000':
        assert 0.8e-4 < v < 1.2e-4 and abs(m - 1000.0) < 1e-3                                       # sigma 0.01 on a mean of 1000 survives
    if name == 'n1':
        assert v == 0.0


def test_volume_moments_without_finite_voxels():
    from deepatlas_amd import ops
    assert ops.volume_moments(torch.full((1, 2, 3), float('nan'), device=DEV)) == (0.0, 0.0, 0.0)


# ---- percentiles -----------------------------------------------------------------------------------------------------------------------
def percentile_cases():
    rng = np.random.RandomState(8)
    cases = [('n%d' % n, (rng.standard_normal(n) * 30).astype(np.float32)) for n in (1, 2, 2047, 2048, 2049)]
    x = (rng.standard_normal(5000) * 2).astype(np.float32)
    x[::7] = 0.0
    x[3::7] = -0.0
    cases.append(('signs_zeros', x))
    cases.append(('duplicates', rng.randint(-3, 4, size=6000).astype(np.float32)))
    cases.append(('all_equal', np.full(3000, -2.5, dtype=np.float32)))
    cases.append(('shared_top_digits', (np.uint32(0x3F800000) + rng.randint(0, 1024, size=4000).astype(np.uint32)).view(np.float32)))
    cases.append(('shared_top_digits_negative', (np.uint32(0xC2000000) + rng.randint(0, 1024, size=4000).astype(np.uint32)).view(np.float32)))
    cases.append(('i16', volume((3, 20, 70), 'i16', 9)))
    cases.append(('u8', volume((3, 20, 70), 'u8', 10)))
    x = (rng.standard_normal(4100) * 5).astype(np.float32)
    x[::11] = np.nan
    cases.append(('nan', x))
    return cases


@pytest.mark.parametrize('name,x', percentile_cases(), ids=[c[0] for c in percentile_cases()])
def test_volume_percentiles_are_exact_order_statistics(name, x):
    from deepatlas_amd import ops
    t = torch.from_numpy(x).to(DEV)
    t = t if t.dim() >= 3 else t.reshape(1, 1, -1)
    vals = x.astype(np.float32).reshape(-1)
    vals = vals[~np.isnan(vals)]
    n = vals.size
    for pair in ((0.0, 100.0), (0.5, 99.5), (50.0,), (99.5, 0.5)):
        res = ops.volume_order_statistics(t, pair)
        assert res['count'] == n and res['nan_count'] == x.size - n
        for p, got, (s_lo, s_hi) in zip(pair, res['percentiles'], res['order_statistics']):
            rank = p / 100.0 * (n - 1)
            k = int(math.floor(rank))
            k1 = min(k + 1, n - 1)
            assert s_lo == float(np.partition(vals, k)[k]) and s_hi == float(np.partition(vals, k1)[k1]), (name, p)
            with np.errstate(invalid='ignore'):
                want = float(np.percentile(vals.astype(np.float64), p))
            print('%s p=%s: %.17g (numpy %.17g)' % (name, p, got, want))
            assert got == want or abs(got - want) <= 1e-12 * abs(want), (name, p)
        assert ops.volume_order_statistics(t, pair) == res                                        # repeats are bit-identical
        assert ops.volume_percentiles(t, pair) == tuple(res['percentiles'])


def test_volume_percentiles_of_nothing():
    from deepatlas_amd import ops
    res = ops.volume_order_statistics(torch.full((1, 1, 9), float('nan'), device=DEV), (50.0,))
    assert res['count'] == 0 and res['nan_count'] == 9 and math.isnan(res['percentiles'][0])


# ---- intensity, look-up table ---------------------------------------------------------------------------------------------------------------
def test_affine_intensity_against_float64():
    """(x - a) / b: one subtraction and one division, each rounded once -> 4 * 2^-24 max(1, |y|) against float64 with a, b rounded to float32."""
    from deepatlas_amd import ops
    for k, kind in enumerate(('f32', 'f64', 'i16', 'u8', 'i32')):
        x = volume((2, 3, 5, 67), kind, seed=20 + k)
        if kind == 'i32':
            x = (x % 1000000).astype(np.int32)
        for a, b, clamp in ((12.3, 457.9, False), (-3.0, 0.37, True), (5.0, -40.0, True), (1.5, 0.0, False), (1.5, 0.0, True)):
            got = ops.affine_intensity(torch.from_numpy(x).to(DEV), a, b, clamp=clamp)
            assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
            got = got.cpu().numpy().astype(np.float64)
            if b == 0.0:
                assert not got.any()
                continue
            y = (x.astype(np.float32).astype(np.float64) - float(np.float32(a))) / float(np.float32(b))
            tol = 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(y))
            if clamp:
                y = np.clip(y, 0.0, 1.0)
                assert got.min() >= 0.0 and got.max() <= 1.0
            err = np.abs(got - y)
            print('affine %s a=%s b=%s clamp=%s: worst err / tol %.3g' % (kind, a, b, clamp, float((err / tol).max())))
            assert (err <= tol).all(), (kind, a, b)


def test_label_lut_is_exact():
    from deepatlas_amd import ops
    rng = np.random.RandomState(3)
    lut = rng.randint(0, 200, size=100)
    x8 = rng.randint(0, 256, size=(3, 5, 67)).astype(np.uint8)
    got = ops.label_lut(torch.from_numpy(x8).to(DEV), lut)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), np.where(x8 < 100, lut[np.minimum(x8, 99)], 0).astype(np.uint8))
    x32 = rng.randint(-5, 70000, size=(2, 3, 5, 67)).astype(np.int32)
    big = rng.randint(0, 2 ** 31 - 1, size=65536)
    got = ops.label_lut(torch.from_numpy(x32).to(DEV), big)
    ok = (x32 >= 0) & (x32 < 65536)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), np.where(ok, big[np.clip(x32, 0, 65535)], 0).astype(np.int32))


# ---- transforms on a sample dict ---------------------------------------------------------------------------------------------------------------
def test_transforms_on_a_sample_dict():
    from deepatlas_amd.lib import transforms as T
    rng = np.random.RandomState(1)
    img = rng.randint(0, 3000, size=(4, 6, 10)).astype(np.int16)
    seg = rng.randint(0, 6, size=(4, 6, 10)).astype(np.uint8)
    s = T.Resample((1.0, 1.0, 1.0))({'image': img, 'segmentation': seg, 'name': 'a', 'spacing': (1.0, 1.0, 2.0)})
    assert s['spacing'] == (1.0, 1.0, 1.0) and tuple(s['image'].shape) == (8, 6, 10) and s['image'].is_cuda and s['image'].dtype == torch.int16
    idx = np.array([0, 1, 1, 2, 2, 3, 3, 3])                      # q = 0, .5, 1, ...: ties go up; q = 3.5 is outside
    want = img[idx].copy()
    want[7] = 0
    assert np.array_equal(s['image'].cpu().numpy(), want)
    wseg = seg[idx].copy()
    wseg[7] = 0
    assert s['segmentation'].dtype == torch.uint8 and np.array_equal(s['segmentation'].cpu().numpy(), wseg)
    s = T.Resample(2.0, interpolator='linear')({'image': torch.from_numpy(img[None]), 'segmentation': torch.from_numpy(seg), 'name': 'a'})      # no spacing: (1, 1, 1)
    assert tuple(s['image'].shape) == (1, 2, 3, 5) and s['image'].dtype == torch.float32 and tuple(s['segmentation'].shape) == (2, 3, 5)
    assert np.array_equal(s['image'].cpu().numpy()[0], img[::2, ::2, ::2].astype(np.float32)) and np.array_equal(s['segmentation'].cpu().numpy(), seg[::2, ::2, ::2])
    # Normalization: mean 0, variance 1 (the tolerance of the pointwise pass: 4 * 2^-24 per voxel)
    s = T.Normalization()({'image': img, 'segmentation': seg, 'name': 'a'})
    y = s['image'].cpu().numpy().astype(np.float64)
    assert s['image'].dtype == torch.float32 and abs(y.mean()) <= 4 * 2.0 ** -24 * max(1.0, np.abs(y).max()) and abs(y.var(ddof=1) - 1.0) <= 1e-5
    m, sd = img.astype(np.float64).mean(), img.astype(np.float64).std(ddof=1)
    assert np.abs(y - (img - float(np.float32(m))) / float(np.float32(sd))).max() <= 4 * 2.0 ** -24 * max(1.0, np.abs(y).max())
    assert not T.Normalization()({'image': np.full((2, 3, 4), 7, dtype=np.int16), 'name': 'a'})['image'].any()
    # PercentileRescale
    s = T.PercentileRescale(1.0, 99.0)({'image': img, 'name': 'a'})
    lo, hi = np.percentile(img.astype(np.float64), [1.0, 99.0])
    want = np.clip((img.astype(np.float64) - float(np.float32(lo))) / float(np.float32(hi - lo)), 0, 1)
    y = s['image'].cpu().numpy().astype(np.float64)
    assert np.abs(y - want).max() <= 4 * 2.0 ** -24 and y.min() == 0.0 and y.max() == 1.0
    y = T.PercentileRescale(0.0, 100.0, clamp=False)({'image': img.astype(np.float32), 'name': 'a'})['image']
    assert float(y.min()) == 0.0 and float(y.max()) == 1.0
    # LeftToRight acts only on a name containing LEFT
    s = T.LeftToRight()({'image': img, 'segmentation': seg, 'name': '9001_LEFT_x'})
    assert np.array_equal(s['image'].cpu().numpy(), img[::-1]) and np.array_equal(s['segmentation'].cpu().numpy(), seg[::-1])
    s = T.LeftToRight()({'image': img, 'segmentation': seg, 'name': '9001_RIGHT_x'})
    assert s['image'] is img and s['segmentation'] is seg
    # SegmentationLabelFilter
    s = T.SegmentationLabelFilter([2, 5, 300])({'image': img, 'segmentation': seg, 'name': 'a'})
    assert np.array_equal(s['segmentation'].cpu().numpy(), np.where(np.isin(seg, [2, 5]), 0, seg))
    s = T.SegmentationLabelFilter([2])({'image': img, 'segmentation': seg.astype(np.int64) * 1000, 'name': 'a'})
    assert np.array_equal(s['segmentation'].cpu().numpy(), seg.astype(np.int32) * 1000)
    assert T.IdentityTransform()(s) is s
    # the chain of the experiments: device tensors in the reference's sample convention
    chain = T.Compose([T.Resample((1.0, 1.0, 1.0)), T.PercentileRescale(), T.SitkToTensor(), T.CropTensor([1, 1, 1])])
    s = chain({'image': img, 'segmentation': seg, 'name': 'a', 'spacing': (1.0, 1.0, 2.0)})
    assert tuple(s['image'].shape) == (1, 6, 4, 8) and s['image'].dtype == torch.float32 and tuple(s['segmentation'].shape) == (6, 4, 8)
    assert s['segmentation'].dtype == torch.uint8 and 0.0 <= float(s['image'].min()) and float(s['image'].max()) <= 1.0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
FILE_SHAPE, SHAPE = (8, 16, 32), (16, 16, 32)                    # spacing (1, 1, 2) -> voxel size 1 doubles z: the smallest shape of the one-epoch tests


def write_dataset(root, names, odd=None):
    from deepatlas_amd.lib.datasets import structured_labels
    from deepatlas_amd.lib.nifti import write_nifti
    os.makedirs(str(root), exist_ok=True)
    for k, name in enumerate(names):
        shape = (8, 16, 24) if name == odd else FILE_SHAPE
        lab = structured_labels(shape, 32, seed=k).numpy()
        rng = np.random.RandomState(k)
        img = (lab.astype(np.float64) * 90 + rng.uniform(0, 300, size=shape)).astype(np.int16)                  # raw intensities, 0 .. ~3100
        write_nifti(os.path.join(str(root), name + '_image.nii.gz'), img, spacing=(1.0, 1.0, 2.0))
        write_nifti(os.path.join(str(root), name + '_masks.nii.gz'), lab, spacing=(1.0, 1.0, 2.0))
    lists = {}
    for key, sel in (('train', names[:4]), ('valid', names[4:]), ('test', names[4:5])):
        lists[key] = os.path.join(str(root), key + '.txt')
        with open(lists[key], 'w') as f:
            f.write(''.join(n + '\n' for n in sel))
    return lists


def data_flags(root, lists, preload=False):
    flags = ['--data', 'OAI', '--data-dir', str(root), '--train-list', lists['train'], '--valid-list', lists['valid'], '--test-list', lists['test'],
             '--voxel-size', '1', '1', '1', '--rescale-percentiles', '0.5', '99.5']
    return flags + (['--preload'] if preload else [])


def seg_config(tmp_path, root, lists, preload):
    import train_seg
    seen = []

    class Capture(object):
        def __init__(self, config):
            seen.append(config)

        def train(self):
            pass

        def test(self):
            pass
    real = train_seg.SegmentationExperiment
    train_seg.SegmentationExperiment = Capture
    try:
        train_seg.main(['--num-samples', '2', '--num-epochs', '1', '--log-root', str(tmp_path / 'logs')] + data_flags(root, lists, preload))
    finally:
        train_seg.SegmentationExperiment = real
    cfg = seen[0]
    cfg.update(lr_mode='const', samples_per_epoch=2, print_batch_period=1)
    return cfg


NAMES = ['s0', 's1_LEFT', 's2', 's3', 'v0', 'v1']


def test_segmentation_experiment_on_nifti_files(tmp_path, capsys):
    from deepatlas_amd import ops
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    root = tmp_path / 'oai'
    lists = write_dataset(root, NAMES)
    first = {}
    for preload in (False, True):
        cfg = seg_config(tmp_path / str(preload), root, lists, preload)
        assert cfg['data'] == 'OAI' and cfg['preload'] is preload and cfg['training_list_file'] == [lists['train']]
        exp = SegmentationExperiment(cfg)
        ops.set_deterministic(True)
        exp.setup_train()
        exp.initialize_model(exp.model, exp.optimizer, '')
        assert len(exp.training_data_loader.dataset) == 4 and len(exp.validation_data_loader.dataset) == 2 and len(exp.testing_data_loader.dataset) == 1
        torch.manual_seed(3)
        images, truths, names = next(iter(exp.training_data_loader))
        assert images.is_cuda and tuple(images.shape) == (1, 1) + SHAPE and images.dtype == torch.float32 and truths.dtype == torch.uint8
        assert tuple(truths.shape) == (1,) + SHAPE and 0.0 <= float(images.min()) and float(images.max()) <= 1.0 and int(truths.max()) < 32
        loss, _ = exp.train_step(images, truths)
        first[preload] = (names[0], float(loss.detach()), images.clone())
    assert first[False][0] == first[True][0] and torch.equal(first[False][2], first[True][2])
    assert first[False][1] == first[True][1] and math.isfinite(first[True][1])                     # preload on and off: the same first step
    ops.set_deterministic(False)
    exp = SegmentationExperiment(seg_config(tmp_path / 'run', root, lists, True))
    exp.train()                                                                                    # one epoch plus validation
    dice_per_class, dice_avg = exp.test()
    out = capsys.readouterr().out
    assert math.isfinite(float(dice_avg)) and 'Testing Model' in out and len([l for l in out.splitlines() if l.startswith('Epoch[')]) == 2


def test_mixed_shapes_raise_at_setup(tmp_path):
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    root = tmp_path / 'oai'
    lists = write_dataset(root, NAMES, odd='s2')
    exp = SegmentationExperiment(seg_config(tmp_path, root, lists, False))
    with pytest.raises(ValueError, match=r's0 16x16x32, s1_LEFT 16x16x32, s2 16x16x24'):
        exp.setup_train()
    cfg = seg_config(tmp_path / 'b', root, write_dataset(tmp_path / 'ok', NAMES), False)
    cfg['data_dir'] = cfg['valid_data_dir'] = str(tmp_path / 'ok')
    cfg['preprocess'] = cfg['preprocess'][1:]                                                      # no resample: 8 x 16 x 32 volumes ...
    cfg['crop_size'] = [1, 0, 0]                                                                   # ... cropped to 6 x 16 x 32
    with pytest.raises(ValueError, match='multiples of 8'):
        SegmentationExperiment(cfg).setup_train()


def reg_flags(tmp_path, root, lists):
    return ['--num-samples', '3', '--num-epochs', '1', '--device', '0', '--log-root', str(tmp_path / 'logs')] + data_flags(root, lists, preload=True)


def test_registration_experiment_on_nifti_files(tmp_path, monkeypatch, capsys):
    import train_reg
    from deepatlas_amd.models.registration import RegistrationExperiment
    monkeypatch.chdir(tmp_path)
    root = tmp_path / 'oai'
    lists = write_dataset(root, NAMES)
    seen = []
    real_init = RegistrationExperiment.__init__

    def init(self, config):
        config.update(lr_mode='const', samples_per_epoch=2, print_batch_period=1)
        real_init(self, config)
        seen.append(self)
    monkeypatch.setattr(RegistrationExperiment, '__init__', init)
    res = train_reg.main(reg_flags(tmp_path, root, lists))
    out = capsys.readouterr().out
    exp = seen[0]
    assert len(exp.training_data_loader.dataset) == 6 and len(exp.validation_data_loader.dataset) == 2              # 3 volumes -> 6 ordered pairs
    assert exp.training_data_loader.dataset.seg.name_list == ['s0', 's1_LEFT', 's2']
    assert len([l for l in out.splitlines() if l.startswith('Validation:')]) == 1 and math.isfinite(float(res['dice_avg']))
    for extra in (['--misalign', '5', '2'], ['--report-tre', '2']):
        with pytest.raises(ValueError, match='synthetic-only'):
            train_reg.main(reg_flags(tmp_path, root, lists) + extra)


def test_joint_experiment_on_nifti_files(tmp_path, monkeypatch):
    import train_joint
    from deepatlas_amd.models import joint
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    monkeypatch.chdir(tmp_path)
    root = tmp_path / 'oai'
    lists = write_dataset(root, NAMES)
    seen, kinds = [], []
    real_init = DeepAtlasExperiment.__init__

    def init(self, config):
        config.update(lr_mode='const', samples_per_epoch=3, print_batch_period=1)
        real_init(self, config)
        seen.append(self)
    monkeypatch.setattr(DeepAtlasExperiment, '__init__', init)
    inner_call = joint.DeepAtlasJointStep.__call__
    monkeypatch.setattr(joint.DeepAtlasJointStep, '__call__',
                        lambda self, im_m, im_t, seg_m, seg_t: kinds.append((seg_m is None, seg_t is None)) or inner_call(self, im_m, im_t, seg_m, seg_t))
    res = train_joint.main(reg_flags(tmp_path, root, lists) + ['--num-labeled', '2'])
    exp = seen[0]
    data = exp.training_data_loader.dataset
    assert exp.labeled == [0, 1] and data.seg.name_list == ['s0', 's1_LEFT', 's2'] and data.pairs == [(1, 0), (2, 0), (0, 1), (2, 1)]
    assert len(kinds) == 3 and all(not t_none for _, t_none in kinds)
    assert set(res) >= {'seg_dice_avg', 'dice_avg'} and math.isfinite(float(res['seg_dice_avg']))


def test_synthetic_run_is_what_it_was(tmp_path):
    """Without the new keys: the config has none of them, and the first step on the loaders setup builds equals the step on the same synthetic
    dataset handed in from outside."""
    import train_seg
    from torch.utils.data import DataLoader
    from deepatlas_amd import ops
    from deepatlas_amd.lib.datasets import SyntheticSegDataset
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    losses = []
    for injected in (False, True):
        ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False, data_root='./data',
                                log_root=str(tmp_path / str(injected)), shape=list(SHAPE))
        cfg = train_seg.build_config(ns)
        assert cfg['data'] == 'synthetic' and not {'training_list_file', 'validation_list_file', 'testing_list_file', 'preprocess'} & set(cfg)
        assert cfg['crop_size'] == [0, 10, 7, 14, 8, 7] and cfg['preload'] is False and cfg['data_dir'] == os.path.join('./data', 'synthetic')
        if injected:
            cfg['training_data_loader'] = DataLoader(SyntheticSegDataset(2, SHAPE, 32, seed=230), batch_size=1, shuffle=True, num_workers=0)
            cfg['validation_data_loader'] = DataLoader(SyntheticSegDataset(2, SHAPE, 32, seed=1230), batch_size=1, shuffle=False, num_workers=0)
        exp = SegmentationExperiment(cfg)
        ops.set_deterministic(True)
        exp.setup_train()
        exp.initialize_model(exp.model, exp.optimizer, '')
        assert isinstance(exp.training_data_loader.dataset, SyntheticSegDataset) and len(exp.training_data_loader.dataset) == 2
        torch.manual_seed(5)
        images, truths, names = next(iter(exp.training_data_loader))
        loss, _ = exp.train_step(images, truths)
        losses.append((names[0], float(loss.detach())))
    assert losses[0] == losses[1] and math.isfinite(losses[0][1])
