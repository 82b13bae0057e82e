"""CPU companion of test_gpu_crop.py: the numpy references of tests/crop_cases.py checked against the definitions they restate, the
properties the GPU tests rely on (the admissible sets of the cases are neither empty nor the whole domain; the fallback case is one), the
host half of the crop ops, and what needs no device of the transforms and the experiment's patch mode."""
import numpy as np
import pytest

import crop_cases as cc
from deepatlas_amd import ops
from deepatlas_amd.lib import transforms as T
from deepatlas_amd.models import nifti_data


def test_integral_image_against_brute_force():
    for shape, window in (((5, 6, 7), (1, 1, 1)), ((5, 6, 7), (5, 1, 7)), ((5, 6, 7), (2, 3, 4)), ((4, 5, 70), (2, 3, 33))):
        lab = cc.ellipsoid_labels(shape, n=2)
        for cls in (0, 1, 2, 9):
            assert np.array_equal(cc.integral_counts(lab, window, cls), cc.brute_counts(lab, window, cls))


def test_cases_have_the_admissible_sets_the_gpu_tests_need():
    shape, window = cc.MAIN
    lab = cc.ellipsoid_labels(shape, n=3)
    dom = cc.domain(shape, window)
    assert dom == (8, 12, 37)
    size = window[0] * window[1] * window[2]
    for cls in (1, 2):
        cnt = cc.integral_counts(lab, window, cls)[:, :dom[0], :dom[1], :dom[2]]
        sizes = [[int((cnt[n] >= cc.min_count(t, size)).sum()) for t in cc.THRESHOLDS] for n in range(3)]
        print('class', cls, 'admissible of', int(np.prod(dom)), sizes)
        for row in sizes:
            assert all(0 < v < np.prod(dom) for v in row) and row[0] > row[1] > row[2]
    shape, window = cc.FALLBACK
    lab = cc.ellipsoid_labels(shape, n=3)
    m = cc.min_count(0.2, window[0] * window[1] * window[2])
    for include_last in (False, True):
        dom = cc.domain(shape, window, include_last)
        for cls in (1, 2):
            assert int((cc.integral_counts(lab, window, cls)[:, :dom[0], :dom[1], :dom[2]] >= m).sum()) == 0
    assert cc.domain(*cc.SINGLE) == (1, 1, 1) and cc.domain(*cc.SINGLE, include_last=True) == (1, 1, 1)


def test_every_admissible_start_is_drawn_and_the_rejection_loop_has_the_same_support():
    shape, window = (6, 9, 40), (2, 3, 16)
    lab = np.zeros((1,) + shape, dtype=np.uint8)
    lab[0, 1:4, 2:6, 5:22] = 1                                              # windows inside the block: 2 x 2 x 2 starts hold only class 1
    full = 2 * 3 * 16
    dom = cc.domain(shape, window)
    cnt = cc.integral_counts(lab, window, 1)[0, :dom[0], :dom[1], :dom[2]]
    admissible = set(map(tuple, np.argwhere(cnt >= full)))
    assert len(admissible) == 8
    starts, info = cc.ref_starts(lab, window, [1] * 512, [full] * 512, seed=12345)
    assert (info[0, :, 0] == 8).all() and (info[0, :, 1] == full).all()
    drawn = set(map(tuple, starts[0]))
    assert drawn == admissible                                              # deterministic for the pinned seed
    rng = np.random.RandomState(7)
    threshold = (full - 1) / full                                           # share > threshold <=> count == full
    assert cc.min_count(threshold, full) == full
    looped, tries = set(), 0
    for _ in range(200):
        s, t = cc.rejection_loop(lab[0], window, 1, threshold, rng)
        looped.add(s)
        tries += t
    print('rejection loop: %.1f tries per crop' % (tries / 200.0))
    assert looped == admissible


def test_unconditioned_draws_cover_the_domain_and_never_the_last_start():
    shape, window = (4, 5, 9), (2, 3, 4)
    lab = np.zeros((1,) + shape, dtype=np.uint8)
    starts, info = cc.ref_starts(lab, window, [None] * 2048, [0] * 2048, seed=1)
    assert set(map(tuple, starts[0])) == set(np.ndindex(2, 2, 5)) and (info[0, :, 0] == 20).all() and (info[0, :, 1] == -1).all()
    starts, _ = cc.ref_starts(lab, window, [None] * 2048, [0] * 2048, seed=1, include_last=True)
    assert set(map(tuple, starts[0])) == set(np.ndindex(3, 3, 6))


def test_crop_min_count_is_the_float64_comparison():
    for size in (1, 7, 96, 100, 1056, 4 * 8 * 33, 32 * 128 * 128):
        ts = [0.0, -0.0, 0.01, 0.05, 0.2, 0.5, 0.999, 1.0, 1.5, -0.1, 1e-9] + [k / size for k in (0, 1, 2, size // 2, size - 1, size) if k <= size]
        ts += list(np.random.RandomState(size).rand(50)) + [np.nextafter(k / size, d) for k in (1, size // 2 + 1) for d in (0.0, 2.0)]
        for t in ts:
            n = T.crop_min_count(t, size)
            assert n == (0 if t < 0 else cc.min_count(t, size)), (t, size)
            assert n > size or np.float64(n) / np.float64(size) > np.float64(t)
            assert n == 0 or not np.float64(n - 1) / np.float64(size) > np.float64(t)
    assert T.crop_min_count(0.01, 100) == 2 and T.crop_min_count(0.0, 5) == 1 and T.crop_min_count(1.0, 5) == 6
    with pytest.raises(ValueError):
        T.crop_min_count(0.1, 0)


def test_crop_conditions_group_the_draws():
    conds, draw = ops.crop_conditions([2, None, 1, 2, 2, 1], [5, 0, 3, 5, 7, 3])
    assert conds.tolist() == [[1, 3], [2, 5], [2, 7]] and draw.tolist() == [1, -1, 0, 1, 2, 0]
    conds, draw = ops.crop_conditions([None], [0])
    assert conds.shape == (0, 2) and draw.tolist() == [-1]
    for bad in (([1], [1, 2]), ([], []), ([1], [-1]), ([2 ** 40], [1]), ([1] * 65537, [1] * 65537)):
        with pytest.raises(ValueError):
            ops.crop_conditions(*bad)
    assert ops.crop_domain((12, 20, 70), (4, 8, 33)) == (8, 12, 37) and ops.crop_domain((12, 20, 70), (12, 8, 33), True) == (1, 13, 38)


def test_crop_constructors_keep_the_reference_asserts():
    assert T.RandomCrop(8).output_size == (8, 8, 8) and T.RandomCrop((1, 2, 3)).output_size == (1, 2, 3)
    t = T.BalancedRandomCrop(8)
    assert t.threshold == (0.01, 0.01, 0.01) and t.current_class == 2 and t.patches == 1
    assert T.BalancedRandomCrop(8, threshold=(0.1, 0.2)).threshold == (0.1, 0.2)
    assert [t._next_tags(1)[0] for _ in range(6)] == [2, 3, 0, 1, 2, 3]
    for bad in (lambda: T.RandomCrop([8, 8, 8]), lambda: T.RandomCrop((8, 8)), lambda: T.BalancedRandomCrop(8, threshold=1),
                lambda: T.BalancedRandomCrop(8, threshold=(0.1, 0.2, 0.3))):
        with pytest.raises(AssertionError):
            bad()
    for bad in (lambda: T.BalancedRandomCrop(8, classes=[]), lambda: T.BalancedRandomCrop(8, classes=[1, 2], threshold=[0.1]),
                lambda: T.BalancedRandomCrop(8, patches=0)):
        with pytest.raises(ValueError):
            bad()
    own = T.BalancedRandomCrop(8, threshold=0.1, classes=[3, None, 5])
    assert own.cycle == [(3, 0.1), (None, 0.1), (5, 0.1)] and own._next_tags(4) == [0, 1, 2, 0]
    assert sorted(T.CROPS) == ['balanced_crop', 'crop']
    made = T.make_augmentation([['crop', {'output_size': [8, 8, 8]}], ['balanced_crop', {'output_size': [8, 8, 8], 'threshold': [0.01, 0.02]}], ['rigid', {}]])
    assert [type(t) for t in made] == [T.RandomCrop, T.BalancedRandomCrop, T.RandomRigidTransform] and made[1].threshold == (0.01, 0.02)
    with pytest.raises(ValueError):
        T.make_augmentation([['patch', {}]])


class _Vols(list):
    pass


def _vols(shapes):
    import torch
    return _Vols((torch.zeros((1,) + s), torch.zeros(s, dtype=torch.uint8), 'v%d' % k) for k, s in enumerate(shapes))


def test_check_shapes_with_a_patch():
    patch = {'size': [8, 16, 16], 'overlap': [2, 4, 4]}
    out = nifti_data.check_shapes([_vols([(8, 16, 24), (9, 17, 16)]), None, _vols([(20, 16, 16)])], ['UNet_light'], patch=patch)
    assert out == (8, 16, 16)
    with pytest.raises(ValueError, match='do not share one shape'):
        nifti_data.check_shapes([_vols([(8, 16, 24), (9, 17, 16)])], ['UNet_light'])                     # as today
    with pytest.raises(ValueError, match=r'v1 7x16x16'):
        nifti_data.check_shapes([_vols([(8, 16, 24), (7, 16, 16)])], ['UNet_light'], patch=patch)        # a volume below the patch
    with pytest.raises(ValueError, match='multiples of 8'):
        nifti_data.check_shapes([_vols([(8, 16, 24)])], ['UNet_light'], patch={'size': [8, 12, 16], 'overlap': [0, 0, 0]})
    with pytest.raises(ValueError, match='overlap'):
        nifti_data.check_shapes([_vols([(8, 16, 24)])], ['UNet_light'], patch={'size': [8, 16, 16], 'overlap': [4, 4, 4]})
    assert nifti_data.check_shapes([_vols([(8, 16, 20)])], ['voxel_morph_cvpr'], patch={'size': [3, 5, 7], 'overlap': [1, 2, 3]}) == (3, 5, 7)


def _args(extra):
    import train_seg
    import argparse
    captured = {}
    real = train_seg.SegmentationExperiment

    class Stop(Exception):
        pass

    def fake(config):
        captured['config'] = config
        raise Stop()
    train_seg.SegmentationExperiment = fake
    try:
        with pytest.raises(Stop):
            train_seg.main(['--num-samples', '2', '--num-epochs', '1'] + extra)
    finally:
        train_seg.SegmentationExperiment = real
    return captured['config']


def test_train_seg_patch_flags_and_names():
    from deepatlas_amd.models.segmentation import SegmentationExperiment, parse_patch
    plain = _args([])
    assert 'patch' not in plain and not any(k.startswith('patch_') or k.startswith('tile_') for k in plain)
    name = SegmentationExperiment.experiment_name(plain)
    assert name == 'Seg_UNet_light_bias_BN_synthetic_2samples_batch_1_1epochs_dice_Uniform_lr_0.001_scheduler_multiStep'
    cfg = _args(['--patch-size', '16', '32', '32', '--patch-mode', 'random', '--patch-threshold', '0.05', '--patches-per-volume', '2',
                 '--tile-overlap', '2', '4', '4', '--tile-batch', '3'])
    assert cfg['patch'] == {'size': [16, 32, 32], 'mode': 'random', 'threshold': 0.05, 'classes': None, 'per_volume': 2, 'overlap': [2, 4, 4],
                            'tile_batch': 3, 'include_last': False}
    assert SegmentationExperiment.experiment_name(cfg) == name + '_patch16x32x32'
    assert parse_patch(None) is None
    assert parse_patch({'size': (32, 64, 64)}) == {'size': [32, 64, 64], 'mode': 'balanced', 'threshold': 0.01, 'classes': None, 'per_volume': 1,
                                                   'overlap': [8, 8, 8], 'tile_batch': 4, 'include_last': False}
    for bad in ({'size': [8, 8]}, {'size': [8, 8, 8], 'mode': 'centre'}, {'size': [8, 8, 8], 'per_volume': 0}, {'size': [8, 8, 8], 'colour': 1},
                {'size': [8, 8, 8], 'tile_batch': 0}, {'size': [0, 8, 8]}):
        with pytest.raises(ValueError):
            parse_patch(bad)


def test_other_experiments_refuse_the_patch_key():
    from deepatlas_amd.models.segmentation import refuse_patch
    refuse_patch({}, 'registration')
    refuse_patch({'patch': None}, 'registration')
    with pytest.raises(ValueError, match='patch'):
        refuse_patch({'patch': {'size': [8, 8, 8]}}, 'registration')
