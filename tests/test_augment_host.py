"""Random rigid / B-spline augmentation (lib/transforms.py:161-290): parameter draws, host-side geometry, argument checks -- no GPU."""
import argparse
import itertools

import numpy as np
import pytest
import torch


def _rot(ax, ay, az):
    """Euler3DTransform, ComputeZYX off: Rz Rx Ry, written out."""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
            @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]))


def test_rigid_draws_replay_the_reference_sequence():
    from deepatlas_amd.lib import transforms as T
    angles, trans, spacing = (10.0, 0.0, 30.0), (4.0, 0.0, 2.0), (1.0, 1.2, 2.0)      # zero scales are drawn all the same
    np.random.seed(7)
    got = T.draw_rigid(1.0, angles, trans, spacing)
    np.random.seed(7)
    assert np.random.rand(1)[0] < 1.0
    want_a = [np.random.normal(0, angles[k] / 2) * np.pi / 180 for k in range(3)]
    want_t = [np.random.normal(0, trans[k] / 2) * spacing[k] for k in range(3)]
    assert np.array_equal(got[0], want_a) and np.array_equal(got[1], want_t)
    assert got[0][1] == 0 and got[1][1] == 0
    # a failed coin draws nothing more
    np.random.seed(3)
    assert T.draw_rigid(0.0, angles, trans, spacing) is None
    after = np.random.rand()
    np.random.seed(3)
    np.random.rand(1)
    assert after == np.random.rand()
    # a batch of 3 = 3 single draws, sample after sample, coins included
    tr = T.RandomRigidTransform(ratio=0.6, rotation_angles=angles, translation=trans)
    np.random.seed(11)
    batch = tr.draw(3, spacing)
    np.random.seed(11)
    singles = [T.draw_rigid(0.6, angles, trans, spacing) for _ in range(3)]
    np.random.seed(11)
    replay = []
    for _ in range(3):
        if np.random.rand(1)[0] < 0.6:
            a = [np.random.normal(0, angles[k] / 2) * np.pi / 180 for k in range(3)]
            t = [np.random.normal(0, trans[k] / 2) * spacing[k] for k in range(3)]
            replay.append((a, t))
        else:
            replay.append(None)
    for b, s, r in zip(batch, singles, replay):
        assert (b is None) == (s is None) == (r is None)
        if b is not None:
            assert np.array_equal(b[0], s[0]) and np.array_equal(b[0], r[0]) and np.array_equal(b[1], r[1])


@pytest.mark.parametrize('mode', ['Normal', 'Uniform'])
def test_bspline_draws_replay_the_reference_sequence(mode):
    from deepatlas_amd.lib import transforms as T
    mesh, order, scale = (2, 4, 3), 2, 3.0
    grid = T.bspline_grid((45, 52, 37), mesh, order)
    assert grid == (4, 6, 5)
    n = 3 * 4 * 6 * 5
    np.random.seed(5)
    got = T.draw_bspline(1.0, n, scale, mode)
    np.random.seed(5)
    np.random.rand(1)
    want = np.random.normal(0, scale / 2, n) if mode == 'Normal' else np.random.random(n) * scale
    want[0:int(n / 3)] = 0                   # the reference's "remove z displacement": the x third in ITK's layout
    assert np.array_equal(got, want) and np.all(got[:n // 3] == 0) and np.any(got[n // 3:] != 0)
    tr = T.RandomBSplineTransform(mesh_size=mesh, bspline_order=order, deform_scale=scale, ratio=0.5, random_mode=mode)
    np.random.seed(2)
    batch = tr.draw(4, (45, 52, 37))
    np.random.seed(2)
    singles = [T.draw_bspline(0.5, n, scale, mode) for _ in range(4)]
    assert [b is None for b in batch] == [s is None for s in singles]
    for b, s in zip(batch, singles):
        assert b is None or np.array_equal(b, s)
    # a zero scale still draws its vector
    np.random.seed(9)
    z = T.draw_bspline(1.0, n, 0.0, mode)
    assert np.all(z == 0) and np.random.rand() == _after(9, n, mode)
    with pytest.raises(ValueError):
        T.draw_bspline(1.0, n, 1.0, 'Laplace')


def _after(seed, n, mode):
    np.random.seed(seed)
    np.random.rand(1)
    np.random.normal(0, 0.0, n) if mode == 'Normal' else np.random.random(n)
    return np.random.rand()


@pytest.mark.parametrize('angles,spacing', [((0.1, -0.2, 0.3), (1.0, 1.0, 1.0)), ((0.5, 0.0, -1.1), (1.0, 1.2, 2.0)),
                                            ((np.pi / 2, 0.3, 0.0), (0.7, 1.0, 1.3)), ((0.0, 0.0, 0.0), (2.0, 1.0, 1.0))])
def test_rigid_index_affine_is_the_physical_space_composition(angles, spacing):
    from deepatlas_amd.lib import transforms as T
    t = np.array([1.5, -2.25, 0.5])
    center = (20, 26, 18)
    A = T.rigid_index_affine(angles, t, spacing, center)
    S = np.diag(spacing)
    R = _rot(*angles)
    c = S @ np.array(center, dtype=np.float64)
    rng = np.random.RandomState(0)
    for i in list(rng.uniform(-5, 50, (20, 3))) + [np.array(center, dtype=np.float64)]:
        want = np.linalg.solve(S, R @ (S @ i - c) + c + t)
        assert np.allclose(A[:, :3] @ i + A[:, 3], want, rtol=0, atol=1e-12)
    A0 = T.rigid_index_affine(angles, (0, 0, 0), spacing, center)
    assert np.allclose(A0[:, :3] @ np.array(center) + A0[:, 3], center, rtol=0, atol=1e-12)        # the centre is a fixed point
    assert np.allclose(np.linalg.det(A[:, :3]), 1.0)


def test_bspline_grid_support_and_coefficient_layout():
    from deepatlas_amd.lib import transforms as T
    for order, M, size in itertools.product((1, 2, 3), (1, 3, 4), (2, 37, 160)):
        i = np.arange(size)
        start, w = T.bspline_support(i, size, M, order)
        g = i * M / (size - 1) + (order - 1) / 2
        assert np.all(start <= M - 1) and np.all(start >= 0) and np.all(start + order <= M + order - 1)
        assert start[-1] == M - 1                                                  # upper face: the clamp, the limit from inside
        inner = g - (order - 1) / 2 < M
        assert np.array_equal(start[inner], np.floor(g - (order - 1) / 2)[inner])
        assert np.allclose(w.sum(1), 1.0, atol=1e-12) and np.all(w >= 0)
        u = g[:, None] - (start[:, None] + np.arange(order + 1))
        assert np.allclose(w, T.bspline_kernel(u, order))
    # the upper face by hand: order 2, M = 3: g = 3.5, start 2 (not 3), weights B2(1.5), B2(0.5), B2(-0.5) = 0, 1/2, 1/2
    s, w = T.bspline_support(np.array([9]), 10, 3, 2)
    assert s[0] == 2 and np.allclose(w[0], [0.0, 0.5, 0.5])
    # hat / quadratic / cubic values
    assert np.allclose(T.bspline_kernel([0, 0.5, 1], 1), [1, 0.5, 0])
    assert np.allclose(T.bspline_kernel([0, 0.5, 1, 1.5], 2), [0.75, 0.5, 0.125, 0])
    assert np.allclose(T.bspline_kernel([0, 1, 2], 3), [2 / 3, 1 / 6, 0])
    # ITK layout: x component first, each grid flattened with x fastest
    grid = T.bspline_grid((45, 52, 37), (2, 4, 3), 3)
    assert grid == (5, 7, 6)
    p = np.arange(3 * 5 * 7 * 6, dtype=np.float64)
    cf = T.bspline_coefficients(p, grid)
    assert cf.shape == (3, 6, 7, 5)
    assert cf[0, 0, 0, 1] == 1 and cf[0, 0, 1, 0] == 5 and cf[0, 1, 0, 0] == 35 and cf[1, 0, 0, 0] == 210 and cf[2, 0, 0, 0] == 420
    for bad in (0, 4):
        with pytest.raises(ValueError):
            T.bspline_grid((8, 8, 8), (3, 3, 3), bad)
        with pytest.raises(ValueError):
            T.RandomBSplineTransform(bspline_order=bad)
    with pytest.raises(ValueError):
        T.bspline_grid((8, 1, 8), (3, 3, 3), 2)


def test_transform_arguments_are_checked_on_the_host():
    from deepatlas_amd.lib import transforms as T
    with pytest.raises(ValueError):
        T.RandomRigidTransform(mode='both_ways')
    for interp in ('bspline', 3):
        with pytest.raises(NotImplementedError):
            T.RandomRigidTransform(interpolator=interp)
        with pytest.raises(NotImplementedError):
            T.RandomBSplineTransform(interpolator=interp)
    assert [type(t).__name__ for t in T.make_augmentation([['rigid', {'rotation_angles': [5, 5, 5]}], ['bspline', {}]])] == \
        ['RandomRigidTransform', 'RandomBSplineTransform']
    assert T.make_augmentation(None) == [] and T.make_augmentation([]) == []
    with pytest.raises(ValueError):
        T.make_augmentation([['flip', {}]])


def test_failed_coin_returns_the_sample_untouched_without_a_device_call(monkeypatch):
    from deepatlas_amd import ops
    from deepatlas_amd.lib import transforms as T

    def no_call(*a, **k):
        raise AssertionError('device call on a failed coin')
    monkeypatch.setattr(ops, 'spatial_resample', no_call)
    img = torch.rand(1, 6, 7, 8)
    seg = torch.zeros(6, 7, 8, dtype=torch.uint8)
    for tr in (T.RandomRigidTransform(ratio=0.0, rotation_angles=(10, 10, 10)), T.RandomBSplineTransform(ratio=0.0, deform_scale=4)):
        sample = {'image': img, 'segmentation': seg}
        out = tr(sample)
        assert out is sample and out['image'] is img and out['segmentation'] is seg
        batch = {'image': img[None].expand(3, -1, -1, -1, -1), 'segmentation': seg[None].expand(3, -1, -1, -1)}
        assert tr(batch)['image'] is batch['image']


def test_spatial_resample_c_abi_rejects_bad_arguments_before_touching_the_device():
    from ctypes import c_void_p
    from deepatlas_amd import _native
    L = _native.lib()
    f, g, a, b = c_void_p(0x1000), c_void_p(0x2000), c_void_p(0x3000), c_void_p(0x4000)
    aff, cf = c_void_p(0x5000), c_void_p(0x6000)
    BAD, UNSUP = -1, -3
    ok = dict(img=f, img_out=g, C=1, interp=0, lab=a, lab_out=b, lb=1, aff=aff, coef=cf, order=2, gx=5, gy=5, gz=5, N=1, D=8, H=8, W=8)

    def run(**kw):
        k = dict(ok, **kw)
        return L.da_spatial_resample(k['img'], k['img_out'], k['C'], k['interp'], k['lab'], k['lab_out'], k['lb'], k['aff'], k['coef'],
                                     k['order'], k['gx'], k['gy'], k['gz'], k['N'], k['D'], k['H'], k['W'], None)
    assert run(N=0) == BAD
    assert run(D=0) == BAD
    assert run(aff=None) == BAD
    assert run(img=None, img_out=None, lab=None, lab_out=None) == BAD                 # nothing to resample
    assert run(img_out=None) == BAD and run(lab_out=None) == BAD                       # an input without its output
    assert run(img_out=f) == BAD                                                       # in place
    assert run(C=0) == BAD and run(interp=2) == BAD
    assert run(lb=2) == BAD and run(lb=0) == BAD                                       # label_bytes 1, 4 or 8
    assert run(order=4) == BAD and run(order=-1) == BAD
    assert run(coef=None) == BAD                                                       # B-spline without coefficients
    assert run(W=1) == BAD                                                             # axis shorter than 2
    assert run(gx=2) == BAD                                                            # control grid smaller than order + 1
    assert run(gx=20, gy=20, gz=20) == UNSUP                                           # above DA_AUG_MAX_GRID_POINTS
    assert run(order=0, coef=None, W=1, gx=0, gy=0, gz=0, C=0) == BAD


def test_build_config_with_and_without_the_augmentation_flags():
    import train_seg
    base = dict(device='0', debug=False, preload=False, num_samples=21, num_epochs=100, lr=1e-3, test_only=False,
                data_root='./data', log_root='./logs', shape=[64, 64, 64])
    c = train_seg.build_config(argparse.Namespace(**base))                 # a Namespace without the new attributes
    assert 'augment' not in c and 'aug_rigid' not in c
    c2 = train_seg.build_config(argparse.Namespace(aug_rigid=None, aug_bspline=None, **base))
    assert c2 == c
    c3 = train_seg.build_config(argparse.Namespace(aug_rigid=[10, 10, 10, 4, 4, 4], aug_bspline=4.0, **base))
    assert c3['augment'] == [['rigid', {'rotation_angles': [10, 10, 10], 'translation': [4, 4, 4]}], ['bspline', {'deform_scale': 4.0}]]
    assert 'aug_rigid' not in c3 and 'aug_bspline' not in c3
    assert {k: v for k, v in c3.items() if k != 'augment'} == c
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    assert SegmentationExperiment.experiment_name(c3) == SegmentationExperiment.experiment_name(c)
    c4 = train_seg.build_config(argparse.Namespace(aug_rigid=None, aug_bspline=2.0, **base))
    assert c4['augment'] == [['bspline', {'deform_scale': 2.0}]]


def test_train_seg_parses_the_augmentation_flags(monkeypatch):
    import train_seg
    seen = []

    class Stop(Exception):
        pass

    def fake_experiment(cfg):
        seen.append(cfg)
        raise Stop()
    monkeypatch.setattr(train_seg, 'SegmentationExperiment', fake_experiment)
    for argv in ([], ['--aug-rigid', '10', '10', '10', '4', '4', '4', '--aug-bspline', '4']):
        with pytest.raises(Stop):
            train_seg.main(argv)
    assert 'augment' not in seen[0]
    assert seen[1]['augment'] == [['rigid', {'rotation_angles': [10.0, 10.0, 10.0], 'translation': [4.0, 4.0, 4.0]}],
                                  ['bspline', {'deform_scale': 4.0}]]
