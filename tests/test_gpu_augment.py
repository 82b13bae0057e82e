"""Random rigid / B-spline augmentation on the device (da_spatial_resample; lib/transforms.py:161-290): exact cases, an fp64 CPU oracle
written here from the ITK rules (independently of the host helpers in deepatlas_amd.lib.transforms), batching, determinism, modes,
label dtypes, and the experiment's `augment` key."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _volume(shape, C=1, seed=0, label_dtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((C,) + tuple(shape), generator=g)
    lab = torch.randint(0, 32, tuple(shape), generator=g).to(label_dtype)
    return img.to(DEV), lab.to(DEV)


# ---- fp64 oracle -----------------------------------------------------------------------------------------------------------------
def _euler(ax, ay, az):
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def _index_grid(shape):
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    return np.stack([x, y, z])


def _q_rigid(shape, angles, t, spacing, center):
    """Output index -> input index of sitk.Euler3DTransform(c, angles, t) with c = S center (physical space, then back to an index)."""
    S = np.asarray(spacing, dtype=np.float64)[:, None, None, None]
    c = np.asarray(spacing, dtype=np.float64) * np.asarray(center, dtype=np.float64)
    p = _index_grid(shape) * S
    R = _euler(*angles)
    q = np.einsum('ij,j...->i...', R, p - c[:, None, None, None]) + (c + np.asarray(t))[:, None, None, None]
    return q / S


def _bspline_value(u, order):
    a = np.abs(u)
    if order == 1:
        return np.maximum(1 - a, 0)
    if order == 2:
        return np.where(a < 0.5, 0.75 - a ** 2, np.where(a < 1.5, (1.5 - a) ** 2 / 2, 0))
    return np.where(a < 1, 2 / 3 - a ** 2 + a ** 3 / 2, np.where(a < 2, (2 - a) ** 3 / 6, 0))


def _basis(size, M, order):
    """size x (M + order): row i holds the weights of the control points along one axis (ITK: start clamped at the upper face)."""
    B = np.zeros((size, M + order))
    for i in range(size):
        g = i * M / (size - 1) + (order - 1) / 2
        s = min(int(np.floor(g - (order - 1) / 2)), M - 1)
        for k in range(order + 1):
            B[i, s + k] = _bspline_value(g - s - k, order)
    return B


def _q_bspline(shape, params, mesh, order, spacing):
    D, H, W = shape
    Mx, My, Mz = mesh
    coef = np.asarray(params, dtype=np.float64).reshape(3, Mz + order, My + order, Mx + order)      # ITK: x, y, z; x fastest
    disp = np.einsum('zc,yb,xa,ncba->nzyx', _basis(D, Mz, order), _basis(H, My, order), _basis(W, Mx, order), coef)
    return _index_grid(shape) + disp / np.asarray(spacing, dtype=np.float64)[:, None, None, None]


def _resample(img, lab, q, interp='linear'):
    """sitk.Resample rules: inside -0.5 <= q < size - 0.5; image trilinear with clamped neighbours (or nearest), labels floor(q + 0.5);
    outside 0.1 / 0.  Returns (image, labels, inside, band): band = voxels whose q lies within 1e-4 of a half-integer on some axis (a
    rounding tie or the inside / outside boundary)."""
    C, D, H, W = img.shape
    qx, qy, qz = q
    inside = (qx >= -0.5) & (qx < W - 0.5) & (qy >= -0.5) & (qy < H - 0.5) & (qz >= -0.5) & (qz < D - 0.5)
    band = np.zeros(qx.shape, dtype=bool)
    for a in (qx, qy, qz):
        band |= np.abs(a - (np.floor(a) + 0.5)) < 1e-4
    nx = np.clip(np.floor(qx + 0.5), 0, W - 1).astype(np.int64)
    ny = np.clip(np.floor(qy + 0.5), 0, H - 1).astype(np.int64)
    nz = np.clip(np.floor(qz + 0.5), 0, D - 1).astype(np.int64)
    lab_o = np.where(inside, lab[nz, ny, nx], 0)
    if interp == 'nearest':
        val = img[:, nz, ny, nx]
    else:
        x0, y0, z0 = np.floor(qx), np.floor(qy), np.floor(qz)
        fx, fy, fz = qx - x0, qy - y0, qz - z0
        val = np.zeros((C,) + qx.shape)
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    w = (fx if cx else 1 - fx) * (fy if cy else 1 - fy) * (fz if cz else 1 - fz)
                    xi = np.clip(x0 + cx, 0, W - 1).astype(np.int64)
                    yi = np.clip(y0 + cy, 0, H - 1).astype(np.int64)
                    zi = np.clip(z0 + cz, 0, D - 1).astype(np.int64)
                    val += w * img[:, zi, yi, xi]
    return np.where(inside, val, 0.1), lab_o, val, band


def _check(got_img, got_lab, img, lab, q, interp='linear'):
    want_img, want_lab, inside_val, band = _resample(img.double().cpu().numpy(), lab.cpu().numpy(), q, interp)
    gi = got_img.double().cpu().numpy()
    err = np.abs(gi - want_img)
    # in the band the fp32 and fp64 coordinates may fall on different sides of the boundary: either side's value is right there
    err = np.where(band[None], np.minimum(err, np.minimum(np.abs(gi - inside_val), np.abs(gi - 0.1))), err)
    assert err.max() <= 5e-5, err.max()
    gl = got_lab.cpu().numpy()
    bad = (gl != want_lab) & ~band
    assert not bad.any(), int(bad.sum())
    assert band.mean() < 1e-3, band.mean()


# ---- exact cases -----------------------------------------------------------------------------------------------------------------
def test_identity_and_zero_bspline_are_bit_exact():
    from deepatlas_amd import ops
    from deepatlas_amd.lib import transforms as T
    img, lab = _volume((13, 17, 20), C=3)
    for tr in (T.RandomRigidTransform(ratio=1.0), T.RandomBSplineTransform(ratio=1.0, deform_scale=0.0, bspline_order=3)):
        for interp in ('linear', 'nearest'):
            tr.interpolator = interp
            out = tr({'image': img, 'segmentation': lab})
            assert out['image'] is not img and torch.equal(out['image'], img) and torch.equal(out['segmentation'], lab)
    a, b = ops.spatial_resample(img[None], lab[None], np.eye(3, 4)[None])
    assert torch.equal(a[0], img) and torch.equal(b[0], lab)


@pytest.mark.parametrize('shape', [(12, 16, 20), (9, 11, 13)])
def test_integer_translation_is_an_exact_shift(shape):
    from deepatlas_amd import ops
    img, lab = _volume(shape, C=2, seed=1)
    t = (3, -2, 5)                                               # (x, y, z): out[z, y, x] = in[z + 5, y - 2, x + 3]
    A = np.eye(3, 4)
    A[:, 3] = t
    a, b = ops.spatial_resample(img[None], lab[None], A[None])
    D, H, W = shape
    want_i = torch.full_like(img, 0.1)
    want_l = torch.zeros_like(lab)
    want_i[:, :D - 5, 2:, :W - 3] = img[:, 5:, :H - 2, 3:]
    want_l[:D - 5, 2:, :W - 3] = lab[5:, :H - 2, 3:]
    assert torch.equal(a[0], want_i) and torch.equal(b[0], want_l)


def test_quarter_turn_about_z():
    from deepatlas_amd import ops
    from deepatlas_amd.lib import transforms as T
    D, H, W = 10, 24, 24
    img, lab = _volume((D, H, W), seed=2)
    c = (W // 2, H // 2, D // 2)
    a, b = ops.spatial_resample(img[None], lab[None], T.rigid_index_affine((0, 0, np.pi / 2), (0, 0, 0), (1, 1, 1), c)[None])
    # R (i - c) + c with Rz(90): input x = cx - (y - cy), input y = cy + (x - cx)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    sx, sy = c[0] - (y - c[1]), c[1] + (x - c[0])
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    li, ll = img[0].cpu().numpy(), lab.cpu().numpy()
    want_l = np.where(ok, ll[z, np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], 0)
    want_i = np.where(ok, li[z, np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], np.float32(0.1))
    assert np.array_equal(b[0].cpu().numpy(), want_l)
    assert np.abs(a[0, 0].cpu().numpy() - want_i).max() <= 1e-5


# ---- against the fp64 oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,spacing,interp', [((37, 52, 45), (1.0, 1.0, 1.0), 'linear'), ((37, 52, 45), (1.0, 1.2, 2.0), 'linear'),
                                                  ((37, 52, 45), (1.0, 1.2, 2.0), 'nearest'), ((160, 192, 160), (1.0, 1.0, 1.0), 'linear')])
def test_random_rigid_against_fp64_oracle(shape, spacing, interp):
    from deepatlas_amd.lib import transforms as T
    img, lab = _volume(shape, C=2 if shape[0] < 100 else 1, seed=3)
    angles, trans = (20.0, 16.0, 24.0), (6.0, 4.0, 5.0)
    tr = T.RandomRigidTransform(ratio=1.0, rotation_angles=angles, translation=trans, interpolator=interp)
    np.random.seed(21)
    out = tr({'image': img, 'segmentation': lab, 'spacing': spacing})
    np.random.seed(21)                                           # the reference's draws, replayed
    np.random.rand(1)
    rad = [np.random.normal(0, angles[k] / 2) * np.pi / 180 for k in range(3)]
    t = [np.random.normal(0, trans[k] / 2) * spacing[k] for k in range(3)]
    D, H, W = shape
    q = _q_rigid(shape, rad, t, spacing, (W // 2, H // 2, D // 2))
    _check(out['image'], out['segmentation'], img, lab, q, interp)


@pytest.mark.parametrize('shape,mesh,order,spacing', [((37, 52, 45), (3, 3, 3), 1, (1.0, 1.0, 1.0)), ((37, 52, 45), (2, 4, 3), 1, (1.0, 1.2, 2.0)),
                                                      ((37, 52, 45), (3, 3, 3), 2, (1.0, 1.2, 2.0)), ((37, 52, 45), (2, 4, 3), 2, (1.0, 1.0, 1.0)),
                                                      ((37, 52, 45), (3, 3, 3), 3, (1.0, 1.0, 1.0)), ((37, 52, 45), (2, 4, 3), 3, (1.0, 1.2, 2.0)),
                                                      ((160, 192, 160), (3, 3, 3), 2, (1.0, 1.0, 1.0))])
def test_random_bspline_against_fp64_oracle(shape, mesh, order, spacing):
    from deepatlas_amd.lib import transforms as T
    img, lab = _volume(shape, C=2 if shape[0] < 100 else 1, seed=4)
    scale = 8.0
    tr = T.RandomBSplineTransform(mesh_size=mesh, bspline_order=order, deform_scale=scale, ratio=1.0)
    np.random.seed(33)
    out = tr({'image': img, 'segmentation': lab, 'spacing': spacing})
    n = 3 * int(np.prod(np.asarray(mesh) + order))
    np.random.seed(33)
    np.random.rand(1)
    p = np.random.normal(0, scale / 2, n)
    p[0:int(n / 3)] = 0
    q = _q_bspline(shape, p, mesh, order, spacing)
    assert np.abs(q - _index_grid(shape)).max() > 2                 # it does deform
    _check(out['image'], out['segmentation'], img, lab, q)


# ---- batching, determinism, modes, label dtypes ----------------------------------------------------------------------------------
def test_batch_of_three_equals_three_single_calls_and_reruns_are_identical():
    from deepatlas_amd.lib import transforms as T
    shape = (20, 24, 28)
    imgs = torch.stack([_volume(shape, seed=s)[0] for s in range(3)])
    labs = torch.stack([_volume(shape, seed=s)[1] for s in range(3)])
    for make in (lambda: T.RandomRigidTransform(ratio=1.0, rotation_angles=(20, 20, 20), translation=(3, 3, 3)),
                 lambda: T.RandomBSplineTransform(mesh_size=(2, 4, 3), bspline_order=3, deform_scale=6.0, ratio=0.7)):
        np.random.seed(5)
        batch = make()({'image': imgs, 'segmentation': labs})
        np.random.seed(5)
        again = make()({'image': imgs, 'segmentation': labs})
        np.random.seed(5)
        tr = make()
        singles = [tr({'image': imgs[k], 'segmentation': labs[k]}) for k in range(3)]
        assert torch.equal(batch['image'], again['image']) and torch.equal(batch['segmentation'], again['segmentation'])
        for k in range(3):
            assert torch.equal(batch['image'][k], singles[k]['image']) and torch.equal(batch['segmentation'][k], singles[k]['segmentation'])
        assert not torch.equal(batch['image'], imgs)


def test_modes_leave_the_other_tensor_untouched_and_int64_labels_match_uint8():
    from deepatlas_amd.lib import transforms as T
    img, lab = _volume((16, 20, 24), seed=6)
    keep_i, keep_l = img.clone(), lab.clone()
    kw = dict(ratio=1.0, rotation_angles=(30, 30, 30), translation=(4, 4, 4))
    np.random.seed(1)
    both = T.RandomRigidTransform(**kw)({'image': img, 'segmentation': lab})
    np.random.seed(1)
    o = T.RandomRigidTransform(mode='img', **kw)({'image': img, 'segmentation': lab})
    assert o['segmentation'] is lab and torch.equal(lab, keep_l) and torch.equal(o['image'], both['image'])
    np.random.seed(1)
    o = T.RandomRigidTransform(mode='seg', **kw)({'image': img, 'segmentation': lab})
    assert o['image'] is img and torch.equal(img, keep_i) and torch.equal(o['segmentation'], both['segmentation'])
    for dt in (torch.int64, torch.int32):
        np.random.seed(1)
        o = T.RandomRigidTransform(**kw)({'image': img, 'segmentation': lab.to(dt)})
        assert o['segmentation'].dtype == dt and torch.equal(o['segmentation'].to(torch.uint8), both['segmentation'])
        np.random.seed(1)
        o = T.RandomBSplineTransform(ratio=1.0, deform_scale=5.0)({'image': img, 'segmentation': lab.to(dt)})
        np.random.seed(1)
        u = T.RandomBSplineTransform(ratio=1.0, deform_scale=5.0)({'image': img, 'segmentation': lab})
        assert torch.equal(o['segmentation'].to(torch.uint8), u['segmentation']) and torch.equal(o['image'], u['image'])


def _two_steps(tmp_path, augment):
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                            data_root='./data', log_root=str(tmp_path), shape=[32, 32, 32])
    cfg = train_seg.build_config(ns)
    if augment:
        cfg['augment'] = augment
    exp = SegmentationExperiment(cfg)
    exp.setup_train()
    exp.initialize_model(exp.model, exp.optimizer, '')
    losses, inputs = [], []
    step = exp.train_step

    def recording_step(images, truths):
        inputs.append((images.detach().clone(), truths.clone()))
        loss, out = step(images, truths)
        losses.append(loss.item())
        return loss, out
    exp.train_step = recording_step
    exp.current_epoch = 1
    exp.train_one_epoch()
    return losses, inputs


def test_segmentation_experiment_trains_on_augmented_batches(tmp_path):
    plain, plain_in = _two_steps(tmp_path / 'a', None)
    aug, aug_in = _two_steps(tmp_path / 'b', [['rigid', {'rotation_angles': [10, 10, 10], 'translation': [4, 4, 4]}],
                                               ['bspline', {'deform_scale': 4.0, 'ratio': 1.0}]])
    assert len(plain) == len(aug) == 2 and all(np.isfinite(aug))
    assert aug != plain
    for (pi, pl), (ai, al) in zip(plain_in, aug_in):
        assert ai.is_cuda and ai.shape == pi.shape and al.shape == pl.shape and al.dtype == pl.dtype
        assert not torch.equal(ai.cpu(), pi.cpu())
