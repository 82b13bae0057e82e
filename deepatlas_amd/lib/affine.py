"""Affine pre-alignment of a pair of volumes: the stage every registration pipeline runs before the deformable one.

`theta` is N x 3 x 4 in the convention of torch.nn.functional.affine_grid(theta, size, align_corners=True): normalised coordinates, rows and
columns in (x, y, z) = (W, H, D) order, the frame of ops.WarpFn's deform.  It maps an OUTPUT point to the point of the source that is sampled
there (a pull-back, as lib/transforms.py rigid_index_affine does in index space), and it does not depend on the resolution: one theta
serves every level of a pyramid.  The warp and the gradient with respect to theta are HIP kernels (ops.AffineWarpFn, csrc/affine.hip);
building theta from 6 or 12 parameters, composing and inverting are a handful of torch operations on tiny device tensors.
"""
import functools

import torch
import torch.nn.functional as F

from .loss import NormalizedCrossCorrelationLoss, VoxelMorphLNCC, MutualInformationLoss
from .. import ops

AFFINE_MODES = ('rigid', 'affine')
N_PARAMS = {'rigid': 6, 'affine': 12}
SIM_LOSSES = {'ncc': NormalizedCrossCorrelationLoss, 'lncc': VoxelMorphLNCC, 'mi': MutualInformationLoss}
DEFAULT_LEVELS, DEFAULT_ITERS, DEFAULT_LR = (4, 2, 1), (60, 40, 20), 0.02
MIN_LEVEL_EXTENT = 8


@functools.lru_cache(maxsize=64)
def _half_extents(size, device, dtype):
    D, H, W = size
    return torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], dtype=dtype, device=device)


def half_extents(size, device=None, dtype=torch.float64):
    """s = ((W - 1) / 2, (H - 1) / 2, (D - 1) / 2) of a volume of `size` = (D, H, W): voxels per normalised unit, in (x, y, z) order.  The
    tensor is built once per (size, device) and shared (never modified): building it is a host-to-device copy, which the optimisation loop
    must not repeat."""
    D, H, W = (int(v) for v in size)
    if min(D, H, W) < 2:
        raise ValueError('an affine map in normalised coordinates needs >= 2 voxels per axis, got size %s' % ((D, H, W),))
    return _half_extents((D, H, W), None if device is None else str(device), dtype)


def _rotation_zxy(angles):
    """R = Rz Rx Ry of lib/transforms.py _rotation_zxy for a batch of angles N x 3 (x, y, z) in radians, with torch operations."""
    ax, ay, az = angles[:, 0], angles[:, 1], angles[:, 2]
    cx, sx, cy, sy, cz, sz = torch.cos(ax), torch.sin(ax), torch.cos(ay), torch.sin(ay), torch.cos(az), torch.sin(az)
    one, zero = torch.ones_like(ax), torch.zeros_like(ax)
    rx = torch.stack([one, zero, zero, zero, cx, -sx, zero, sx, cx], 1).reshape(-1, 3, 3)
    ry = torch.stack([cy, zero, sy, zero, one, zero, -sy, zero, cy], 1).reshape(-1, 3, 3)
    rz = torch.stack([cz, -sz, zero, sz, cz, zero, zero, zero, one], 1).reshape(-1, 3, 3)
    return rz @ rx @ ry


def rigid_theta(angles, translation_vox, size):
    """theta N x 3 x 4 of a rigid map of a volume of `size` = (D, H, W): rotation by `angles` N x 3 ((x, y, z), radians, the order of
    transforms._rotation_zxy) about the volume's centre, then a translation of `translation_vox` N x 3 voxels (x, y, z).  The rotation is one
    in VOXEL space: theta_lin = S^-1 R S with S = diag(s_x, s_y, s_z) (a rotation in the normalised coordinates of a non-cubic volume would
    be a shear), theta_3 = t / s.  In index space this is rigid_index_affine(angles, t, (1, 1, 1), ((W - 1) / 2, (H - 1) / 2, (D - 1) / 2)).
    Computed in float64 and returned in the dtype of `angles`; differentiable."""
    angles = torch.as_tensor(angles)
    if angles.dim() != 2 or angles.shape[1] != 3:
        raise ValueError('angles must be N x 3 (x, y, z) in radians, got %s' % (tuple(angles.shape),))
    t = torch.as_tensor(translation_vox, device=angles.device)
    if tuple(t.shape) != tuple(angles.shape):
        raise ValueError('translation_vox must be N x 3 matching the angles, got %s' % (tuple(t.shape),))
    s = half_extents(size, angles.device)
    R = _rotation_zxy(angles.double())
    lin = R * s.view(1, 1, 3) / s.view(1, 3, 1)
    return torch.cat([lin, (t.double() / s).unsqueeze(2)], 2).to(angles.dtype)


def theta_from_params(p, mode, size):
    """theta N x 3 x 4 from the optimiser's parameters p.  'rigid': N x 6 = (angles (x, y, z) in radians, translation (x, y, z) as a share
    of the half extent (size - 1) / 2, i.e. in normalised units) -- both of the order of 0.1 for a misalignment of a few degrees and voxels,
    so one learning rate fits all six; the map is rigid_theta(angles, translation x s, size).  'affine': N x 12, theta = I + p.view(3, 4).
    p = 0 is the identity in both modes."""
    if mode not in AFFINE_MODES:
        raise ValueError("mode must be one of %s, got %r" % (', '.join(AFFINE_MODES), mode))
    if p.dim() != 2 or p.shape[1] != N_PARAMS[mode]:
        raise ValueError("%s parameters must be N x %d, got %s" % (mode, N_PARAMS[mode], tuple(p.shape)))
    if mode == 'rigid':
        return rigid_theta(p[:, :3], p[:, 3:].double() * half_extents(size, p.device), size).to(p.dtype)
    eye = torch.eye(3, 4, dtype=p.dtype, device=p.device)
    return eye.unsqueeze(0) + p.reshape(-1, 3, 4)


def identity_theta(n, device=None, dtype=torch.float32):
    return torch.eye(3, 4, dtype=dtype, device=device).unsqueeze(0).repeat(int(n), 1, 1)


def _check_theta(theta, name='theta'):
    if theta.dim() != 3 or tuple(theta.shape[1:]) != (3, 4):
        raise ValueError('%s must be N x 3 x 4, got %s' % (name, tuple(theta.shape)))


def compose_theta(a, b):
    """The map x -> a(b(x)) of two thetas (N x 3 x 4 each), in float64, returned in the dtype of `a`.  For warps (pull-backs):
    AffineWarpFn(AffineWarpFn(src, a), b) samples src at a(b(x)), i.e. it is AffineWarpFn(src, compose_theta(a, b)) with one interpolation."""
    _check_theta(a, 'a')
    _check_theta(b, 'b')
    ad, bd = a.double(), b.double()
    lin = ad[:, :, :3] @ bd[:, :, :3]
    off = (ad[:, :, :3] @ bd[:, :, 3:]) + ad[:, :, 3:]
    return torch.cat([lin, off], 2).to(a.dtype)


def invert_theta(theta):
    """The inverse map of a theta N x 3 x 4 (adjugate over determinant of the 3 x 3 part, in float64), in the dtype of `theta`."""
    _check_theta(theta)
    t = theta.double()
    m = t[:, :, :3]
    c0 = torch.cross(m[:, 1], m[:, 2], dim=1)
    c1 = torch.cross(m[:, 2], m[:, 0], dim=1)
    c2 = torch.cross(m[:, 0], m[:, 1], dim=1)
    det = (m[:, 0] * c0).sum(1)
    inv = torch.stack([c0, c1, c2], 2) / det.view(-1, 1, 1)
    off = -(inv @ t[:, :, 3:])
    return torch.cat([inv, off], 2).to(theta.dtype)


def make_sim(sim='ncc', sim_settings=None, device=None):
    if sim not in SIM_LOSSES:
        raise ValueError("sim must be one of %s, got %r" % (', '.join(sorted(SIM_LOSSES)), sim))
    return SIM_LOSSES[sim](**dict(sim_settings or {})).to(device)


def check_schedule(levels, iters):
    """(levels, iters) as tuples of ints: pooling factors >= 1 and fixed iteration counts >= 0, one per level."""
    levels, iters = tuple(levels), tuple(iters)
    if not levels or len(levels) != len(iters):
        raise ValueError('levels and iters must be sequences of one length >= 1, got %r and %r' % (levels, iters))
    for f in levels:
        if isinstance(f, bool) or int(f) != f or f < 1:
            raise ValueError('a pyramid level is a pooling factor >= 1, got %r' % (f,))
    for k in iters:
        if isinstance(k, bool) or int(k) != k or k < 0:
            raise ValueError('an iteration count is an integer >= 0, got %r' % (k,))
    return tuple(int(f) for f in levels), tuple(int(k) for k in iters)


def pyramid_levels(size, levels, iters, min_extent=MIN_LEVEL_EXTENT):
    """[(factor, iterations)] of the levels that run on a volume of `size`: a level whose pooled extent would fall below `min_extent` on
    some axis is skipped (factor 1 always runs)."""
    return [(f, k) for f, k in zip(levels, iters) if f == 1 or min(int(v) // f for v in size) >= min_extent]


def affine_register(moving, fixed, mode='rigid', sim='ncc', sim_settings=None, levels=DEFAULT_LEVELS, iters=DEFAULT_ITERS, lr=DEFAULT_LR,
                    init=None, return_params=False):
    """Finds the theta (N x 3 x 4 float32, on the device) that aligns `moving` to `fixed` (both N x 1 x D x H x W float32 on the GPU):
    AffineWarpFn(moving, theta) is the pre-aligned moving image.  mode 'rigid' (6 parameters) or 'affine' (12); sim 'ncc' | 'lncc' | 'mi'
    with `sim_settings` the constructor arguments of that loss, as config['sim_loss'] / config['sim_settings'] of the experiments.

    Coarse to fine over `levels` (pooling factors, F.avg_pool3d, built once per pair) with `iters` Adam iterations each; theta is
    resolution-independent, so the parameters simply carry over.  A pooled level's voxel centres sit half a coarse voxel off the
    align_corners=True frame (its corner voxels' centres are not the fine volume's corner centres), so the coarse levels only initialise:
    the last level, factor 1, is exact.  A level whose pooled extent would fall below 8 voxels is skipped.  The learning rate of a level
    is lr x factor / (the coarsest factor that runs): the first level steps by lr, then the steps shrink with the voxels.
    Per level: torch.optim.Adam on the N x 6 (N x 12) device parameter tensor, AffineWarpFn -> the similarity kernel, fixed iteration
    counts and no host synchronisation inside the loop.  Every sample has its own parameters; the loss is the sum over the samples (the
    batch mean of the similarity times N), so a sample's trajectory does not depend on the batch it is in for the per-sample
    similarities (NCC, MI).
    init: a theta N x 3 x 4 to start from; the parameters then describe the map applied BEFORE it, theta = compose_theta(init, theta(p)).
    return_params: (theta, p)."""
    if moving.shape != fixed.shape or moving.dim() != 5 or moving.shape[1] != 1:
        raise ValueError('affine_register expects two N x 1 x D x H x W volumes of one shape, got %s and %s' % (tuple(moving.shape), tuple(fixed.shape)))
    if moving.dtype != torch.float32 or fixed.dtype != torch.float32:
        raise ValueError('affine_register expects float32 volumes')
    if mode not in AFFINE_MODES:
        raise ValueError("mode must be one of %s, got %r" % (', '.join(AFFINE_MODES), mode))
    levels, iters = check_schedule(levels, iters)
    ops.nat.require_cuda(moving, fixed)
    dev = moving.device
    N = moving.shape[0]
    size = tuple(int(v) for v in moving.shape[2:])
    crit = make_sim(sim, sim_settings, dev)
    if init is not None:
        _check_theta(init, 'init')
        init = init.detach().to(dev, torch.float32)
    moving, fixed = moving.detach(), fixed.detach()
    p = torch.zeros((N, N_PARAMS[mode]), dtype=torch.float32, device=dev, requires_grad=True)
    run = pyramid_levels(size, levels, iters)
    top = max(f for f, _ in run) if run else 1
    with torch.enable_grad():
        for f, n_iter in run:
            if n_iter == 0:
                continue
            m = moving if f == 1 else F.avg_pool3d(moving, f)
            t = fixed if f == 1 else F.avg_pool3d(fixed, f)
            opt = torch.optim.Adam([p], lr=lr * f / top)
            for _ in range(n_iter):
                opt.zero_grad(set_to_none=True)
                theta = theta_from_params(p, mode, size)
                if init is not None:
                    theta = compose_theta(init, theta)
                loss = crit(ops.AffineWarpFn.apply(m, theta), t) * float(N)
                loss.backward()
                opt.step()
    with torch.no_grad():
        theta = theta_from_params(p, mode, size)
        if init is not None:
            theta = compose_theta(init, theta)
        theta = theta.detach().contiguous()
    return (theta, p.detach()) if return_params else theta


def corner_error_vox(theta, theta_ref, size):
    """Largest distance, in voxels, between the points two thetas (N x 3 x 4) send the eight corners of a volume of `size` to: float64 [N]."""
    s = half_extents(size, theta.device)
    c = torch.tensor([[x, y, z, 1.0] for z in (-1.0, 1.0) for y in (-1.0, 1.0) for x in (-1.0, 1.0)], dtype=torch.float64, device=theta.device)
    d = (theta.double() - theta_ref.double().to(theta.device)) @ c.t()              # N x 3 x 8, normalised
    return (d * s.view(1, 3, 1)).norm(dim=1).max(dim=1).values
