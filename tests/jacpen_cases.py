"""Inputs and the float64 reference of the Jacobian folding penalty tests (test_jacpen_reference.py on the CPU, test_gpu_jacpen.py on the GPU).
Nothing here calls the code under test.

Definition: L = mean over all N V voxels of max(0, eps - det J)^p, det J of x -> x + u(x) with u_c = disp_c (size_c - 1) / 2 voxels and
numpy.gradient differences at unit spacing (central inside, one-sided on the faces; an axis of extent 1 has derivative zero) -- the
determinant of regeval_cases.jacobian_np.  Reference: that formula in torch on the CPU in float64 (torch.gradient per component and axis,
clamp(eps - det, min=0).pow(p).mean()) on the float32 input; its gradient comes from autograd.

Fields: regeval_cases.smooth_field(shape, n, sd, seed) + noise x randn (voxels, seeded generator) passed through to_normalised; the smooth
field alone does not fold at these sizes.  An axis of extent 1 has no normalised unit (size - 1 = 0, and its component is multiplied by 0):
there the field is built with the unit 1 for that axis, everything else the same (field()).

Guard band: the gradient of p = 1 jumps where det = eps, so a case is admissible only if NO voxel has |det64 - eps| <= the bound of
regeval_cases.jacobian_bound (4 x the float32 numpy evaluation's largest error on that field).  That is a condition on the inputs, asserted by
test_jacpen_reference.py; a seed that fails it is replaced, the rule is not.

Tolerances: the yardstick is the SAME formula evaluated in float32 on the CPU.  FP32_DISTANCE holds, per (case, eps, p), its distance from the
float64 result as measured when the cases were written: the loss's relative error and the gradient's max-norm error over the gradient's
largest magnitude.  The kernels get FACTOR = 4 x those distances (another association, FMA contraction, sums in double), but never less than
the floors LOSS_FLOOR = 5e-7 and GRAD_FLOOR = 1e-6.  The floors stand for the float32 arithmetic itself, where a recorded distance happens to
be smaller than it: an entry of J carries about three roundings (the scale, the difference, the 1 +), a term of det is a product of three
entries and det a sum of six terms whose magnitude exceeds eps - det, so a voxel's penalty is off by several units of 2^-24 = 6e-8 and the
mean keeps a part of that (measured float32 distances of the loss: 1e-9 - 2e-7); a gradient entry is a sum of up to seven cofactors, each a
difference of two rounded products of such entries, scaled twice -- about eight roundings, 8 x 2^-23 = 1e-6, against the largest entry
(measured: 3e-8 - 3e-7).  test_jacpen_reference.py re-measures the distances and checks that they still fit the bounds."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import regeval_cases as rc

LOSS_FLOOR, GRAD_FLOOR, FACTOR = 5e-7, 1e-6, 4.0
EPS_VALUES, POWERS = (0.0, 0.25), (1, 2)

# name: (D x H x W, N, standard deviation of the smooth field in voxels, standard deviation of the added noise in voxels, what it is there for)
# CASE_SEED: seed 0 wherever the guard band is empty with it; 33x47x61 had one or two voxels in the band at eps = 0.25 with the seeds 0 - 4
# and takes 5, the first seed that leaves it empty
CASES = {
    '2x2x2':    ((2, 2, 2), 1, 0.5, 0.3, 'every voxel on three faces: one-sided differences only, extent 2 (both neighbours of a row are faces)'),
    '2x3x5':    ((2, 3, 5), 2, 1.0, 0.3, 'every voxel on a face, batch 2'),
    '5x2x3':    ((5, 2, 3), 1, 1.0, 0.3, 'every voxel on a face, the short axis in the middle'),
    '1x4x6':    ((1, 4, 6), 1, 1.0, 0.3, 'an extent of 1: zero derivative along D, a scale of 0 for the z component'),
    '7x9x66':   ((7, 9, 66), 1, 1.5, 0.35, 'a row of 66 voxels crosses a wavefront'),
    '17x30x22': ((17, 30, 22), 3, 1.5, 0.35, 'ragged, batch 3: 11220 voxels, 43 workgroups (not a multiple of 8: the plain loop), the last one partly filled'),
    '33x47x61': ((33, 47, 61), 2, 1.5, 0.25, 'ragged, batch 2: 369 workgroups rounded down to 368, the XCD-contiguous split with ragged eighths'),
    '80x96x80': ((80, 96, 80), 1, 1.5, 0.3, '614400 voxels on the 2048 x 256 launch: the grid-stride loop runs more than once'),
}
IDS = list(CASES)
CASE_SEED = dict({name: 0 for name in IDS}, **{'33x47x61': 5})
COMBOS = [(name, eps, p) for name in IDS for eps in EPS_VALUES for p in POWERS]
COMBO_IDS = ['%s-eps%g-p%d' % c for c in COMBOS]

# float32-torch-vs-float64 distances (loss relative, gradient max norm over max |gradient|), measured on the CPU when the cases were written
FP32_DISTANCE = {
    ('2x2x2', 0.0, 1):           (5.76e-08, 7.36e-08),
    ('2x2x2', 0.0, 2):           (1.02e-07, 1.12e-07),
    ('2x2x2', 0.25, 1):          (8.29e-08, 1.07e-07),
    ('2x2x2', 0.25, 2):          (7.00e-08, 1.19e-07),
    ('2x3x5', 0.0, 1):           (7.95e-08, 1.24e-07),
    ('2x3x5', 0.0, 2):           (1.59e-08, 4.88e-08),
    ('2x3x5', 0.25, 1):          (1.37e-07, 1.24e-07),
    ('2x3x5', 0.25, 2):          (6.34e-08, 7.07e-08),
    ('5x2x3', 0.0, 1):           (6.33e-08, 5.22e-08),
    ('5x2x3', 0.0, 2):           (6.23e-08, 7.16e-08),
    ('5x2x3', 0.25, 1):          (5.96e-08, 5.16e-08),
    ('5x2x3', 0.25, 2):          (3.72e-08, 1.52e-07),
    ('1x4x6', 0.0, 1):           (8.89e-08, 4.00e-08),
    ('1x4x6', 0.0, 2):           (1.38e-07, 1.42e-07),
    ('1x4x6', 0.25, 1):          (1.69e-08, 4.00e-08),
    ('1x4x6', 0.25, 2):          (2.42e-07, 2.52e-07),
    ('7x9x66', 0.0, 1):          (3.07e-08, 1.05e-07),
    ('7x9x66', 0.0, 2):          (1.16e-08, 2.16e-07),
    ('7x9x66', 0.25, 1):         (2.22e-08, 1.05e-07),
    ('7x9x66', 0.25, 2):         (1.57e-08, 1.66e-07),
    ('17x30x22', 0.0, 1):        (8.24e-10, 9.91e-08),
    ('17x30x22', 0.0, 2):        (1.31e-08, 1.99e-07),
    ('17x30x22', 0.25, 1):       (1.07e-08, 9.91e-08),
    ('17x30x22', 0.25, 2):       (2.70e-08, 2.01e-07),
    ('33x47x61', 0.0, 1):        (6.86e-09, 1.33e-07),
    ('33x47x61', 0.0, 2):        (3.13e-08, 2.90e-07),
    ('33x47x61', 0.25, 1):       (3.02e-08, 1.46e-07),
    ('33x47x61', 0.25, 2):       (1.16e-07, 2.43e-07),
    ('80x96x80', 0.0, 1):        (6.80e-08, 1.92e-07),
    ('80x96x80', 0.0, 2):        (9.09e-08, 4.87e-07),
    ('80x96x80', 0.25, 1):       (2.05e-08, 2.17e-07),
    ('80x96x80', 0.25, 2):       (1.64e-07, 4.11e-07),
}


def bounds(name, eps, p):
    """(loss bound, gradient bound) of a combination: 4 x the recorded float32 distances, not below the floors."""
    l, g = FP32_DISTANCE[(name, eps, p)]
    return max(FACTOR * l, LOSS_FLOOR), max(FACTOR * g, GRAD_FLOOR)


@functools.lru_cache(maxsize=None)
def field(name):
    """The displacement field of a case: float32 N x 3 x D x H x W in normalised units (never modified by a test)."""
    shape, n, sd, noise, _ = CASES[name]
    seed = CASE_SEED[name]
    g = torch.Generator().manual_seed(1000 + seed)
    rough = noise * torch.randn((n, 3) + tuple(shape), generator=g, dtype=torch.float64)
    if min(shape) > 1:
        return (rc.smooth_field(shape, n, sd, seed) + rc.to_normalised(rough).float()).contiguous()
    # an extent of 1: smooth_field / to_normalised as they are written, with 2 / (size - 1) taken as 1 where size = 1
    D, H, W = shape
    gs = torch.Generator().manual_seed(seed)
    lattice = torch.randn((n, 3, 5, 6, 7), generator=gs, dtype=torch.float64)
    u = F.interpolate(lattice, size=tuple(shape), mode='trilinear', align_corners=True)
    u = u * (sd / float(u.std()))
    scale = torch.tensor([2.0 / (s - 1) if s > 1 else 1.0 for s in (W, H, D)], dtype=torch.float64).view(1, 3, 1, 1, 1)
    return ((u * scale).float() + (rough * scale).float()).contiguous()


def det_torch(disp):
    """det J, N x D x H x W in the dtype of disp (differentiable)."""
    _, _, D, H, W = disp.shape
    size, dim_of = (W, H, D), (3, 2, 1)          # component / derivative along x, y, z <-> dim W, H, D of an N x D x H x W tensor
    J = [[None] * 3 for _ in range(3)]
    for c in range(3):
        u = disp[:, c] * ((size[c] - 1) / 2.0)
        for a in range(3):
            g = torch.gradient(u, dim=dim_of[a])[0] if u.shape[dim_of[a]] > 1 else torch.zeros_like(u)
            J[c][a] = g + 1.0 if c == a else g
    return (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
            + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))


def penalty(disp, eps, p):
    """The definition, in the dtype of disp."""
    return (eps - det_torch(disp)).clamp(min=0).pow(p).mean()


def evaluate(disp, eps, p, dtype):
    """(loss, d loss / d disp) of the definition in `dtype` on the CPU (gradient by autograd), returned as (float, float64 tensor)."""
    x = disp.detach().cpu().to(dtype).requires_grad_(True)
    loss = penalty(x, eps, p)
    loss.backward()
    return float(loss.detach().double()), x.grad.double()


@functools.lru_cache(maxsize=None)
def reference(name, eps, p):
    """(loss, gradient) of a combination in float64: computed once, shared by the tests, never modified."""
    return evaluate(field(name), eps, p, torch.float64)


@functools.lru_cache(maxsize=None)
def det64(name):
    """det J of a case's field in float64 (numpy array N x D x H x W), from the torch reference."""
    with torch.no_grad():
        return det_torch(field(name).double()).numpy()


def numpy_field(name):
    """The field regeval_cases' numpy functions can take: numpy.gradient needs two samples per axis, so an axis of extent 1 is doubled (the
    derivative along it stays 0 and the determinant, expanded along that column (0, 0, 1), the same)."""
    f = field(name)
    for dim in (2, 3, 4):
        if f.shape[dim] == 1:
            f = torch.cat([f, f], dim=dim)
    return f


@functools.lru_cache(maxsize=None)
def guard_bound(name):
    """Half-width of the guard band around det = eps: regeval_cases.jacobian_bound's bound on this field."""
    return float(rc.jacobian_bound(numpy_field(name))[1])


def in_guard_band(name, eps):
    """Number of voxels of a case with |det64 - eps| <= guard_bound."""
    return int((np.abs(det64(name) - eps) <= guard_bound(name)).sum())


def folding_share(name, eps=0.0):
    """Share of the voxels with det64 < eps (eps = 0: folded)."""
    return float((det64(name) < eps).mean())


def rel_max(got, want):
    """max |got - want| / max |want| (the gradient's own scale)."""
    return float((got.double() - want).abs().max() / want.abs().max())


def measure_fp32(name, eps, p):
    """The float32 evaluation's distances from the float64 reference: (loss relative, gradient max norm over max |gradient|)."""
    l64, g64 = reference(name, eps, p)
    l32, g32 = evaluate(field(name), eps, p, torch.float32)
    return abs(l32 - l64) / abs(l64), rel_max(g32, g64)


# ---- descent -----------------------------------------------------------------------------------------------------------------------
# Plain gradient descent on the field of DESCENT_CASE with the penalty alone: disp <- disp - DESCENT_LR * d L / d disp, DESCENT_STEPS times.
# Chosen on the CPU: the float64 twin's loss falls at every step and its folding count (det <= 0) ends below a quarter of the first one
# (test_jacpen_reference.py asserts both); the device has to end below half of it.
DESCENT_CASE, DESCENT_EPS, DESCENT_POWER = '17x30x22', 0.0, 1
DESCENT_LR, DESCENT_STEPS = 20.0, 12


def descent_twin(dtype=torch.float64):
    """(losses before each step and after the last one, folding counts at the same points) of the descent in `dtype` on the CPU."""
    x = field(DESCENT_CASE).to(dtype)
    losses, folds = [], []
    for _ in range(DESCENT_STEPS + 1):
        l, g = evaluate(x, DESCENT_EPS, DESCENT_POWER, dtype)
        with torch.no_grad():
            folds.append(int((det_torch(x) <= 0).sum()))
        losses.append(l)
        x = x - DESCENT_LR * g.to(dtype)
    return losses, folds
