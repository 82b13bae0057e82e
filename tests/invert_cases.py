"""Inputs and the float64 references of the field-inversion tests (test_invert_reference.py on the CPU, test_gpu_invert.py on the GPU).
Nothing here calls the code under test.

Definition (conventions of warp.hip / invcons.hip: disp N x 3 x D x H x W, channels (x, y, z) = the (W, H, D) axes, normalised units,
s_c = (size_c - 1) / 2 converts to voxels, identity as warp_cases.identity):
    B[u](p) = F.grid_sample(u, p, 'bilinear', padding_mode='border', align_corners=True)
    v_0 = 0,  v_{k+1}(x) = -B[u](identity(x) + v_k(x)),  d_k(x) = |s (v_{k+1}(x) - v_k(x))|  (Euclidean norm, voxels)
    a voxel stops after applying the first update with d_k <= tol_vox, or after max_iters updates.
Points (N x P x 3, voxel index coordinates (x, y, z)): forward q = p + s B[u](p); inverse: the same iteration started at the point's
normalised coordinate index / (size - 1) * 2 - 1, x = q + s v.
Statistics per sample: the largest final update, the number of elements whose final update exceeds tol_vox, the number of updates performed,
the number of elements whose last sample point leaves [0, size - 1] on some axis.
Reference: that definition in torch on the CPU in float64 on the float32 inputs (`iterate`).

Fields: regeval_cases.smooth_field(shape, n, 1.0, seed) + 0.15 voxel of iid normal noise (seeded generator), scaled so that the Lipschitz bound
-- the largest Euclidean difference of the displacement between axis-adjacent voxels, in voxels, times sqrt(3) -- equals LIP (2e-6 below it,
so that the float32 rounding of the field cannot push it above); at 17x30x22 and 33x47x61 also the noise-free smooth field at LIP = 0.5, whose
displacements are larger.  The iteration is a contraction with constant <= LIP.

Conditions on the inputs, asserted by test_invert_reference.py (a seed that fails is replaced in CASE_SEED, the rule is not): the bound is
<= LIP; the float64 iteration's update after 32 updates is <= 1e-9 voxel.

The outside count is an integer that jumps where a sample coordinate crosses 0 or size - 1, so only elements whose float64 coordinate is
within warp_cases.DELTA of a face can be counted differently in float32: `near_face` counts them per sample, and a count may differ from the
reference's by at most that number.  On the three smallest shapes (EXACT_OUTSIDE) the seeds keep every coordinate DELTA away from the faces
and the counts agree exactly (asserted by the companion).  On the larger shapes no seed can: a smooth field puts thousands of face voxels'
coordinates within a fraction of a voxel of 0, about ten of them within DELTA at 80x96x80 whatever the seed.

Tolerance, the project's rule: FP32_DISTANCE[(case, LIP)] is the distance of the same iteration evaluated in float32 torch on the CPU from the
float64 result, the max norm of s (v32 - v64) in voxels, measured when the cases were written.  The kernels get FACTOR = 4 x that (another
association, FMA contraction), never below the floor 4 x warp_cases.COORD_ERR x (largest extent - 1) / 2 voxels.  Derivation of the floor:
the sample coordinate ((identity + v) + 1) / 2 * (size - 1) takes five roundings of at most 2^-24 on values of magnitude <= 2 in normalised
units, COORD_ERR (size - 1) / 2 = 3e-7 (size - 1) / 2 voxels (warp_cases.COORD_ERR); a coordinate error e moves the sampled displacement by at
most LIP e, and the fixed point of a contraction with constant LIP moves by at most e LIP / (1 - LIP) <= 4 e at LIP = 0.8, under the
amplification of at most 1 / (1 - LIP) = 5: 4 x COORD_ERR x (size - 1) / 2 covers it, and nothing below the float32 coordinate error can be
asked of a float32 kernel.  test_invert_reference.py re-measures the distances and asserts that they still fit."""
import functools
import math

import torch
import torch.nn.functional as F

import invcons_cases as ic
import regeval_cases as rc
import warp_cases as wc

FACTOR = 4.0
LIPS = (0.25, 0.5, 0.8)
NOISE_VOX = 0.15
CASES = ic.CASES
IDS = list(CASES)
CASE_SEED = {name: 0 for name in IDS}            # a seed that fails the conditions is replaced here
SMOOTH_IDS = ('17x30x22', '33x47x61')            # also the noise-free field at LIP 0.5
COMBOS = [(name, lip, 'noisy') for name in IDS for lip in LIPS] + [(name, 0.5, 'smooth') for name in SMOOTH_IDS]
COMBO_IDS = ['%s-lip%g-%s' % c for c in COMBOS]
SMALL_COMBOS = [c for c in COMBOS if c[0] != '80x96x80']
SMALL_IDS = ['%s-lip%g-%s' % c for c in SMALL_COMBOS]
MAX_ITERS = 32
TOLS = (1e-2, 1e-3)

# float32-torch-vs-float64 distance of the converged inverse in voxels, measured on the CPU when the cases were written
FP32_DISTANCE = {
    ('2x2x2', 0.25, 'noisy'): 5.32e-09, ('2x2x2', 0.5, 'noisy'): 9.96e-09, ('2x2x2', 0.8, 'noisy'): 9.13e-09,
    ('2x3x5', 0.25, 'noisy'): 1.84e-08, ('2x3x5', 0.5, 'noisy'): 2.66e-08, ('2x3x5', 0.8, 'noisy'): 4.67e-08,
    ('5x2x3', 0.25, 'noisy'): 7.70e-09, ('5x2x3', 0.5, 'noisy'): 2.49e-08, ('5x2x3', 0.8, 'noisy'): 4.11e-08,
    ('7x9x66', 0.25, 'noisy'): 9.41e-08, ('7x9x66', 0.5, 'noisy'): 2.15e-07, ('7x9x66', 0.8, 'noisy'): 2.96e-07,
    ('5x7x29', 0.25, 'noisy'): 4.06e-08, ('5x7x29', 0.5, 'noisy'): 9.27e-08, ('5x7x29', 0.8, 'noisy'): 1.79e-07,
    ('17x30x22', 0.25, 'noisy'): 1.81e-07, ('17x30x22', 0.5, 'noisy'): 3.10e-07, ('17x30x22', 0.8, 'noisy'): 4.79e-07,
    ('33x47x61', 0.25, 'noisy'): 4.23e-07, ('33x47x61', 0.5, 'noisy'): 8.96e-07, ('33x47x61', 0.8, 'noisy'): 1.50e-06,
    ('80x96x80', 0.25, 'noisy'): 8.40e-07, ('80x96x80', 0.5, 'noisy'): 2.29e-06, ('80x96x80', 0.8, 'noisy'): 3.18e-06,
    ('17x30x22', 0.5, 'smooth'): 2.89e-07, ('33x47x61', 0.5, 'smooth'): 1.05e-06,
}
# the rigid field: (float32-torch distance from the closed-form inverse in voxels, share of the voxels compared)
RIGID_FP32_DISTANCE = {
    '17x30x22': (7.59e-07, 0.046), '33x47x61': (9.50e-07, 0.127),           # (the float64 iteration: 1.2e-7 and 1.9e-7)
}


def scales(vol, dtype=torch.float64):
    D, H, W = vol
    return torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], dtype=dtype).view(1, 3, 1, 1, 1)


def lipschitz_bound(u):
    """largest Euclidean difference of the displacement (voxels) between axis-adjacent voxels, times sqrt(3); float64"""
    g = u.double() * scales(tuple(u.shape[2:]))
    steps = [g[:, :, 1:] - g[:, :, :-1], g[:, :, :, 1:] - g[:, :, :, :-1], g[..., 1:] - g[..., :-1]]
    return max(float(s.pow(2).sum(1).sqrt().max()) for s in steps if s.numel()) * math.sqrt(3.0)


def floor_vox(vol):
    return 4.0 * wc.COORD_ERR * (max(vol) - 1) / 2.0


def bound(name, lip, kind='noisy'):
    """the kernels' distance from the float64 inverse, voxels"""
    return max(FACTOR * FP32_DISTANCE[(name, lip, kind)], floor_vox(CASES[name][0]))


@functools.lru_cache(maxsize=None)
def field(name, lip, kind='noisy'):
    """float32 N x 3 x D x H x W, normalised units, Lipschitz bound lip (never modified by a test)"""
    shape, n, _ = CASES[name]
    seed = CASE_SEED[name]
    u = rc.smooth_field(shape, n, 1.0, seed).double()
    if kind == 'noisy':
        g = torch.Generator().manual_seed(1000 + seed)
        u = u + rc.to_normalised(NOISE_VOX * torch.randn((n, 3) + tuple(shape), generator=g, dtype=torch.float64))
    return (u * (lip * (1.0 - 2e-6) / lipschitz_bound(u))).float().contiguous()


def sample(u, p):
    """B[u](p): u N x 3 x D x H x W, p N x 3 x ... normalised coordinates (channel 0 = x), any trailing shape with three axes"""
    return F.grid_sample(u, p.permute(0, 2, 3, 4, 1), mode='bilinear', padding_mode='border', align_corners=True)


def voxel_coords(p, vol):
    """grid_sampler_unnormalize(align_corners=True) of normalised coordinates N x 3 x ..."""
    D, H, W = vol
    return (p + 1) / 2 * torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=p.dtype).view(1, 3, 1, 1, 1)


def iterate(u, base, dtype, max_iters=MAX_ITERS, tol_vox=0.0):
    """The definition from the normalised base coordinates `base` (N x 3 x A x B x C) in `dtype` on the CPU.  Returns a dict: v (float64, the
    result in normalised units), last (float64 N x A x B x C: the final update in voxels), iters (int64: updates performed), coords (float64:
    voxel coordinates of every element's last sample point)."""
    vol = tuple(u.shape[2:])
    u = u.detach().cpu().to(dtype)
    base = base.to(dtype)
    s = scales(vol, dtype)
    v = torch.zeros_like(base)
    active = torch.ones(base.shape[:1] + base.shape[2:], dtype=torch.bool)
    last = torch.zeros(active.shape, dtype=dtype)
    iters = torch.zeros(active.shape, dtype=torch.int64)
    at = base.clone()
    for _ in range(max_iters):
        if not bool(active.any()):
            break
        p = base + v
        nv = -sample(u, p)
        d = ((nv - v) * s).pow(2).sum(1).sqrt()
        a = active.unsqueeze(1)
        v = torch.where(a, nv, v)
        at = torch.where(a, p, at)
        last = torch.where(active, d, last)
        iters = iters + active.long()
        active = active & ~(d <= tol_vox)
    return dict(v=v.double(), last=last.double(), iters=iters, coords=voxel_coords(at.double(), vol))


def dense(u, dtype, max_iters=MAX_ITERS, tol_vox=0.0):
    """the dense inverse of a field: iterate from the identity grid of `dtype`"""
    vol = tuple(u.shape[2:])
    return iterate(u, wc.identity(vol, dtype).unsqueeze(0).expand(u.shape[0], -1, -1, -1, -1), dtype, max_iters, tol_vox)


def outside_count(coords, vol):
    """per sample: elements whose coordinate (N x 3 x ...) leaves [0, size - 1] on some axis"""
    D, H, W = vol
    hi = torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=coords.dtype).view(1, 3, 1, 1, 1)
    out = ((coords < 0) | (coords > hi)).any(1)
    return out.reshape(out.shape[0], -1).sum(1).double()


def face_distance(coords, vol):
    """the smallest distance of any coordinate component to 0 or size - 1, voxels"""
    D, H, W = vol
    hi = torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=coords.dtype).view(1, 3, 1, 1, 1)
    return float(torch.minimum(coords.abs(), (coords - hi).abs()).min())


EXACT_OUTSIDE = ('2x2x2', '2x3x5', '5x2x3')


def near_face(coords, vol):
    """per sample: elements with a coordinate component within warp_cases.DELTA of 0 or size - 1"""
    D, H, W = vol
    hi = torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=coords.dtype).view(1, 3, 1, 1, 1)
    near = (torch.minimum(coords.abs(), (coords - hi).abs()) < wc.DELTA).any(1)
    return near.reshape(near.shape[0], -1).sum(1).double()


def stats_of(res, vol, tol_vox):
    """float64 N x 4: what the kernels report, from an `iterate` result"""
    n = res['last'].shape[0]
    last = res['last'].reshape(n, -1)
    return torch.stack([last.max(1).values, (last > tol_vox).sum(1).double(), res['iters'].reshape(n, -1).sum(1).double(),
                        outside_count(res['coords'], vol)], 1)


@functools.lru_cache(maxsize=None)
def reference(name, lip, kind='noisy'):
    """the float64 inverse after MAX_ITERS updates at tol 0: computed once, shared by the tests, never modified"""
    return dense(field(name, lip, kind), torch.float64)


@functools.lru_cache(maxsize=None)
def masked_reference(name, lip, kind, tol_vox):
    return dense(field(name, lip, kind), torch.float64, MAX_ITERS, tol_vox)


def vox_distance(got, want):
    """max norm of s (got - want) in voxels; got / want N x 3 x D x H x W in normalised units"""
    vol = tuple(want.shape[2:])
    return float(((got.detach().cpu().double() - want.double()) * scales(vol)).abs().max())


def measure_fp32(name, lip, kind='noisy'):
    return vox_distance(dense(field(name, lip, kind), torch.float32)['v'], reference(name, lip, kind)['v'])


def early_exit_bound(tol_vox, lip):
    """A contraction with constant L whose last update was d is within d L / (1 - L) of its fixed point: |v* - v_{k+1}| <= sum_j L^j d."""
    return tol_vox * lip / (1.0 - lip)


# ---- rigid field: closed-form inverse ------------------------------------------------------------------------------------------------
RIGID_IDS = ('17x30x22', '33x47x61')
RIGID_ANGLES_DEG, RIGID_SHIFT_VOX = (8.0, -5.0, 6.0), (2.0, -1.5, 1.0)


def _rotation():
    ax, ay, az = (math.radians(a) for a in RIGID_ANGLES_DEG)
    rx = torch.tensor([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]], dtype=torch.float64)
    ry = torch.tensor([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]], dtype=torch.float64)
    rz = torch.tensor([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]], dtype=torch.float64)
    return rz @ ry @ rx


def _nodes(vol):
    """3 x D x H x W float64 voxel coordinates (x, y, z)"""
    D, H, W = vol
    zz, yy, xx = torch.meshgrid(torch.arange(D, dtype=torch.float64), torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    return torch.stack([xx, yy, zz])


@functools.lru_cache(maxsize=None)
def rigid(name):
    """(u float32 1 x 3 x D x H x W normalised, the closed-form inverse field float64 normalised, mask 1 x D x H x W of the voxels compared):
    y = R (x - c) + c + t in voxels, inverse x = R^T (y - c - t) + c; compared where the inverse point stays max |u| + 1 voxels inside."""
    vol = CASES[name][0]
    D, H, W = vol
    R, t = _rotation(), torch.tensor(RIGID_SHIFT_VOX, dtype=torch.float64).view(3, 1)
    c = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], dtype=torch.float64).view(3, 1)
    x = _nodes(vol).reshape(3, -1)
    u_vox = (R @ (x - c) + c + t - x).reshape(1, 3, D, H, W)
    inv_pt = R.t() @ (x - c - t) + c
    inv_vox = (inv_pt - x).reshape(1, 3, D, H, W)
    margin = float(u_vox.pow(2).sum(1).sqrt().max()) + 1.0
    hi = torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=torch.float64).view(3, 1)
    mask = ((inv_pt >= margin) & (inv_pt <= hi - margin)).all(0).reshape(1, D, H, W)
    u = (u_vox / scales(vol)).float().contiguous()
    return u, inv_vox / scales(vol), mask


def rigid_distance(got, name):
    """max norm in voxels of s (got - closed form) over the compared voxels"""
    _, inv, mask = rigid(name)
    e = ((got.detach().cpu().double() - inv) * scales(CASES[name][0])).abs()
    return float(e[mask.unsqueeze(1).expand_as(e)].max())


def rigid_bound(name):
    return FACTOR * RIGID_FP32_DISTANCE[name][0]


# ---- points --------------------------------------------------------------------------------------------------------------------------
POINT_CASES = [(name, n, P) for name in ('5x7x29', '17x30x22') for n in (1, 3) for P in (1, 63, 65, 1000)]
POINT_IDS = ['%s-n%d-P%d' % c for c in POINT_CASES]
POINT_LIP = 0.5


@functools.lru_cache(maxsize=None)
def point_field(name, n):
    """a field of batch n at the case's shape (the case's own generator, LIP 0.5)"""
    shape = CASES[name][0]
    u = rc.smooth_field(shape, n, 1.0, 7).double()
    g = torch.Generator().manual_seed(1007)
    u = u + rc.to_normalised(NOISE_VOX * torch.randn((n, 3) + tuple(shape), generator=g, dtype=torch.float64))
    return (u * (POINT_LIP * (1.0 - 2e-6) / lipschitz_bound(u))).float().contiguous()


@functools.lru_cache(maxsize=None)
def points(name, n, P, margin=0.0):
    """N x P x 3 float32 voxel coordinates, uniform over the volume widened by `margin` voxels on every side (negative: inside)"""
    D, H, W = CASES[name][0]
    g = torch.Generator().manual_seed(31 * P + n)
    hi = torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=torch.float64)
    return (-margin + torch.rand((n, P, 3), generator=g, dtype=torch.float64) * (hi + 2 * margin)).float()


def points_base(pts, vol, dtype):
    """N x P x 3 voxel coordinates -> N x 3 x 1 x 1 x P normalised base coordinates, index / (size - 1) * 2 - 1 in `dtype`"""
    D, H, W = vol
    size = torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=dtype)
    return (pts.to(dtype) / size * 2.0 - 1).permute(0, 2, 1).reshape(pts.shape[0], 3, 1, 1, pts.shape[1])


def transport_ref(u, pts, inverse, dtype=torch.float64, max_iters=MAX_ITERS, tol_vox=0.0):
    """float64 N x P x 3: the definition of the point transport"""
    vol = tuple(u.shape[2:])
    res = iterate(u, points_base(pts, vol, dtype), dtype, max_iters if inverse else 1, tol_vox if inverse else float('inf'))
    sv = (res['v'] * scales(vol)).reshape(pts.shape[0], 3, -1).permute(0, 2, 1)
    return pts.double() + sv if inverse else pts.double() - sv
