"""Inputs and the float64 reference of the affine pre-alignment tests (test_affine_reference.py on the CPU, test_gpu_affine.py on the GPU).
Nothing here calls the code under test.

Definition: theta N x 3 x 4 in the convention of F.affine_grid(theta, size, align_corners=True) (normalised coordinates, (x, y, z) =
(W, H, D) order), and
    out = F.grid_sample(src, F.affine_grid(theta, src.shape, align_corners=True), 'bilinear', 'zeros', align_corners=True)
Reference: that expression in torch on the CPU in float64 on the float32 inputs; d_theta = autograd's gradient of sum(g * out) for a random
cotangent g.  The compose kernel's reference is its formula in float64: out(x) = theta (x_n + disp(x), 1) - x_n with x_n the normalised
identity coordinate of voxel x.

Tolerance: the project's usual rule, no fixed constants.  measure_fp32(case, kind) evaluates the SAME torch expression in float32 on the
CPU and takes its distances from the float64 result (relative max norm per output, invcons_cases.rel_max); the kernel may be at most
FACTOR = 4 x that far from float64 (the margin of mi_cases.py).  Where the float32 torch distance is exactly zero the bound is the floor:
one float32 ulp of the output's largest entry times the tap count, 8 x 2^-23 in the relative metric.

Conditioning: the derivative of the trilinear sample jumps where a sample coordinate crosses an integer.  A (case, kind) is admissible only
if NO sample coordinate lies within GUARD = 1e-4 voxel of an integer in float64 (lattice_distance); test_affine_reference.py asserts it for
every pinned combination.  That is a condition on the inputs: a combination that fails it gets another NUDGE (a shift of 0.0137 voxel per
unit, pinned below), the rule stays.  Generic matrices cannot meet it on the 589 824-voxel case (its 1.8 million coordinates are
equidistributed modulo 1), so that case takes the 'dyadic' kinds only: index-space matrices whose entries are multiples of 1 / 16 (applied to
half-integers: multiples of 1 / 32) and whose offsets are an odd multiple of 1 / 64, so that every coordinate is 1 / 64 from the nearest
multiple of 1 / 32, up to the float32 rounding of theta (3e-6 voxel).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

FACTOR = 4.0
TAPS = 8
ULP32 = 2.0 ** -23
GUARD = 1e-4

# name: (D x H x W, N, C, what it is there for)
CASES = {
    '5x6x7':    ((5, 6, 7), 3, 1, 'batch 3, every extent different'),
    '4x9x13':   ((4, 9, 13), 2, 3, 'odd W, the channel loop'),
    '2x2x2':    ((2, 2, 2), 1, 1, 'every tap on a border'),
    '6x5x9':    ((6, 5, 9), 5, 2, 'ragged batch of 5'),
    '96x96x64': ((96, 96, 64), 1, 1, '589 824 voxels: more than 2048 x 256 threads, the grid-stride sweep runs a second time'),
}
KINDS = ('rigid', 'affine', 'outside')
BIG_KINDS = ('dyadic', 'dyadic_outside')
COMBOS = [(name, kind) for name in CASES for kind in (BIG_KINDS if name == '96x96x64' else KINDS)]
COMBO_IDS = ['%s-%s' % c for c in COMBOS]
# shifts of 0.0137 voxel that move a combination off the lattice guard band (0 unless listed)
NUDGE = {('5x6x7', 'rigid'): 4, ('5x6x7', 'affine'): 1, ('5x6x7', 'outside'): 3, ('4x9x13', 'rigid'): 4, ('4x9x13', 'affine'): 1,
         ('4x9x13', 'outside'): 10, ('2x2x2', 'affine'): 1, ('6x5x9', 'rigid'): 4, ('6x5x9', 'affine'): 1}


def half_extents(vol):
    D, H, W = vol
    return np.array([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0])


def rotation_zxy(angles):
    """R = Rz Rx Ry, angles (x, y, z) in radians: the order of lib/transforms.py _rotation_zxy, written out again."""
    ax, ay, az = angles
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def rigid_theta_ref(angles_deg, trans_vox, vol):
    """[S^-1 R S | t / s] in float64 (numpy), the voxel-space rotation about the volume's centre in normalised coordinates."""
    s = half_extents(vol)
    R = rotation_zxy([a * math.pi / 180 for a in angles_deg])
    th = np.empty((3, 4))
    th[:, :3] = R * s[None, :] / s[:, None]
    th[:, 3] = np.asarray(trans_vox, dtype=np.float64) / s
    return th


def index_theta(A, b, vol):
    """theta of the index-space map q = A (i - s) + s + b (centred: s the half extents)."""
    s = half_extents(vol)
    th = np.empty((3, 4))
    th[:, :3] = np.asarray(A, dtype=np.float64) * s[None, :] / s[:, None]
    th[:, 3] = np.asarray(b, dtype=np.float64) / s
    return th


def make_theta(vol, n, kind, nudge=0):
    """float32 N x 3 x 4; sample k differs from sample 0 by a small rotation / offset so that a batch holds different maps."""
    small = 0.25 if min(vol) < 4 else 1.0                      # a 2-voxel volume keeps some samples inside
    shift = 0.0137 * nudge
    rows = []
    for k in range(n):
        if kind == 'rigid':
            th = rigid_theta_ref((7.0 + 1.5 * k, -4.0 - 0.8 * k, 11.0 + 0.6 * k),
                                 (small * (1.3 + 0.37 * k) + shift, small * (-0.7 - 0.21 * k) + shift, small * (2.1 - 0.29 * k) + shift), vol)
        elif kind == 'affine':
            s = half_extents(vol)
            th = np.array([[0.9 + 0.01 * k, 0.05, -0.02, 0.03],
                           [-0.03, 1.15 - 0.01 * k, 0.05, -0.02],
                           [0.05, 0.02, 1.05, 0.04]], dtype=np.float64)
            th[:, 3] += shift / s
        elif kind == 'outside':
            th = rigid_theta_ref((3.0 + 0.5 * k, 2.0, -2.5 - 0.4 * k), (shift, 0.17 + shift, -0.23 + shift), vol)
            th[0, 3] += 2.0 / 3.0                              # a third of the volume's width: those samples leave it
        elif kind == 'dyadic':
            th = index_theta([[15 / 16, 1 / 16, 0], [-1 / 16, 9 / 8, 1 / 16], [1 / 16, 0, 1]], (1 + 1 / 64 + k, -2 - 1 / 64, 0.5 + 1 / 64), vol)
        elif kind == 'dyadic_outside':
            th = index_theta([[1, 1 / 16, 0], [0, 1, -1 / 16], [1 / 16, 0, 1]], ((vol[2] - 1) / 3.0 + 1 / 64, 0.5 + 1 / 64, -1 - 1 / 64), vol)
        else:
            raise KeyError(kind)
        rows.append(th)
    return torch.from_numpy(np.stack(rows)).float().contiguous()


@functools.lru_cache(maxsize=None)
def inputs(name, kind):
    """(src N x C x D x H x W, theta N x 3 x 4, g like src): float32 CPU tensors, never modified by a test."""
    vol, n, c, _ = CASES[name]
    gen = torch.Generator().manual_seed(17 + 31 * list(CASES).index(name))
    src = torch.randn((n, c) + vol, generator=gen)
    g = torch.randn((n, c) + vol, generator=gen)
    return src, make_theta(vol, n, kind, NUDGE.get((name, kind), 0)), g


def sample_coords(theta, vol):
    """float64 voxel coordinates N x D x H x W x 3 (x, y, z) the warp samples at: grid_sample's unnormalisation of affine_grid's grid."""
    n = theta.shape[0]
    grid = F.affine_grid(theta.double(), (n, 1) + tuple(vol), align_corners=True)
    return (grid + 1.0) / 2.0 * torch.from_numpy(2.0 * half_extents(vol))


def lattice_distance(theta, vol):
    """smallest distance of a sample coordinate from an integer, in voxels (float64)"""
    q = sample_coords(theta, vol)
    return float((q - q.round()).abs().min())


def warp(src, theta):
    grid = F.affine_grid(theta, list(src.shape), align_corners=True)
    return F.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def evaluate(src, theta, g, dtype):
    """The torch expression in `dtype` on the CPU: dict(out, d_theta), both float64."""
    th = theta.detach().cpu().to(dtype).requires_grad_(True)
    out = warp(src.detach().cpu().to(dtype), th)
    (out * g.detach().cpu().to(dtype)).sum().backward()
    return dict(out=out.detach().double(), d_theta=th.grad.double())


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """float64 reference of a combination: computed once, shared by the tests, never modified."""
    return evaluate(*inputs(name, kind), torch.float64)


def rel_max(got, want):
    """max |got - want| / max |want| (invcons_cases.rel_max); where the reference is zero everywhere, the absolute distance."""
    scale = float(want.abs().max())
    return float((got.detach().cpu().double() - want).abs().max()) / (scale if scale > 0 else 1.0)


def bound_of(fp32_distance):
    """FACTOR x the float32 torch distance; the floor TAPS x one float32 ulp (relative to the largest entry) where that distance is zero."""
    return FACTOR * fp32_distance if fp32_distance > 0 else TAPS * ULP32


@functools.lru_cache(maxsize=None)
def measure_fp32(name, kind):
    """{'out': d, 'd_theta': d}: the float32 CPU evaluation's distances from the float64 reference."""
    ref = reference(name, kind)
    got = evaluate(*inputs(name, kind), torch.float32)
    return {k: rel_max(got[k], ref[k]) for k in ('out', 'd_theta')}


def bounds(name, kind):
    return {k: bound_of(v) for k, v in measure_fp32(name, kind).items()}


def d_theta_per_sample(got, want):
    """rel_max of d_theta per sample: [N] floats (each sample against its own largest entry)"""
    return [rel_max(got[k], want[k]) for k in range(want.shape[0])]


# ---- the compose kernel --------------------------------------------------------------------------------------------------------------
def identity_norm(vol, dtype=torch.float64):
    """x_n: 1 x 3 x D x H x W, channel (x, y, z), linspace(-1, 1, size) per axis"""
    D, H, W = vol
    z, y, x = torch.meshgrid(torch.linspace(-1, 1, D, dtype=dtype), torch.linspace(-1, 1, H, dtype=dtype), torch.linspace(-1, 1, W, dtype=dtype),
                             indexing='ij')
    return torch.stack([x, y, z], 0).unsqueeze(0)


def compose_ref(theta, disp, vol, dtype=torch.float64):
    """out(x) = theta (x_n + disp(x), 1) - x_n in `dtype`: N x 3 x D x H x W"""
    th = theta.detach().cpu().to(dtype)
    xn = identity_norm(vol, dtype)
    p = xn if disp is None else xn + disp.detach().cpu().to(dtype)
    p = p.expand(th.shape[0], -1, -1, -1, -1)
    out = torch.einsum('nkj,njdhw->nkdhw', th[:, :, :3], p) + th[:, :, 3].view(-1, 3, 1, 1, 1)
    return out - xn


def smooth_disp(vol, n, amp_vox=2.0):
    """A smooth displacement field of `amp_vox` voxels, N x 3 x D x H x W float32 in normalised units."""
    xn = identity_norm(vol)
    x, y, z = xn[0, 0], xn[0, 1], xn[0, 2]
    s = torch.from_numpy(half_extents(vol)).view(3, 1, 1, 1)
    rows = []
    for k in range(n):
        u = torch.stack([torch.sin(2.1 * y + 0.3 * k) * torch.cos(1.3 * z), torch.cos(1.7 * x - 0.2 * k) * torch.sin(0.9 * z + 0.4),
                         torch.sin(1.1 * x + 0.8) * torch.cos(2.3 * y + 0.1 * k)], 0)
        rows.append(amp_vox * u / s)
    return torch.stack(rows).float().contiguous()


# ---- whole-voxel translation ---------------------------------------------------------------------------------------------------------
# theta is float32: a shift of t voxels is the entry 2 t / (size - 1), exact only where (size - 1) / 2 is a power of two
TRANSLATION_VOL, TRANSLATION_SHIFT = (5, 9, 17), (3, -2, 1)          # D x H x W; shift (x, y, z) in voxels: 3 / 8, -2 / 4, 1 / 2


def translation_theta(n=1):
    s = half_extents(TRANSLATION_VOL)
    th = np.tile(np.eye(3, 4), (n, 1, 1))
    th[:, :, 3] = np.asarray(TRANSLATION_SHIFT, dtype=np.float64) / s
    return torch.from_numpy(th).float()


def shifted(src, shift):
    """out[..., d, h, w] = src[..., d + tz, h + ty, w + tx], zeros where that leaves the volume (exact copy)"""
    tx, ty, tz = shift
    out = torch.zeros_like(src)
    D, H, W = src.shape[-3:]

    def rng(t, size):
        return slice(max(0, -t), min(size, size - t)), slice(max(0, t), min(size, size + t))
    (dz, sz), (dy, sy), (dx, sx) = rng(tz, D), rng(ty, H), rng(tx, W)
    out[..., dz, dy, dx] = src[..., sz, sy, sx]
    return out


# ---- the optimiser's twin ------------------------------------------------------------------------------------------------------------
TWIN_VOL, TWIN_N, TWIN_STEPS, TWIN_LR = (24, 28, 32), 2, 3, 0.02


def ncc_loss(x, y):
    """1 - NCC per sample, mean over the batch (lib/loss.py NormalizedCrossCorrelationLoss), in the dtype of the inputs"""
    n = x.shape[0]
    a, b = x.reshape(n, -1), y.reshape(n, -1)
    a, b = a - a.mean(1, keepdim=True), b - b.mean(1, keepdim=True)
    ncc = (a * b).sum(1) / ((a * a).sum(1) * (b * b).sum(1)).sqrt()
    return (1.0 - ncc).mean()


def blob_volume(vol, n, seed=0):
    """Smooth, asymmetric test images N x 1 x D x H x W float32 in [0, 1]: a few Gaussian blobs per sample."""
    xn = identity_norm(vol)[0]
    gen = torch.Generator().manual_seed(100 + seed)
    rows = []
    for _ in range(n):
        img = torch.zeros(vol, dtype=torch.float64)
        for _b in range(5):
            c = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * 1.0
            w = 0.25 + 0.2 * torch.rand(1, generator=gen, dtype=torch.float64)
            img += torch.exp(-((xn[0] - c[0]) ** 2 + (xn[1] - c[1]) ** 2 + (xn[2] - c[2]) ** 2) / (2 * w * w))
        rows.append(img / img.max())
    return torch.stack(rows).unsqueeze(1).float().contiguous()


def twin_register(moving, fixed, theta_fn, dtype, steps=TWIN_STEPS, lr=TWIN_LR):
    """`steps` Adam iterations at full resolution on the rigid parameters, the loop of affine_register(levels=(1,)) restated with torch on
    the CPU in `dtype`: p -> theta_fn(p) -> affine_grid + grid_sample -> NCC (summed over the samples) -> Adam.  Returns p (float64)."""
    m, f = moving.detach().cpu().to(dtype), fixed.detach().cpu().to(dtype)
    n = m.shape[0]
    p = torch.zeros((n, 6), dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        loss = ncc_loss(warp(m, theta_fn(p)), f) * float(n)
        loss.backward()
        opt.step()
    return p.detach().double()
