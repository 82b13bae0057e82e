"""Inputs, float64 references and tolerances of the instance-refinement tests (test_refine_reference.py on the CPU, test_gpu_refine.py on the
GPU).  Nothing here calls the code under test.

Definition (torch on the CPU; float64 is the reference, float32 the yardstick):
    loss(disp) = lambda_sim * oracle.losses.ncc_loss(F.grid_sample(moving, identity + disp, 'bilinear', 'zeros', align_corners=True), fixed)
               + lambda_reg * oracle.losses.bending_energy_loss(disp, **reg)
identity = linspace(-1, 1, extent) per axis (0 along an axis of extent 1: every coordinate samples index 0 there), disp N x 3 x D x H x W with
channels (x, y, z) = (W, H, D).  The gradient is autograd's; the update is Adam restated in float64 with the per-channel step
lr3[c] = lr_vox * 2 / (extent_c - 1) (0 for an extent of 1) and the gradient multiplied by grad_scale first (adam_step); test_refine_reference.py
shows that the restatement is torch.optim.Adam on grad_scale * loss when lr3 is isotropic.

Tolerances: affine_cases.bound_of -- FACTOR = 4 x the distance of the float32 torch evaluation of the SAME formula from float64 (rel_max: largest
error over largest reference entry), the floor TAPS x 2^-23 where that distance is zero -- measured per case here, not typed in.  The update
given the gradient is held to datapath_cases.adam_p_excess / TOL['adam'], the rule da_adam_step is held to.

Conditioning: the derivative of the trilinear sample jumps where a sample coordinate crosses an integer, so every case's coordinates are
nudged to stay NUDGE_TO = 2e-3 voxel from the lattice and test_refine_reference.py asserts the distance GUARD = 1e-4 (affine_cases.GUARD) in
float64.  The lattice fields (zero, whole-voxel translations) are the exception on purpose: they pin the derivative's side.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from affine_cases import FACTOR, TAPS, ULP32, GUARD, bound_of, rel_max            # noqa: F401  (the shared rule)
from datapath_cases import da_grid
from oracle import losses as ol

NUDGE_TO = 2e-3
BETAS, EPS = (0.9, 0.999), 1e-8

# ---- the launcher's grid, restated (refine.hip rf_blocks: both kernels) ------------------------------------------------------------------
BLOCK, GRID_CAP = 256, 2048


def rf_blocks(V):
    g = da_grid(V, BLOCK, GRID_CAP)
    return g // 8 * 8 if g >= 8 else g


def runs_second_trip(V):
    """some thread of the sweep over V voxels takes a second trip (with a grid that is a multiple of 8 each eighth of the volume is swept by grid / 8 workgroups)"""
    g = rf_blocks(V)
    return g * BLOCK < V


# name: (D x H x W, N, amplitudes in voxels (one per sample), shift (x, y, z) in voxels added to every sample, lambda_reg, what it is there for)
# (the 8-voxel field goes with the large volume: on an extent of 12 it would throw most of a sample out; the cases without a shift that the trajectory
# tests use are tapered towards the faces, smooth_field)
CASES = {
    '5x6x7':     ((5, 6, 7), 1, (0.3,), (0, 0, 0), 0.5, 'every tap on or next to a face; below one workgroup'),
    '1x9x40':    ((1, 9, 40), 1, (2.0,), (0, 0, 0), 0.0, 'an extent of 1 (the bending energy is not defined there: lambda_reg = 0)'),
    '12x20x36':  ((12, 20, 36), 3, (0.3, 2.0, 2.0), (0, 0, 0), 0.5, 'ragged batch (34 workgroups rounded down to 32), N > 1 in the NCC mean'),
    '65x90x90':  ((65, 90, 90), 1, (8.0,), (0, 0, 0), 0.5, '526 500 voxels: more than 2048 x 256 lanes, both sweeps run a second trip'),
    '16x16x24o': ((16, 16, 24), 1, (2.0,), (8.0, 0, 0), 0.5, 'a shift of a third of the width: about a third of the sample points leave the volume'),
}
SMALL = [n for n in CASES if n != '65x90x90']
TAPERED = ('5x6x7', '1x9x40', '12x20x36')
SEEDS = {'12x20x36': 13}             # a case's seed is its position in CASES unless pinned here (chosen so that the float64 trajectory leaves out <= 2 %)
LAMBDA_SIM = 0.7
assert runs_second_trip(65 * 90 * 90) and rf_blocks(65 * 90 * 90) == GRID_CAP          # the capped grid's second trip
assert runs_second_trip(12 * 20 * 36) and not runs_second_trip(16 * 16 * 24)            # 34 workgroups rounded down to 32: a ragged second trip


def half_extents(vol):
    D, H, W = vol
    return np.array([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0])


def lr3_of(lr_vox, vol):
    D, H, W = vol
    return tuple(lr_vox * 2.0 / (e - 1) if e > 1 else 0.0 for e in (W, H, D))


def identity(vol, dtype=torch.float64):
    """1 x 3 x D x H x W, channel (x, y, z): linspace(-1, 1, extent) per axis, 0 along an axis of extent 1"""
    ax = [torch.linspace(-1, 1, e, dtype=dtype) if e > 1 else torch.zeros(1, dtype=dtype) for e in vol]
    z, y, x = torch.meshgrid(ax[0], ax[1], ax[2], indexing='ij')
    return torch.stack([x, y, z], 0).unsqueeze(0)


def sample_coords(disp, vol):
    """float64 voxel coordinates N x 3 x D x H x W the warp samples at (grid_sample's unnormalisation of identity + disp)"""
    s = torch.from_numpy(half_extents(vol)).view(1, 3, 1, 1, 1)
    return (identity(vol) + disp.double() + 1.0) * s


def lattice_distance(disp, vol):
    """smallest distance of a sample coordinate from an integer, in voxels, over the axes of extent > 1"""
    q = sample_coords(disp, vol)
    keep = [c for c, e in enumerate((vol[2], vol[1], vol[0])) if e > 1]
    q = q[:, keep]
    return float((q - q.round()).abs().min())


def nudged(disp, vol):
    """the field with every sample coordinate closer than NUDGE_TO to an integer moved to that distance (on its own side), float32"""
    s = torch.from_numpy(np.maximum(half_extents(vol), 0.5)).view(1, 3, 1, 1, 1)
    q = sample_coords(disp, vol)
    r = q - q.round()
    side = torch.where(r < 0, -torch.ones_like(r), torch.ones_like(r))
    q = torch.where(r.abs() < NUDGE_TO, q.round() + side * NUDGE_TO, q)
    live = torch.tensor([e > 1 for e in (vol[2], vol[1], vol[0])]).view(1, 3, 1, 1, 1)
    return torch.where(live, q / s - 1.0 - identity(vol), disp.double()).float().contiguous()


def smooth_field(vol, amps, shift=(0, 0, 0), seed=0, noise=0.1, taper=False):
    """N x 3 x D x H x W float32, normalised units: a smooth field of amps[k] voxels plus `noise` x that of white noise plus a constant shift (voxels).
    taper: the smooth part falls to zero towards the faces (sin(pi (i + 1/2) / extent) per axis), so that no sample point leaves the volume by a whole
    voxel: such a point has no similarity gradient at all, and the trajectory tests may leave out only 2 % of their elements."""
    xn = identity(vol)[0]
    x, y, z = xn[0], xn[1], xn[2]
    s = torch.from_numpy(np.maximum(half_extents(vol), 0.5)).view(3, 1, 1, 1)
    live = torch.tensor([float(e > 1) for e in (vol[2], vol[1], vol[0])], dtype=torch.float64).view(3, 1, 1, 1)
    gen = torch.Generator().manual_seed(900 + seed)
    rows = []
    for k, amp in enumerate(amps):
        u = torch.stack([torch.sin(2.1 * y + 0.3 * k) * torch.cos(1.3 * z + 0.7 * x), torch.cos(1.7 * x - 0.2 * k) * torch.sin(0.9 * z + 0.4 + 1.1 * y),
                         torch.sin(1.1 * x + 0.8) * torch.cos(2.3 * y + 0.1 * k)], 0)
        if taper:
            t = [torch.sin(math.pi * (torch.arange(e, dtype=torch.float64) + 0.5) / e) if e > 1 else torch.ones(1, dtype=torch.float64) for e in vol]
            u = u * (t[0].view(-1, 1, 1) * t[1].view(1, -1, 1) * t[2].view(1, 1, -1))
        u = amp * (u + noise * torch.randn(u.shape, generator=gen, dtype=torch.float64)) + torch.tensor(shift, dtype=torch.float64).view(3, 1, 1, 1)
        rows.append(u * live / s)
    return torch.stack(rows).float().contiguous()


def sinusoid_image(vol, n, seed, phase=0.0, noise=0.02, wavelength=6.0):
    """N x 1 x D x H x W float32 in about [0, 1]: a band-limited sum of sinusoids (wavelengths of `wavelength` voxels and more) plus a little noise"""
    D, H, W = vol
    z, y, x = torch.meshgrid(torch.arange(D, dtype=torch.float64), torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    gen = torch.Generator().manual_seed(500 + seed)
    rows = []
    for k in range(n):
        img = torch.zeros(vol, dtype=torch.float64)
        for j in range(6):
            kv = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * 2.0 * (2 * math.pi / wavelength)
            ph = torch.rand(1, generator=gen, dtype=torch.float64) * 2 * math.pi
            img += torch.sin(kv[0] * x + kv[1] * y + kv[2] * z + ph + phase) / (1 + j)
        rows.append(0.5 + 0.2 * img)
    out = torch.stack(rows).unsqueeze(1)
    return (out + noise * torch.randn(out.shape, generator=torch.Generator().manual_seed(700 + seed), dtype=torch.float64)).float().contiguous()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(moving, fixed N x 1 x D x H x W, disp N x 3 x D x H x W): float32 CPU tensors, never modified by a test.  moving and fixed share their
    sinusoids up to a phase and their shortest wavelength is five times the largest displacement (at least 6 voxels), so NCC is well inside (0, 1)."""
    vol, n, amps, shift, _, _ = CASES[name]
    seed = SEEDS.get(name, list(CASES).index(name))
    wl = max(6.0, 5.0 * max(amps))
    return (sinusoid_image(vol, n, seed, wavelength=wl), sinusoid_image(vol, n, seed, phase=0.6, noise=0.03, wavelength=wl),
            nudged(smooth_field(vol, amps, shift, seed, taper=name in TAPERED), vol))


def reg_of(name):
    return CASES[name][4]


# ---- the formula -------------------------------------------------------------------------------------------------------------------------
def warp(moving, disp):
    grid = (identity(tuple(moving.shape[2:]), disp.dtype) + disp).permute(0, 2, 3, 4, 1)
    return F.grid_sample(moving, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def total_loss(moving, fixed, disp, lambda_sim, lambda_reg, reg=None):
    """(loss, 1 - NCC)"""
    sim = ol.ncc_loss(warp(moving, disp), fixed)
    loss = lambda_sim * sim
    if lambda_reg:
        loss = loss + lambda_reg * ol.bending_energy_loss(disp, **dict(reg or {}))
    return loss, sim


def stats_of(w, f):
    """da_ncc_fwd's rows N x 8 from the warped image and the fixed one (float64)"""
    n = w.shape[0]
    a, b = w.reshape(n, -1).double(), f.reshape(n, -1).double()
    ma, mb = a.mean(1), b.mean(1)
    cov = (a * b).mean(1) - ma * mb
    va, vb = (a * a).mean(1) - ma * ma, (b * b).mean(1) - mb * mb
    return torch.stack([ma, mb, cov, va, vb, cov / (va.sqrt() * vb.sqrt()), torch.full_like(ma, a.shape[1]), torch.zeros_like(ma)], 1)


def evaluate(moving, fixed, disp, dtype, lambda_sim=LAMBDA_SIM, lambda_reg=0.0, reg=None):
    """The formula in `dtype` on the CPU: dict(sim = 1 - NCC, grad = d loss / d disp, stats), all float64."""
    m, f = moving.detach().cpu().to(dtype), fixed.detach().cpu().to(dtype)
    u = disp.detach().cpu().to(dtype).requires_grad_(True)
    loss, sim = total_loss(m, f, u, lambda_sim, lambda_reg, reg)
    loss.backward()
    return dict(sim=sim.detach().double(), grad=u.grad.double(), stats=stats_of(warp(m, u.detach()), f))


@functools.lru_cache(maxsize=None)
def reference(name, with_reg=False):
    """float64 reference of a case (similarity gradient alone, or with the case's lambda_reg): computed once, shared, never modified"""
    return evaluate(*inputs(name), torch.float64, lambda_reg=reg_of(name) if with_reg else 0.0)


@functools.lru_cache(maxsize=None)
def grad_bound(name, with_reg=False):
    """the bound on rel_max(gradient): FACTOR x the float32 torch evaluation's distance from float64, floored (affine_cases.bound_of)"""
    got = evaluate(*inputs(name), torch.float32, lambda_reg=reg_of(name) if with_reg else 0.0)
    return bound_of(rel_max(got['grad'], reference(name, with_reg)['grad']))


@functools.lru_cache(maxsize=None)
def stats_bound(name):
    """Absolute bounds N x 6 on da_refine_moments' rows {mean_w, mean_f, cov, var_w, var_f, ncc}, from the rounding of their float32 inputs (the sums
    themselves are in double).  A warped voxel is eight float32 products and sums: it is within e_w = TAPS x 2^-23 x max|moving| of the exact sample, the
    floor of bound_of applied to one voxel; a fixed voxel enters as the float32 difference from the pivot, within e_f = 2^-23 x max|fixed|.  With the
    standard deviations s_w, s_f of the reference: |d mean_w| <= e_w, |d mean_f| <= e_f, |d cov| <= 2 (e_w s_f + e_f s_w), |d var_w| <= 4 e_w s_w,
    |d var_f| <= 4 e_f s_f (first order, doubled), and ncc = cov / (s_w s_f) moves by at most |d cov| / (s_w s_f) + |d var_w| / (2 s_w^2) +
    |d var_f| / (2 s_f^2) = 4 (e_w / s_w + e_f / s_f)."""
    mv, fx, _ = inputs(name)
    st = reference(name)['stats']
    n = mv.shape[0]
    e_w = TAPS * ULP32 * mv.reshape(n, -1).abs().max(1).values.double()
    e_f = ULP32 * fx.reshape(n, -1).abs().max(1).values.double()
    s_w, s_f = st[:, 3].sqrt(), st[:, 4].sqrt()
    return torch.stack([e_w, e_f, 2 * (e_w * s_f + e_f * s_w), 4 * e_w * s_w, 4 * e_f * s_f, 4 * (e_w / s_w + e_f / s_f)], 1)


# ---- lattice fields ----------------------------------------------------------------------------------------------------------------------
LATTICE_VOL, LATTICE_N = (5, 9, 17), 2              # (extent - 1) / 2 a power of two: a whole-voxel shift is exact in float32 (affine_cases.TRANSLATION_VOL)
LATTICE_SHIFTS = ((0, 0, 0), (3, -2, 1), (-1, 0, 2))


@functools.lru_cache(maxsize=None)
def lattice_inputs(k):
    vol = LATTICE_VOL
    s = torch.from_numpy(half_extents(vol)).view(1, 3, 1, 1, 1)
    disp = (torch.tensor(LATTICE_SHIFTS[k], dtype=torch.float64).view(1, 3, 1, 1, 1) / s).expand((LATTICE_N, 3) + vol).float().contiguous()
    return sinusoid_image(vol, LATTICE_N, 40 + k), sinusoid_image(vol, LATTICE_N, 40 + k, phase=0.5), disp


@functools.lru_cache(maxsize=None)
def lattice_bound(k):
    """the gradient bound of a lattice field by the same rule (both torch evaluations take the floor's side, and the coordinates are exact in either)"""
    got, ref = evaluate(*lattice_inputs(k), torch.float32), evaluate(*lattice_inputs(k), torch.float64)
    return bound_of(rel_max(got['grad'], ref['grad']))


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def adam_step(p, m, v, g, step, lr3, grad_scale, betas=BETAS, eps=EPS):
    """One Adam step (torch.optim.Adam's update, no weight decay, no amsgrad) in the dtype of p on N x 3 x ... tensors: the gradient is multiplied by
    grad_scale first, channel c steps by lr3[c].  The hyper-parameters are the float32 values the C ABI receives and the bias corrections are formed
    in double from those, as da_adam_step does (datapath_cases.adam_hyper: 1 - float32(0.999) is 4.7e-5 from 0.001).  Returns (p, m, v)."""
    b1, b2, eps, grad_scale = f32(betas[0]), f32(betas[1]), f32(eps), f32(grad_scale)
    lr = torch.tensor([f32(x) for x in lr3], dtype=p.dtype).view(1, 3, 1, 1, 1)
    gi = g * grad_scale
    m = b1 * m + (1 - b1) * gi
    v = b2 * v + (1 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps)), m, v


def adam_path(p0, grads, lr3, grad_scale):
    """float64 [(p, m, v)] after each of len(grads) steps from p0 with zero moments, as numpy arrays (datapath_cases.adam_p_excess's `path`)"""
    p = p0.double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for k, g in enumerate(grads):
        p, m, v = adam_step(p, m, v, g.double(), k + 1, lr3, grad_scale)
        out.append((p.numpy().copy(), m.numpy().copy(), v.numpy().copy()))
    return out


def twin(moving, fixed, disp0, dtype, iters, lr_vox, lambda_sim, lambda_reg, reg=None, grad_scale=None):
    """refine_field restated with torch on the CPU in `dtype`, computing its own gradients: dict(disp, hist [iters] = 1 - NCC before each update,
    grads = the list of gradients), float64."""
    vol = tuple(disp0.shape[2:])
    m_, f_ = moving.detach().cpu().to(dtype), fixed.detach().cpu().to(dtype)
    lr3 = lr3_of(lr_vox, vol)
    gs = float(np.prod(vol)) if grad_scale is None else grad_scale
    p = disp0.detach().cpu().to(dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hist, grads = [], []
    for k in range(iters):
        u = p.clone().requires_grad_(True)
        loss, sim = total_loss(m_, f_, u, lambda_sim, lambda_reg, reg)
        loss.backward()
        hist.append(float(sim.detach()))
        grads.append(u.grad.double())
        p, m, v = adam_step(p, m, v, u.grad, k + 1, lr3, gs)
    return dict(disp=p.double(), hist=torch.tensor(hist, dtype=torch.float64), grads=grads)


# ---- trajectory --------------------------------------------------------------------------------------------------------------------------
TRAJ_CASES = ('5x6x7', '1x9x40', '12x20x36', '16x16x24o')
TRAJ_ITERS, TRAJ_LR = 5, 0.1
MAX_LEFT_OUT = 0.02


@functools.lru_cache(maxsize=None)
def trajectory(name, iters=TRAJ_ITERS):
    """dict(ref, f32: the two twins; keep: the elements whose float64 gradient stays at or above the gradient bound (in units of the largest
    entry of that iteration's gradient) in every iteration; bound_disp, bound_hist)"""
    mv, fx, d0 = inputs(name)
    lam = reg_of(name)
    ref = twin(mv, fx, d0, torch.float64, iters, TRAJ_LR, LAMBDA_SIM, lam)
    f32 = twin(mv, fx, d0, torch.float32, iters, TRAJ_LR, LAMBDA_SIM, lam)
    gb = grad_bound(name, with_reg=True)
    keep = torch.ones_like(d0, dtype=torch.bool)
    for g in ref['grads']:
        keep &= g.abs() >= gb * float(g.abs().max())
    live = torch.tensor([e > 1 for e in (d0.shape[4], d0.shape[3], d0.shape[2])]).view(1, 3, 1, 1, 1).expand_as(keep)
    return dict(ref=ref, f32=f32, keep=keep, live=live, left_out=float((~keep & live).sum()) / float(live.sum()),
                bound_disp=bound_of(traj_dist(f32['disp'], ref['disp'], d0, keep)), bound_hist=bound_of(rel_max(f32['hist'], ref['hist'])))


def traj_dist(got, want, disp0, keep):
    """largest error of the refined field over the kept elements, in units of the largest update the reference made"""
    got, want = got.detach().cpu().double(), want.double()
    scale = float((want - disp0.double()).abs().max())
    return float((got - want).abs()[keep].max()) / (scale if scale > 0 else 1.0)


# ---- recovery ----------------------------------------------------------------------------------------------------------------------------
REC_VOL, REC_ITERS, REC_LR, REC_LAMBDA_REG, REC_AMP = (24, 28, 32), 60, 0.1, 5.0, 1.5


def _rec_fn(x, y, z):
    """an analytic band-limited image on voxel coordinates (wavelengths of 9 voxels and more)"""
    return (0.5 + 0.2 * torch.sin(0.55 * x + 0.3) * torch.cos(0.45 * y) + 0.15 * torch.sin(0.5 * z + 0.35 * y + 1.0) + 0.1 * torch.cos(0.6 * x - 0.4 * z)
            + 0.1 * torch.sin(0.3 * x + 0.35 * y + 0.4 * z))


def _rec_shears(x, y, z, inverse=False):
    """T = S3 o S2 o S1, three smooth shears (x += a(y, z); y += b(x, z); z += c(x, y)), each inverted exactly: together a smooth map about REC_AMP
    voxels from the identity with a closed-form inverse"""
    a = lambda y, z: 0.9 * torch.sin(0.21 * y + 0.4) * torch.cos(0.17 * z)
    b = lambda x, z: 0.9 * torch.cos(0.19 * x - 0.3) * torch.sin(0.23 * z + 0.2)
    c = lambda x, y: 0.9 * torch.sin(0.16 * x + 0.25 * y + 0.8)
    if not inverse:
        x = x + a(y, z)
        y = y + b(x, z)
        return x, y, z + c(x, y)
    z = z - c(x, y)
    y = y - b(x, z)
    return x - a(y, z), y, z


@functools.lru_cache(maxsize=None)
def recovery_inputs():
    """(moving, fixed, known field): fixed = fn on the grid, moving = fn o T^-1 on the grid (the same function evaluated through the known map), so
    that moving o T = fixed exactly in the continuum and T - identity is the field to recover (normalised units, float32)."""
    vol = REC_VOL
    D, H, W = vol
    z, y, x = torch.meshgrid(torch.arange(D, dtype=torch.float64), torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    tx, ty, tz = _rec_shears(x, y, z)
    known = torch.stack([tx - x, ty - y, tz - z], 0).unsqueeze(0) / torch.from_numpy(half_extents(vol)).view(1, 3, 1, 1, 1)
    fixed = _rec_fn(x, y, z).view((1, 1) + vol)
    moving = _rec_fn(*_rec_shears(x, y, z, inverse=True)).view((1, 1) + vol)
    return moving.float().contiguous(), fixed.float().contiguous(), known.float().contiguous()


def endpoint_error(disp, known):
    """mean endpoint error in voxels over the interior (two voxels in from every face)"""
    vol = tuple(known.shape[2:])
    s = torch.from_numpy(half_extents(vol)).view(1, 3, 1, 1, 1)
    e = ((disp.detach().cpu().double() - known.double()) * s).pow(2).sum(1).sqrt()
    return float(e[:, 2:-2, 2:-2, 2:-2].mean())


@functools.lru_cache(maxsize=None)
def recovery_twin():
    mv, fx, known = recovery_inputs()
    zero = torch.zeros_like(known)
    ref = twin(mv, fx, zero, torch.float64, REC_ITERS, REC_LR, 1.0, REC_LAMBDA_REG)
    f32 = twin(mv, fx, zero, torch.float32, REC_ITERS, REC_LR, 1.0, REC_LAMBDA_REG)
    after = float(total_loss(mv.double(), fx.double(), ref['disp'], 1.0, 0.0)[1])
    return dict(ref=ref, sim_before=float(ref['hist'][0]), sim_after=after, epe_before=endpoint_error(zero, known), epe_after=endpoint_error(ref['disp'], known),
                bound_hist=bound_of(rel_max(f32['hist'], ref['hist'])))
