"""Inputs and the float64 reference of the mutual-information tests (test_mi_reference.py on the CPU, test_gpu_mi.py on the GPU).
Nothing here calls the code under test.

Reference: VoxelMorph's global MutualInformation written out in torch (mi_loss below), evaluated in float64 on the float32 inputs; its
gradients come from autograd.  The yardstick of every tolerance is the SAME function evaluated in float32 on the CPU: FP32_DISTANCE holds,
per case, its distance from the float64 result as measured when the cases were written (loss: absolute; gradients: max norm over the
gradient's max).  The kernels get 4 x those per-case distances -- they accumulate in another order and their partial sums are doubles --
with floors of 5e-7 (loss) and 2e-6 (gradients).  test_mi_reference.py re-measures the distances and checks that the float32 evaluation
itself still fits the bounds derived from the recorded ones.

Guard band: no voxel lies within 1e-3 of vmin or vmax (on either side), so the clamp's subgradient is never in question."""
import functools

import torch

GUARD = 1e-3
LOSS_FLOOR, GRAD_FLOOR, FACTOR = 5e-7, 2e-6, 4.0

# name: (N, shape (a D x H x W triple = 5-D input N x 1 x D x H x W, a single extent = flat N x V), bins, sigma_ratio, (vmin, vmax), input kind,
#        the launcher branch it exercises).  Forward: 256-voxel tiles, min(ceil(tiles / 2), 512) workgroups per sample, fp32 accumulators
# flushed into doubles every 4 tiles; backward: 32-voxel tiles per wave.  Loads are dwords, so V % 4 != 0 (sample bases off 16 bytes) takes
# the same code as an aligned sample -- 'ragged' is there to show it.
CASES = {
    'tiny':     (1, (3, 4, 5), 32, 1.0, (0.0, 1.0), 'related', 'V = 60: below one tile, one partly filled wave, three idle waves'),
    'ragged':   (3, (7, 9, 11), 32, 1.0, (0.0, 1.0), 'independent', 'V = 693, V % 4 = 1: ragged last tile, unaligned sample bases, a workgroup with 2 tiles and one with 1'),
    'aligned':  (2, (16, 16, 16), 16, 0.5, (0.0, 1.0), 'related', 'V = 4096: 16 full tiles, 8 workgroups of 2 tiles; 16 bins padded to 32; sigma_ratio 0.5'),
    'narrow':   (1, (9, 10, 12), 32, 0.5, (0.0, 1.0), 'related', 'V = 1080: 32 bins at sigma_ratio 0.5 (weights concentrated on 2 - 3 bins)'),
    'range5':   (2, (1000,), 5, 1.0, (-0.5, 2.0), 'outside', 'flat N x V input, 5 bins padded to 32, non-default range, values beyond both ends on both images'),
    'constant': (1, (5, 6, 7), 32, 1.0, (0.0, 1.0), 'constant', 'V = 210: one image constant (MI = 0 up to the epsilons; gradient by cancellation)'),
    'capped':   (1, (64, 96, 96), 16, 1.0, (0.0, 1.0), 'related', 'V = 589824: 2304 tiles on the 512-workgroup cap, 4 - 5 tiles per workgroup: the mid-loop flush and the remainder'),
}
IDS = list(CASES)
# the constant image is held on the loss only: its gradient is ~1e-8 by cancellation and float32 torch is already 1 % - 6000 % off
GRAD_CASES = [k for k in IDS if k != 'constant']

# float32-torch-vs-float64 distances (loss abs, dx rel, dy rel), measured on the CPU when the cases were written
FP32_DISTANCE = {
    'tiny':     (1.05e-08, 6.66e-07, 3.65e-07),
    'ragged':   (6.23e-08, 6.83e-07, 1.04e-06),
    'aligned':  (1.41e-08, 1.03e-06, 6.73e-07),
    'narrow':   (9.06e-09, 1.34e-06, 1.64e-06),
    'range5':   (7.43e-08, 4.03e-07, 5.03e-07),
    'constant': (2.70e-08, 3.53e-02, 2.87e-02),
    'capped':   (3.08e-08, 5.60e-07, 5.10e-07),
}


def bounds(name):
    """(loss bound, dx bound, dy bound) of a case: 4 x the recorded float32 distances, not below the floors."""
    l, gx, gy = FP32_DISTANCE[name]
    return max(FACTOR * l, LOSS_FLOOR), max(FACTOR * gx, GRAD_FLOOR), max(FACTOR * gy, GRAD_FLOOR)


def guard(t, vmin, vmax):
    """Move every value closer than 2 GUARD to vmin or vmax to 2 GUARD inside or outside of it (its side kept)."""
    for edge in (vmin, vmax):
        d = t - edge
        near = d.abs() < 2 * GUARD
        t = torch.where(near, edge + torch.where(d >= 0, torch.full_like(t, 2 * GUARD), torch.full_like(t, -2 * GUARD)), t)
    return t


def in_guard_band(t, vmin, vmax):
    """True where a value lies within GUARD of vmin or vmax."""
    return ((t - vmin).abs() < GUARD) | ((t - vmax).abs() < GUARD)


def inputs(name):
    """(x, y) float32 CPU tensors of a case, N x 1 x D x H x W or N x V."""
    N, shape, bins, sr, (vmin, vmax), kind, _ = CASES[name]
    g = torch.Generator().manual_seed(1000 + IDS.index(name))
    full = (N, 1) + tuple(shape) if len(shape) == 3 else (N,) + tuple(shape)
    span = vmax - vmin
    u = torch.rand(full, generator=g, dtype=torch.float64)
    noise = torch.randn(full, generator=g, dtype=torch.float64)
    if kind == 'related':              # y a non-monotonic function of x plus noise: what MI is for
        x = vmin + span * u
        y = vmin + span * (0.1 + 0.8 * (2 * u - 1).abs() ** 1.5 + 0.04 * noise)
    elif kind == 'independent':
        x = vmin + span * u
        y = vmin + span * torch.rand(full, generator=g, dtype=torch.float64)
    elif kind == 'outside':            # a quarter of the voxels beyond either end, on both images
        x = vmin + span * (1.6 * u - 0.3)
        y = vmin + span * (1.6 * (0.5 + 0.5 * torch.sin(7 * u + 0.3 * noise)) - 0.3)
    elif kind == 'constant':
        x = torch.full(full, vmin + 0.3 * span, dtype=torch.float64)
        y = vmin + span * u
    else:
        raise KeyError(kind)
    x, y = guard(x.float(), vmin, vmax), guard(y.float(), vmin, vmax)
    return x.contiguous(), y.contiguous()


def mi_loss(x, y, bins, sigma_ratio, vmin, vmax):
    """The definition, in the dtype of x: -mean over the batch of MI.  x, y: N x ... (flattened per sample)."""
    N = x.shape[0]
    x, y = x.reshape(N, -1), y.reshape(N, -1)
    V = x.shape[1]
    c = torch.linspace(vmin, vmax, bins, dtype=x.dtype)
    sigma = (vmax - vmin) / (bins - 1) * sigma_ratio
    p = 1.0 / (2.0 * sigma * sigma)

    def weights(t):
        e = torch.exp(-p * (t.clamp(vmin, vmax).unsqueeze(-1) - c) ** 2)
        return e / e.sum(-1, keepdim=True)
    wx, wy = weights(x), weights(y)
    P = torch.bmm(wx.transpose(1, 2), wy) / V
    a, b = wx.mean(1), wy.mean(1)
    Q = a.unsqueeze(2) * b.unsqueeze(1) + 1e-6
    R = P / Q + 1e-6
    mi = (P * torch.log(R)).sum((1, 2))
    return -mi.mean()


def evaluate(x, y, bins, sigma_ratio, vmin, vmax, dtype):
    """(loss, dx, dy) of mi_loss in `dtype` on the CPU (gradients by autograd), returned as float64."""
    a = x.detach().cpu().to(dtype).requires_grad_(True)
    b = y.detach().cpu().to(dtype).requires_grad_(True)
    loss = mi_loss(a, b, bins, sigma_ratio, vmin, vmax)
    loss.backward()
    return float(loss.detach().double()), a.grad.double(), b.grad.double()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(loss, dx, dy) of a case in float64: computed once, shared by the tests, never modified."""
    _, _, bins, sr, (vmin, vmax), _, _ = CASES[name]
    x, y = inputs(name)
    return evaluate(x, y, bins, sr, vmin, vmax, torch.float64)


def rel_max(got, want):
    """max |got - want| / max |want| (the gradient's own scale)."""
    return float((got.double() - want).abs().max() / want.abs().max())


def measure_fp32(name):
    """The float32 evaluation's distances from the float64 reference: (loss abs, dx rel, dy rel)."""
    _, _, bins, sr, (vmin, vmax), _, _ = CASES[name]
    x, y = inputs(name)
    l64, dx64, dy64 = reference(name)
    l32, dx32, dy32 = evaluate(x, y, bins, sr, vmin, vmax, torch.float32)
    return abs(l32 - l64), rel_max(dx32, dx64), rel_max(dy32, dy64)


# ---- shift property --------------------------------------------------------------------------------------------------------------
SHIFT_SHAPE, SHIFTS = (12, 16, 24), (-3, -2, -1, 0, 1, 2, 3)


def shift_volume():
    """A smooth structured volume in (0, 1), 1 x 1 x D x H x W float32."""
    D, H, W = SHIFT_SHAPE
    z = torch.arange(D, dtype=torch.float64).view(D, 1, 1)
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    v = 0.5 + 0.22 * torch.sin(0.55 * x + 0.3 * y) + 0.2 * torch.cos(0.45 * y - 0.35 * z + 0.2 * x) * torch.sin(0.4 * z + 1.0)
    return guard(v.clamp(0.02, 0.98).float(), 0.0, 1.0).view(1, 1, D, H, W).contiguous()


def shifted_fold(vol, s):
    """The 'fold' remap |2 x - 1| of vol, translated by s voxels along W (cyclic: every voxel keeps a partner)."""
    return torch.roll((2.0 * vol - 1.0).abs(), shifts=s, dims=-1).contiguous()
