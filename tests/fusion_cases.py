"""Inputs and oracles of the multi-atlas label-fusion tests (test_label_fusion_reference.py on the CPU, test_gpu_label_fusion.py on the
GPU).  Nothing here calls the code under test.

Vote: the per-atlas warped labels and their exclusion masks come from regeval_cases.nearest_oracle (torch-CPU grid_sample, nearest,
float64, a band of 1e-4 voxels around the half-integers); the scores are a float64 sum of one_hot x weight, argmax returns the first
maximum (= the smallest label), the confidence is formed in float64.  A target voxel may be left out of the label comparison only if
SOME atlas's coordinate lies in the band there; the excluded share is capped at K x 1e-3 (the per-atlas share is 4 - 7e-4).

Weights of locally weighted voting: the definition evaluated in numpy with direct separable window sums, in float64; the yardstick of the
tolerance is the same evaluation in float32 on the same input, the bound 4 x its maximum error (the factor covers another association
and FMA contraction, as in regeval_cases.jacobian_bound)."""
import numpy as np
import torch

import regeval_cases as rc
from deepatlas_amd.lib.datasets import structured_labels

MAX_EXCLUDED_PER_ATLAS = 1e-3
NEAR_TIE = 1e-5                  # locally weighted vote: float64 top-two scores closer than this share of the total may be left out
MAX_NEAR_TIE = 1e-3
N_CLASS_BLOCKY = 8

# (shape, N, K, field sigma in voxels, per-target atlas maps, label dtype, label kind).  K takes every bucket of the kernel (<= 4, 8, 16,
# 32) and both sides of each boundary; 33 x 47 x 61 has an odd voxel count (the element-access path), the others are multiples of 4.
VOTE_CASES = [
    ((17, 30, 22), 1, 1, 1.5, False, torch.uint8, 'blocky'),
    ((17, 30, 22), 2, 2, 4.0, True, torch.int64, 'blocky'),
    ((24, 40, 56), 1, 3, 1.5, False, torch.int64, 'blocky'),
    ((24, 40, 56), 2, 4, 4.0, False, torch.uint8, 'blocky'),
    ((33, 47, 61), 1, 5, 4.0, False, torch.uint8, 'blocky'),
    ((33, 47, 61), 2, 8, 1.5, True, torch.int64, 'blocky'),
    ((40, 48, 72), 1, 9, 1.5, False, torch.uint8, 'blocky'),
    ((40, 48, 72), 2, 16, 4.0, True, torch.uint8, 'blocky'),
    ((24, 40, 56), 1, 17, 4.0, False, torch.int64, 'blocky'),
    ((17, 30, 22), 2, 32, 1.5, True, torch.uint8, 'blocky'),
    ((33, 47, 61), 1, 32, 4.0, False, torch.int64, 'blocky'),
    ((24, 40, 56), 1, 5, 4.0, False, torch.uint8, 'iid32'),
]
VOTE_IDS = ['%dx%dx%d-n%d-k%d-s%g-%s-%s-%s' % (s + (n, k, sd, 'pertarget' if per else 'shared', 'u8' if dt == torch.uint8 else 'i64', kind))
            for s, n, k, sd, per, dt, kind in VOTE_CASES]
# the weighted votes (per-atlas and per-voxel weights) and the locally weighted vote run on these
WEIGHT_CASES = [VOTE_CASES[i] for i in (2, 3, 4, 5, 7, 8, 9)]
WEIGHT_IDS = [VOTE_IDS[i] for i in (2, 3, 4, 5, 7, 8, 9)]
LOCAL_CASES = [VOTE_CASES[i] for i in (2, 4, 5, 7)]           # K = 3, 5, 8, 16
LOCAL_IDS = [VOTE_IDS[i] for i in (2, 4, 5, 7)]

# (shape, N, K, radius, sigma): the shapes above and volumes with an extent below 2 r + 1
MSD_CASES = [
    ((17, 30, 22), 1, 3, 1, 0.05),
    ((24, 40, 56), 2, 2, 2, 0.2),
    ((33, 47, 61), 1, 2, 4, 0.05),
    ((40, 48, 72), 1, 1, 2, 0.05),
    ((33, 47, 61), 1, 3, 1, 0.2),
    ((3, 5, 7), 2, 3, 4, 0.2),
    ((2, 9, 4), 1, 2, 2, 0.05),
    ((5, 3, 11), 1, 2, 4, 0.05),
]
MSD_IDS = ['%dx%dx%d-n%d-k%d-r%d-s%g' % (s + (n, k, r, sg)) for s, n, k, r, sg in MSD_CASES]


def atlas_labels(shape, n_maps, dtype, kind, seed):
    """n_maps atlas label maps: blocky 8-class anatomy (every map another arrangement) or iid 32-class labels."""
    if kind == 'iid32':
        return rc.random_labels(shape, n_maps, dtype, seed, n_class=32)
    return torch.stack([structured_labels(shape, N_CLASS_BLOCKY, seed=seed + 3 * i) for i in range(n_maps)]).to(dtype)


def vote_inputs(case, seed=100):
    """(labels K or (N K) x D x H x W, disp (N K) x 3 x D x H x W float32, atlas index fastest) of a VOTE_CASES entry."""
    shape, n, k, sigma, per, dtype, kind = case
    disp = rc.smooth_field(shape, n * k, sigma, seed=seed + k)
    labels = atlas_labels(shape, n * k if per else k, dtype, kind, seed=seed + 7)
    return labels, disp


def exact_weights(shape_prefix, seed):
    """Weights that are multiples of 1/64 in [0, 4]: every fp32 sum of <= 32 of them is exact, in any order."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 257, tuple(shape_prefix), generator=g, dtype=torch.int64).double() / 64.0).float()


def vote_oracle(labels, disp, n, k, weights=None):
    """float64 vote on the CPU.  Returns a dict: fused int64 N x D x H x W, conf float64, excluded bool (some atlas in the band), total
    float64, gap float64 (top score - second score, as a share of the total; +inf for a zero total), warped int64 N x K x D x H x W."""
    labels, disp = labels.cpu(), disp.detach().cpu()
    shape = tuple(disp.shape[2:])
    if labels.shape[0] == k and n > 1:
        labels = labels.repeat(n, 1, 1, 1)                    # shared atlas maps: atlas index fastest in the batch
    warped, excl = rc.nearest_oracle(labels, disp)
    warped = (warped % 256).view((n, k) + shape)              # (the device stores uint8)
    excluded = excl.view((n, k) + shape).any(1)
    out = vote_from_warped(warped, weights)
    out.update(excluded=excluded, warped=warped)
    return out


def vote_from_warped(warped, weights=None):
    """The float64 vote of already warped labels, int64 N x K x D x H x W: dict of fused, conf, total, gap (see vote_oracle)."""
    n, k = warped.shape[:2]
    shape = tuple(warped.shape[2:])
    if weights is None:
        w = torch.ones((n, k) + shape, dtype=torch.float64)
    else:
        w = weights.detach().cpu().double()
        w = w.view(n, k, 1, 1, 1).expand((n, k) + shape) if w.dim() == 2 else w
    n_class = int(warped.max()) + 1
    scores = torch.zeros((n, max(n_class, 2)) + shape, dtype=torch.float64)
    for a in range(k):                                        # one_hot x weight, summed in float64
        scores.scatter_add_(1, warped[:, a:a + 1], w[:, a:a + 1].contiguous())
    fused = scores.argmax(1)                                  # first maximum = smallest label
    total = w.sum(1)
    top2 = scores.topk(2, dim=1).values
    safe = torch.where(total > 0, total, torch.ones_like(total))
    conf = torch.where(total > 0, top2[:, 0] / safe, torch.zeros_like(total))
    gap = torch.where(total > 0, (top2[:, 0] - top2[:, 1]) / safe, torch.full_like(total, float('inf')))
    return dict(fused=fused, conf=conf, total=total, gap=gap)


def shifted(lab, tx, ty, tz):
    """lab (... x D x H x W) read at (d + tz, h + ty, w + tx), zero outside: what an integer translation (tx, ty, tz) voxels warps it to."""
    D, H, W = lab.shape[-3:]
    out = torch.zeros_like(lab)
    d0, d1 = max(0, -tz), min(D, D - tz)
    h0, h1 = max(0, -ty), min(H, H - ty)
    w0, w1 = max(0, -tx), min(W, W - tx)
    if d1 > d0 and h1 > h0 and w1 > w0:
        out[..., d0:d1, h0:h1, w0:w1] = lab[..., d0 + tz:d1 + tz, h0 + ty:h1 + ty, w0 + tx:w1 + tx]
    return out


def tie_share(labels, disp, n, k):
    """Share of the voxels whose unweighted vote has an exact tie for the top count (the tie rule is exercised there)."""
    o = vote_oracle(labels, disp, n, k)
    return float((o['gap'] == 0).double().mean())


def msd_inputs(case, seed=300):
    """(warped N x K x D x H x W, target N x D x H x W) float32 images in [0, 1]: atlas k differs from the target by noise of
    0.03 (k + 1), so that exp(-m / 2 sigma^2) spreads over (0, 1) for the sigmas used."""
    shape, n, k, _, _ = case
    g = torch.Generator().manual_seed(seed + k)
    target = torch.rand((n,) + tuple(shape), generator=g, dtype=torch.float64)
    amp = 0.03 * torch.arange(1, k + 1, dtype=torch.float64).view(1, k, 1, 1, 1)
    warped = target[:, None] + amp * torch.randn((n, k) + tuple(shape), generator=g, dtype=torch.float64)
    return warped.clamp_(0, 1).float().contiguous(), target.float().contiguous()


def _box_axis(a, axis, r):
    """Direct window sum along `axis`, zero outside: the 2 r + 1 shifted terms added in window order, in a's dtype."""
    out = np.zeros_like(a)
    size = a.shape[axis]
    for t in range(-r, r + 1):
        lo, hi = max(0, -t), min(size, size - t)              # out[i] += a[i + t]
        if hi <= lo:
            continue
        dst = [slice(None)] * a.ndim
        src = [slice(None)] * a.ndim
        dst[axis], src[axis] = slice(lo, hi), slice(lo + t, hi + t)
        out[tuple(dst)] += a[tuple(src)]
    return out


def msd_weights_np(warped, target, radius, sigma, dtype=np.float64):
    """w = exp(-beta m), m = (2 r + 1)^-3 x the window sum of (warped - target)^2, beta = 1 / (2 sigma^2): N x K x D x H x W in `dtype`."""
    a = np.asarray(warped.detach().cpu().numpy() if torch.is_tensor(warped) else warped).astype(dtype)
    b = np.asarray(target.detach().cpu().numpy() if torch.is_tensor(target) else target).astype(dtype)
    e = a - b[:, None]
    s = e * e
    for axis in (4, 3, 2):
        s = _box_axis(s, axis, radius)
    n3 = dtype((2 * radius + 1) ** 3)
    beta = dtype(1.0 / (2.0 * float(sigma) * float(sigma)))
    w = np.exp(-beta * (s / n3))
    assert w.dtype == dtype
    return w


def msd_bound(warped, target, radius, sigma):
    """(w64, bound, yardstick): bound = 4 x the maximum absolute error of the float32 numpy evaluation on the same input."""
    w64 = msd_weights_np(warped, target, radius, sigma, np.float64)
    w32 = msd_weights_np(warped, target, radius, sigma, np.float32)
    yard = float(np.abs(w32.astype(np.float64) - w64).max())
    return w64, 4.0 * yard, yard
