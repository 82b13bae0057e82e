"""Inputs and host references of the distance-transform tests (test_edt_reference.py on the CPU, test_gpu_edt.py on the GPU).  Nothing here
calls the code under test.

Definition: for a set of sites S of a volume D x H x W with the spacing s = (sD, sH, sW),  d2(x) = min over y in S of sum_a (s_a (x_a - y_a))^2,
+inf when S is empty.  A mask's sites are its ZERO voxels (scipy's convention: ops.distance_transform_edt(mask) is 0 on them).

References:
  * edt_sq_scipy: scipy.ndimage.distance_transform_edt(mask, sampling=spacing) squared, float64.  With unit spacing d2 is an integer below
    2^24, np.rint of it is exact (test_edt_reference.py checks that against integer arithmetic on return_indices), and the device result --
    float32 integers -- is compared by exact equality.  A sample without a zero voxel is +inf here (scipy's own answer is meaningless there).
  * edt_sq_exhaustive: the plain minimum over all sites in numpy, for the small cases; holds the oracle itself.
  * signed_maps: phi_c = edt(not class c) - edt(class c) from the scipy reference, 0 for a class absent from a sample or filling it.
  * boundary_loss: the float64 torch evaluation  mean over (n, c in classes, x) of softmax(z)_c phi_c  with autograd, and the same in float32
    as the yardstick of the tolerance.

Tolerances of the loss: the project's rule.  The kernels get FACTOR = 4 x the distance of the float32 torch-CPU evaluation from the float64
one (loss: relative; gradient: max norm over the gradient's largest magnitude), never less than the floors of mi_cases.py (LOSS_FLOOR,
GRAD_FLOOR), which stand for the float32 arithmetic itself where a measured distance happens to be smaller.  The distances are measured when
a test asks for them (the shapes are small), once per case."""
import functools

import numpy as np
import torch
from scipy import ndimage

from mi_cases import LOSS_FLOOR, GRAD_FLOOR, FACTOR

ANISO = (1.0, 0.7, 2.5)
ANISO_RTOL = 1e-6          # <= three float32 roundings of 6e-8 per squared term (the issue's derivation); no case is excluded


# ---- references ---------------------------------------------------------------------------------------------------------------------
def edt_sq_scipy(mask, spacing=(1, 1, 1)):
    """Squared distance of every voxel of `mask` (N x D x H x W, nonzero = foreground) to the nearest zero voxel of its sample, float64."""
    out = np.empty(mask.shape, dtype=np.float64)
    unit = tuple(float(s) for s in spacing) == (1.0, 1.0, 1.0)
    for n, m in enumerate(mask):
        if (m != 0).all():
            out[n] = np.inf
            continue
        d = ndimage.distance_transform_edt(m != 0, sampling=tuple(float(s) for s in spacing))
        out[n] = np.rint(d * d) if unit else d * d
    return out


def edt_sq_exhaustive(mask, spacing=(1, 1, 1)):
    """The definition: minimum over all zero voxels, float64 (small cases only: O(V^2))."""
    out = np.empty(mask.shape, dtype=np.float64)
    s = np.asarray(spacing, dtype=np.float64)
    for n, m in enumerate(mask):
        pos = np.stack(np.meshgrid(*[np.arange(k) for k in m.shape], indexing='ij'), axis=-1).reshape(-1, 3).astype(np.float64) * s
        sites = pos[(m == 0).reshape(-1)]
        if len(sites) == 0:
            out[n] = np.inf
            continue
        d2 = ((pos[:, None, :] - sites[None, :, :]) ** 2).sum(-1).min(1)
        out[n] = d2.reshape(m.shape)
    return out


def signed_maps(labels, classes, spacing=(1, 1, 1)):
    """phi [N][K'][D][H][W] float64: + distance to class c outside it, - distance to its complement inside it, 0 where the class is absent
    from the sample or fills it."""
    N = labels.shape[0]
    out = np.zeros((N, len(classes)) + labels.shape[1:], dtype=np.float64)
    for n in range(N):
        for j, c in enumerate(classes):
            inside = labels[n] == c
            if not inside.any() or inside.all():
                continue
            d_out = np.sqrt(edt_sq_scipy((~inside)[None], spacing)[0])        # zero voxels of ~inside = the class
            d_in = np.sqrt(edt_sq_scipy(inside[None], spacing)[0])
            out[n, j] = d_out - d_in
    return out


def boundary_loss(logits, phi, classes, dtype=torch.float64):
    """(loss, d loss / d logits) of the definition in `dtype` on the CPU, as (float, float64 tensor)."""
    z = logits.detach().cpu().to(dtype).requires_grad_(True)
    p = torch.softmax(z, dim=1)[:, list(classes)]
    loss = (p * phi.detach().cpu().to(dtype)).mean()
    loss.backward()
    return float(loss.detach().double()), z.grad.double()


def boundary_grad_formula(logits, phi, classes):
    """dz_k = p_k (m_k phi_k - sum_c m_c p_c phi_c) / (N K' V) in float64, written out by hand."""
    z = logits.double()
    N, K = z.shape[:2]
    V = z[0, 0].numel()
    p = torch.softmax(z, dim=1)
    full = torch.zeros_like(z)
    full[:, list(classes)] = phi.double()
    S = (p * full).sum(1, keepdim=True)
    return p * (full - S) / (N * len(classes) * V)


def rel_max(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


# ---- site patterns ------------------------------------------------------------------------------------------------------------------
def rng(seed):
    return np.random.RandomState(seed)


def site_patterns(shape, seed=0):
    """[(name, sites)]: boolean arrays D x H x W, True = a site."""
    D, H, W = shape
    out = []

    def single(p):
        s = np.zeros(shape, dtype=bool)
        s[p] = True
        return s
    out.append(('corner', single((0, 0, 0))))
    out.append(('far_corner', single((D - 1, H - 1, W - 1))))
    mid = (D // 2, H // 2, W // 2)
    for axis in range(3):
        for end in (0, shape[axis] - 1):
            p = list(mid)
            p[axis] = end
            out.append(('face%d_%d' % (axis, end), single(tuple(p))))
    out.append(('none', np.zeros(shape, dtype=bool)))
    out.append(('all', np.ones(shape, dtype=bool)))
    d, h, w = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    out.append(('checkerboard', (d + h + w) % 2 == 0))
    two = np.zeros(shape, dtype=bool)                            # two sites at the same distance from the voxels between them
    two[0, 0, 0] = True
    two[0, 0, W - 1] = True
    two[D - 1, H - 1, 0] = True
    out.append(('equidistant', two))
    r = rng(seed)
    for density in (0.002, 0.05, 0.5):
        s = r.rand(*shape) < density
        out.append(('noise%g' % density, s))
    return out


def blocky_labels(shape, n_labels, block=(3, 4, 5), seed=0, dtype=np.uint8, n=1):
    """N x D x H x W label map of random blocks with labels 0 .. n_labels - 1."""
    r = rng(seed)
    D, H, W = shape
    out = []
    for _ in range(n):
        coarse = r.randint(0, n_labels, size=tuple(-(-s // b) for s, b in zip(shape, block)))
        fine = np.repeat(np.repeat(np.repeat(coarse, block[0], 0), block[1], 1), block[2], 2)[:D, :H, :W]
        out.append(fine)
    return np.ascontiguousarray(np.stack(out).astype(dtype))


# ---- boundary-loss cases ------------------------------------------------------------------------------------------------------------
# name: (K, N, D x H x W, classes or None (= 1 .. K - 1), what it is there for).  The launcher gives K / 4 lanes to a voxel when K % 4 == 0 and
# K / 4 is a power of two <= 16, otherwise a thread; both forms walk a sample with at most 1024 workgroups.
LOSS_CASES = {
    'K4':       (4, 2, (3, 5, 7), None, 'one lane per voxel, batch 2'),
    'K8':       (8, 1, (5, 6, 11), [1, 3, 4, 7], 'two lanes per voxel, a class list with gaps'),
    'K16':      (16, 1, (4, 7, 9), None, 'four lanes per voxel'),
    'K32':      (32, 2, (6, 9, 13), None, "eight lanes per voxel: the registry's channel count; 702 voxels, ragged last pass"),
    'K64':      (64, 1, (11, 37, 43), None, 'sixteen lanes per voxel; 17501 voxels = 1094 passes on 1024 workgroups: the loop runs twice'),
    'K5':       (5, 2, (3, 5, 7), [0, 2, 4], 'a thread per voxel (K % 4 != 0), the background in the list'),
    'K12':      (12, 1, (5, 6, 11), None, 'a thread per voxel (K / 4 = 3 is no power of two)'),
    'K5_long':  (5, 1, (40, 81, 83), None, 'a thread per voxel; 268920 voxels = 1051 workgroups of work on 1024: the loop runs twice'),
}
LOSS_IDS = list(LOSS_CASES)
LOGIT_MAX = 20.0


def case_classes(name):
    K, _, _, classes, _ = LOSS_CASES[name]
    return list(range(1, K)) if classes is None else list(classes)


@functools.lru_cache(maxsize=None)
def loss_inputs(name):
    """(logits float32 N x K x D x H x W with magnitudes up to LOGIT_MAX, phi float32 N x K' x D x H x W from the scipy reference of a blocky
    label map).  Never modified by a test."""
    K, N, shape, _, _ = LOSS_CASES[name]
    seed = LOSS_IDS.index(name)
    g = torch.Generator().manual_seed(100 + seed)
    z = (7.0 * torch.randn((N, K) + tuple(shape), generator=g, dtype=torch.float64)).clamp(-LOGIT_MAX, LOGIT_MAX).float()
    z[:, :, 0, 0, 0] = LOGIT_MAX * torch.sign(torch.randn((N, K), generator=g))          # the extremes are present
    labels = blocky_labels(shape, K, seed=seed, n=N, dtype=np.int64)
    phi = torch.from_numpy(signed_maps(labels, case_classes(name))).float()
    return z.contiguous(), phi.contiguous()


@functools.lru_cache(maxsize=None)
def loss_reference(name):
    z, phi = loss_inputs(name)
    return boundary_loss(z, phi, case_classes(name), torch.float64)


@functools.lru_cache(maxsize=None)
def loss_bounds(name):
    """(loss bound, relative; gradient bound, relative to max |gradient|): FACTOR x the float32 torch evaluation's distance, not below the floors."""
    z, phi = loss_inputs(name)
    l64, g64 = loss_reference(name)
    l32, g32 = boundary_loss(z, phi, case_classes(name), torch.float32)
    return max(FACTOR * abs(l32 - l64) / abs(l64), LOSS_FLOOR), max(FACTOR * rel_max(g32, g64), GRAD_FLOOR)
