"""Inputs and oracles of the registration-evaluation tests (test_regeval_host.py on the CPU, test_gpu_regeval.py and
test_gpu_reg_experiments.py on the GPU).  Nothing here calls the code under test.

Nearest warp: F.grid_sample(mode='nearest', padding_mode='zeros', align_corners=True) on torch-CPU in float64 with an fp64 identity grid.
A voxel may be left out of a comparison only if its fp64 sampling coordinate lies within BAND voxels of a half-integer on some axis
(rounding is discontinuous there and an fp32 coordinate at extent <= 200 carries about 1e-5 of error); the excluded share is capped at
MAX_EXCLUDED.  Jacobian: the definition evaluated with numpy.gradient in float64; the yardstick of every tolerance is the same formula in
float32 on the same input."""
import numpy as np
import torch
import torch.nn.functional as F

BAND = 1e-4
MAX_EXCLUDED = 2e-3
N_CLASS = 32

# (shape D x H x W, N, standard deviation of the field in voxels, label dtype): D != H != W, odd extents included
WARP_CASES = [
    ((24, 40, 56), 1, 1.5, torch.uint8),
    ((24, 40, 56), 3, 4.0, torch.int64),
    ((33, 47, 61), 1, 4.0, torch.uint8),
    ((33, 47, 61), 3, 1.5, torch.int64),
    ((40, 48, 72), 1, 4.0, torch.int64),
    ((40, 48, 72), 3, 1.5, torch.uint8),
]
WARP_IDS = ['%dx%dx%d-n%d-s%g-%s' % (s + (n, sd, 'u8' if dt == torch.uint8 else 'i64')) for s, n, sd, dt in WARP_CASES]
JAC_CASES = [((24, 40, 56), 1, 1.5), ((33, 47, 61), 3, 4.0), ((40, 48, 72), 1, 10.0), ((17, 30, 22), 3, 1.5), ((33, 47, 61), 1, 10.0)]
JAC_IDS = ['%dx%dx%d-n%d-s%g' % (s + (n, sd)) for s, n, sd in JAC_CASES]
FULL_SHAPE = (160, 192, 160)


def to_normalised(u_vox):
    """Displacement in voxels N x 3 x D x H x W (channels x, y, z = W, H, D axis) -> normalised units (2 / (size - 1) per voxel)."""
    D, H, W = u_vox.shape[2:]
    scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)], dtype=u_vox.dtype).view(1, 3, 1, 1, 1)
    return u_vox * scale


def smooth_field(shape, n, sigma_vox, seed):
    """A 5 x 6 x 7 lattice of normal values per component, trilinearly up-sampled to `shape` and scaled to `sigma_vox` voxels of standard
    deviation; returned in normalised units, float32 N x 3 x D x H x W."""
    g = torch.Generator().manual_seed(seed)
    lattice = torch.randn((n, 3, 5, 6, 7), generator=g, dtype=torch.float64)
    u = F.interpolate(lattice, size=tuple(shape), mode='trilinear', align_corners=True)
    u = u * (sigma_vox / float(u.std()))
    return to_normalised(u).float().contiguous()


def noise_field(shape, n, sigma_vox, seed):
    """iid normal displacements of `sigma_vox` voxels (the rough counterpart of smooth_field)."""
    g = torch.Generator().manual_seed(seed)
    return to_normalised(torch.randn((n, 3) + tuple(shape), generator=g, dtype=torch.float64) * sigma_vox).float().contiguous()


def random_labels(shape, n, dtype, seed, n_class=N_CLASS):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_class, (n,) + tuple(shape), generator=g, dtype=torch.int64).to(dtype)


def affine_field(shape, A, n=1):
    """u = A x in voxels (x = (x, y, z) voxel coordinates) as a normalised float32 field; A is 3 x 3, rows / columns in (x, y, z)."""
    D, H, W = shape
    z, y, x = torch.meshgrid(torch.arange(D, dtype=torch.float64), torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    pos = torch.stack([x, y, z], 0)
    u = torch.einsum('ca,adhw->cdhw', torch.as_tensor(A, dtype=torch.float64), pos)
    return to_normalised(u[None].repeat(n, 1, 1, 1, 1)).float().contiguous()


def identity_grid64(shape):
    """lib/utils.py:89-102 in float64: D x H x W x 3, last axis (x, y, z)."""
    D, H, W = shape
    z, y, x = torch.meshgrid(torch.linspace(-1, 1, D, dtype=torch.float64), torch.linspace(-1, 1, H, dtype=torch.float64),
                             torch.linspace(-1, 1, W, dtype=torch.float64), indexing='ij')
    return torch.stack([x, y, z], -1)


def nearest_oracle(labels, disp, dtype=torch.float64):
    """(warped int64 N x D x H x W, excluded bool N x D x H x W) on the CPU.  `dtype`=float32 is torch's own fp32 path on the same input
    (the conditioning test compares the two); the exclusion band always comes from the fp64 coordinates."""
    labels, disp = labels.cpu(), disp.detach().cpu()
    shape = tuple(disp.shape[2:])
    grid64 = disp.double().permute(0, 2, 3, 4, 1) + identity_grid64(shape)
    grid = grid64 if dtype == torch.float64 else (disp.float().permute(0, 2, 3, 4, 1) + identity_grid64(shape).float())
    out = F.grid_sample(labels.to(dtype)[:, None], grid.to(dtype), mode='nearest', padding_mode='zeros', align_corners=True)[:, 0]
    size = torch.tensor([shape[2], shape[1], shape[0]], dtype=torch.float64)
    vox = (grid64 + 1) / 2 * (size - 1)
    frac = vox - torch.floor(vox)
    excluded = ((frac - 0.5).abs() < BAND).any(-1) | ~torch.isfinite(vox).all(-1)
    return out.round().to(torch.int64), excluded


def counts_np(pred, truth, n_class):
    """[N][n_class][3] int64 = (|pred==c|, |truth==c|, |both|); labels outside [0, n_class) ignored."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    n = pred.shape[0]
    out = np.zeros((n, n_class, 3), dtype=np.int64)
    for i in range(n):
        p, t = pred[i].reshape(-1).astype(np.int64), truth[i].reshape(-1).astype(np.int64)
        pv, tv = (p >= 0) & (p < n_class), (t >= 0) & (t < n_class)
        out[i, :, 0] = np.bincount(p[pv], minlength=n_class)
        out[i, :, 1] = np.bincount(t[tv], minlength=n_class)
        out[i, :, 2] = np.bincount(p[pv & (p == t)], minlength=n_class)
    return out


def jacobian_np(disp, dtype=np.float64):
    """det J of x -> x + u(x), N x D x H x W in `dtype`: u_c = disp_c (size_c - 1) / 2, numpy.gradient (unit spacing), cofactor expansion."""
    d = np.asarray(disp.detach().cpu().numpy() if torch.is_tensor(disp) else disp).astype(dtype)
    N, _, D, H, W = d.shape
    size = {0: W, 1: H, 2: D}
    axis_of = {0: 3, 1: 2, 2: 1}             # derivative along x / y / z = array axis W / H / D of an N x D x H x W array
    J = [[None] * 3 for _ in range(3)]
    for c in range(3):
        u = d[:, c] * dtype((size[c] - 1) / 2.0)
        for a in range(3):
            g = np.gradient(u, axis=axis_of[a]).astype(dtype)
            J[c][a] = g + dtype(1) if c == a else g
    det = (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
           + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))
    assert det.dtype == dtype
    return det


def jacobian_bound(disp):
    """(det64, per-voxel bound) with bound = 4 x the maximum absolute error of the float32 numpy evaluation on the same input
    (the factor covers a different association and FMA contraction)."""
    det64 = jacobian_np(disp, np.float64)
    det32 = jacobian_np(disp, np.float32)
    yard = float(np.abs(det32.astype(np.float64) - det64).max())
    return det64, 4.0 * yard, yard
