"""Cases, float64 numpy references, float32 torch evaluations, guard-band rules and tolerances of the intensity-augmentation kernels
(da_gauss_blur3d, da_bilateral3d, da_intensity_augment), shared by test_intensity_reference.py (CPU) and test_gpu_intensity.py (GPU).

The references restate the definitions of include/deepatlas_hip.h in float64, independently of the host helpers in deepatlas_amd
(ops.bilateral_tables, lib.transforms.discrete_gaussian_taps / bspline_support).  Neither SimpleITK nor ITK is available to these tests:
agreement with ITK itself is NOT tested, only agreement with the stated definitions.

Tolerance (the project's rule): a device result is held to  max(4 x d32, FLOOR_ULPS float32 ulps of the data range)  where d32 is the
largest distance of a float32 torch evaluation of the same formula (the *_torch32 functions, on the CPU) from the float64 reference on
the same case.  d32 as measured on the cases below (max over the case lists; `python tests/intensity_cases.py` prints them):
    blur        default 1.4e-07, r1 1.4e-07, rmax (R = 16) 2.2e-07, axes 1.6e-07                          (data in [0, 1))
    bilateral   lattice radius <= 2: 0.6 - 2.1e-07, aniso 2.1e-07, radius 4 3.7e-07 (data in [0, 0.25)); continuous 4.7e-07
    pointwise   bias 1.1e-07, gamma 3.4e-08, inverted gamma 4.6e-08, linear 1.0e-07, noise 8.0e-08, clamp 7.2e-08, all 1.5e-07
so the blur and bilateral bounds are 4 x d32 (5e-07 .. 1.9e-06) and most pointwise bounds sit at the floor, 4.8e-07 for data in [0, 1].

Guard band of the bilateral filter's continuous case.  The table index floor(delta * scale) is discontinuous, and the device forms it in
float32: delta32 = fl(b - a) = delta (1 + e1), scale32 = scale (1 + e2), the product rounds once more (1 + e3), every |e| <= u = 2^-24.
So |delta32 scale32 - delta scale| <= 3 u delta scale (1 + O(u)) < 3 u S, since delta scale < S for a tap that takes part.  A voxel is
left out when any of its taps has delta scale within GUARD = 4 u S of an integer (one u of margin), or delta within 4 u c of the cutoff c
(both sides of `delta < c` carry one rounding each).  On the lattice cases (values k / 256) delta is exact in float32 and delta scale
sits >= 1 / 768 from every integer (asserted for every (sigma_r, S) pair used), so nothing is left out there.  The share left out may
not exceed GUARD_CAP.
"""
import functools

import numpy as np
import torch

from deepatlas_amd import ops
from oracle import datapath as oracle_datapath

U32 = 2.0 ** -24                 # unit roundoff of float32
FLOOR_ULPS = 4                   # "a few float32 ulps of the data range"
GUARD_CAP = 0.02
LATTICE = 256                    # lattice images hold multiples of 1 / 256 ...
LATTICE_LEVELS = 64              # ... below 64 / 256, so deltas reach past the cutoff 0.24 of RANGE_PAIRS[0]
RANGE_PAIRS = [(0.06, 50), (0.1, 100)]          # (sigma_r, S); the first is the reference's default


def tolerance(ref64, eval32):
    d32 = float(np.nanmax(np.abs(np.asarray(eval32, dtype=np.float64) - ref64))) if ref64.size else 0.0
    rng = float(np.nanmax(np.abs(ref64))) if ref64.size else 1.0
    return max(4.0 * d32, FLOOR_ULPS * 2.0 ** -23 * rng), d32


def lattice_image(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, LATTICE_LEVELS, tuple(shape), generator=g).float() / LATTICE


def rand_image(shape, seed):
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed))


def _axis_extent_shapes(rest=(5, 6, 7)):
    """extents of 1 and 2 on each axis in turn (below every radius): N x C x D x H x W"""
    out = {}
    for ax, name in enumerate('DHW'):
        for e in (1, 2):
            s = list(rest)
            s[ax] = e
            out['%s%d' % (name, e)] = (1, 1) + tuple(s)
    return out


# ---- Gaussian blur ----------------------------------------------------------------------------------------------------------------
def blur_shapes():
    s = _axis_extent_shapes()
    s['small'] = (1, 1, 3, 4, 7)
    s['ragged'] = (1, 1, 9, 11, 70)                              # W no multiple of 64, several workgroup trips, H / D odd
    s['long_w'] = (1, 1, 1, 2, ops.BLUR_BLOCK + 44)              # one line longer than a workgroup's (and a wave's) chunk of W
    s['c2'] = (1, 2, 4, 5, 9)
    return s


def gauss_taps(variance, radius):
    """a sampled, normalised Gaussian of 2 radius + 1 taps (any positive taps would do: the kernel takes what it is given)"""
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    t = np.exp(-k * k / (2.0 * variance))
    return t / t.sum()


def blur_taps():
    """tap sets (x, y, z): the reference default (asserted equal to discrete_gaussian_taps(0.5, 1, 0.9) by the CPU companion), another
    R = 1, R = DA_BLUR_MAX_RADIUS, and three different vectors on the three axes (pins the axis order)."""
    default = np.array([0.16329949, 0.67340102, 0.16329949])
    default = default / default.sum()
    R = ops.BLUR_MAX_RADIUS
    return {'default': [default] * 3, 'r1': [np.array([0.3, 0.45, 0.25])] * 3, 'rmax': [gauss_taps(30.0, R)] * 3,
            'axes': [gauss_taps(0.6, 2), np.array([0.0, 0.1, 0.2, 0.4, 0.3, 0.0, 0.0]), gauss_taps(2.0, 3)]}


def padded_taps(taps):
    R = max(len(t) for t in taps) // 2
    out = np.zeros((3, 2 * R + 1))
    for k, t in enumerate(taps):
        r = len(t) // 2
        out[k, R - r:R + r + 1] = t
    return out.astype(np.float32), R                              # (rounded once to float32, as the device receives them)


def blur_reference(img, taps):
    """float64: per axis W, H, D  out[i] = sum_k taps[k] in[clamp(i + k - R)]; img N x C x D x H x W; taps (x, y, z)"""
    tp, R = padded_taps(taps)
    x = np.asarray(img, dtype=np.float64)
    for axis, t in ((4, tp[0]), (3, tp[1]), (2, tp[2])):
        n = x.shape[axis]
        acc = np.zeros_like(x)
        for k in range(2 * R + 1):
            acc += float(t[k]) * np.take(x, np.clip(np.arange(n) + k - R, 0, n - 1), axis=axis)
        x = acc
    return x


def blur_torch32(img, taps):
    tp, R = padded_taps(taps)
    x = img.float()
    for axis, t in ((4, tp[0]), (3, tp[1]), (2, tp[2])):
        n = x.shape[axis]
        acc = torch.zeros_like(x)
        for k in range(2 * R + 1):
            acc = acc + torch.tensor(t[k]) * x.index_select(axis, torch.clamp(torch.arange(n) + k - R, 0, n - 1))
        x = acc
    return x.numpy()


# ---- bilateral filter -------------------------------------------------------------------------------------------------------------
def bilateral_cases():
    """name -> dict(shape N x C x D x H x W, kind 'lattice' | 'rand', sigma_d, pair (index into RANGE_PAIRS), spacing (x, y, z))"""
    td, th, tw = ops.BILATERAL_TILE
    c = {}
    for name, shape in _axis_extent_shapes((4, 5, 6)).items():
        c[name] = dict(shape=shape, kind='lattice', sigma_d=0.5, pair=0)
    c['small'] = dict(shape=(1, 1, 3, 5, 9), kind='lattice', sigma_d=0.5, pair=0)
    c['ragged'] = dict(shape=(1, 1, td + 3, th + 5, tw + 7), kind='lattice', sigma_d=0.5, pair=0)
    c['long_w'] = dict(shape=(1, 1, 2, 3, 70), kind='lattice', sigma_d=0.5, pair=1)
    c['c2'] = dict(shape=(1, 2, 4, 6, 10), kind='lattice', sigma_d=0.4, pair=1)
    c['aniso'] = dict(shape=(1, 1, td + 1, th + 2, tw + 2), kind='lattice', sigma_d=1.0, pair=0, spacing=(1.0, 0.7, 2.5))
    c['radius4'] = dict(shape=(1, 1, td + 1, th + 2, tw + 2), kind='lattice', sigma_d=1.5, pair=0)
    c['continuous'] = dict(shape=(1, 1, td + 1, th + 2, tw + 2), kind='rand', sigma_d=0.5, pair=0)
    for k, (name, case) in enumerate(sorted(c.items())):
        case.setdefault('spacing', (1.0, 1.0, 1.0))
        case['seed'] = 100 + k
    return c


def bilateral_input(case):
    return (lattice_image if case['kind'] == 'lattice' else rand_image)(case['shape'], case['seed'])


def bilateral_setup(sigma_d, sigma_r, S, spacing):
    """radii (x, y, z), domain weights [z][y][x], cutoff, table, scale -- float64, restated from the definition"""
    r = [int(np.ceil(2.5 * sigma_d / float(s))) for s in spacing]
    wd = np.zeros((2 * r[2] + 1, 2 * r[1] + 1, 2 * r[0] + 1))
    for oz in range(-r[2], r[2] + 1):
        for oy in range(-r[1], r[1] + 1):
            for ox in range(-r[0], r[0] + 1):
                wd[oz + r[2], oy + r[1], ox + r[0]] = np.exp(-((ox * spacing[0]) ** 2 + (oy * spacing[1]) ** 2 + (oz * spacing[2]) ** 2) / (2 * sigma_d ** 2))
    c = 4.0 * sigma_r
    table = np.array([np.exp(-0.5 * (i * c / S) ** 2 / sigma_r ** 2) for i in range(S)])
    return r, wd, c, table, S / c


def _shifted(x, r, oz, oy, ox):
    D, H, W = x.shape[-3:]
    x = np.take(x, np.clip(np.arange(D) + oz, 0, D - 1), axis=-3)
    x = np.take(x, np.clip(np.arange(H) + oy, 0, H - 1), axis=-2)
    return np.take(x, np.clip(np.arange(W) + ox, 0, W - 1), axis=-1)


def bilateral_reference(img, sigma_d, sigma_r, S, spacing=(1.0, 1.0, 1.0)):
    """float64 reference and the guard mask: (out, guarded) with guarded[v] true when any tap of v lies within the guard band."""
    r, wd, c, table, scale = bilateral_setup(sigma_d, sigma_r, S, spacing)
    a = np.asarray(img, dtype=np.float64)
    num, den = np.zeros_like(a), np.zeros_like(a)
    guarded = np.zeros(a.shape, dtype=bool)
    guard = 4 * U32 * S
    with np.errstate(invalid='ignore'):
        for oz in range(-r[2], r[2] + 1):
            for oy in range(-r[1], r[1] + 1):
                for ox in range(-r[0], r[0] + 1):
                    b = _shifted(a, r, oz, oy, ox)
                    delta = np.abs(b - a)
                    take = delta < c
                    pos = delta * scale
                    idx = np.where(take, np.floor(pos), 0).astype(np.int64)
                    w = np.where(take, wd[oz + r[2], oy + r[1], ox + r[0]] * table[np.minimum(idx, S - 1)], 0.0)
                    num += np.where(take, w * b, 0.0)
                    den += w
                    near_edge = take & (np.abs(pos - np.round(pos)) < guard) & (np.round(pos) > 0)
                    guarded |= near_edge | (np.abs(delta - c) < 4 * U32 * c)
        out = num / den
    return out, guarded


def bilateral_torch32(img, sigma_d, sigma_r, S, spacing=(1.0, 1.0, 1.0)):
    """the same formula, sum w b / sum w, in float32 torch, offset by offset (shifted slices)"""
    r, wd, c, table, scale = bilateral_setup(sigma_d, sigma_r, S, spacing)
    a = img.float()
    D, H, W = a.shape[-3:]
    tb = torch.from_numpy(table.astype(np.float32))
    c32, s32 = torch.tensor(np.float32(c)), torch.tensor(np.float32(scale))
    num, den = torch.zeros_like(a), torch.zeros_like(a)
    for oz in range(-r[2], r[2] + 1):
        for oy in range(-r[1], r[1] + 1):
            for ox in range(-r[0], r[0] + 1):
                b = a.index_select(-3, torch.clamp(torch.arange(D) + oz, 0, D - 1)).index_select(-2, torch.clamp(torch.arange(H) + oy, 0, H - 1))
                b = b.index_select(-1, torch.clamp(torch.arange(W) + ox, 0, W - 1))
                delta = (b - a).abs()
                take = delta < c32
                idx = torch.where(take, torch.floor(delta * s32), torch.zeros_like(delta)).long().clamp(max=S - 1)
                w = torch.where(take, torch.tensor(np.float32(wd[oz + r[2], oy + r[1], ox + r[0]])) * tb[idx], torch.zeros_like(a))
                num = num + torch.where(take, w * b, torch.zeros_like(a))
                den = den + w
    return (num / den).numpy()


def lattice_min_distance(sigma_r, S):
    """smallest distance of delta scale from an integer, and of delta from the cutoff (in units of 1 / 256), over the lattice deltas
    m / 256, 1 <= m < LATTICE_LEVELS (delta = 0 is index 0 exactly in any precision)"""
    c = 4.0 * sigma_r
    m = np.arange(1, LATTICE_LEVELS, dtype=np.float64)
    pos = m / LATTICE * (S / c)
    inside = m / LATTICE < c
    d_int = np.abs(pos - np.round(pos))[inside].min()
    d_cut = np.abs(m / LATTICE - c).min()
    return float(d_int), float(d_cut)


@functools.lru_cache(maxsize=None)
def bilateral_expected(name):
    """(input, float64 reference, guard mask, tolerance, d32) of one case, computed once and shared"""
    case = bilateral_cases()[name]
    sigma_r, S = RANGE_PAIRS[case['pair']]
    img = bilateral_input(case)
    ref, guarded = bilateral_reference(img.numpy(), case['sigma_d'], sigma_r, S, case['spacing'])
    t32 = bilateral_torch32(img, case['sigma_d'], sigma_r, S, case['spacing'])
    keep = ~guarded
    tol, d32 = tolerance(ref[keep], t32[keep])
    return img, ref, guarded, tol, d32


# ---- fused pointwise pass ---------------------------------------------------------------------------------------------------------
def pointwise_shapes():
    s = _axis_extent_shapes((4, 5, 6))
    s['small'] = (1, 1, 3, 4, 7)
    s['ragged'] = (1, 1, 5, 7, 67)                               # W no multiple of 4 (scalar tail) nor of 64
    s['vector'] = (1, 1, 4, 6, 72)                               # W a multiple of 4: the 16-byte path
    s['long_w'] = (1, 1, 1, 2, 4 * 256 + 4)                      # one line longer than a workgroup's chunk (256 threads x 4 voxels)
    s['c2'] = (1, 2, 4, 5, 9)
    return s


STAGES = {
    'bias': dict(bias=True),
    'gamma': dict(gamma=1.37),
    'gamma_inv': dict(gamma=0.8, invert=True),
    'linear': dict(gain=1.2, offset=-0.07),
    'noise': dict(noise_std=0.05, seed=77),
    'clamp': dict(gain=1.6, offset=-0.2, clamp=True),
    'all': dict(bias=True, gamma=1.3, invert=True, gain=0.9, offset=0.04, noise_std=0.03, clamp=True, seed=5),
    'neutral': dict(gamma=1.0, gain=1.0, offset=0.0, noise_std=0.0, seed=3),        # bits ON with neutral values: within tolerance, not exact
}


def _bspline_value(u, order, xp):
    a = xp.abs(u)
    if order == 1:
        return xp.clip(1 - a, 0, None) if xp is np else torch.clamp(1 - a, min=0)
    if order == 2:
        return xp.where(a < 0.5, 0.75 - a * a, xp.where(a < 1.5, 0.5 * (1.5 - a) ** 2, 0 * a))
    return xp.where(a < 1, 2.0 / 3.0 - a * a + 0.5 * a ** 3, xp.where(a < 2, (2 - a) ** 3 / 6.0, 0 * a))


def bspline_basis(size, M, order):
    """size x (M + order) float64: row i holds the weights of output index i (grid coordinate g = i M / (size - 1) + (order - 1) / 2, support
    start floor(g - (order - 1) / 2) clamped to M - 1: ITK's nudge at the upper face)"""
    B = np.zeros((size, M + order))
    for i in range(size):
        g = i * M / (size - 1) + (order - 1) / 2
        s = min(int(np.floor(g - (order - 1) / 2)), M - 1)
        for k in range(order + 1):
            B[i, s + k] = _bspline_value(np.float64(g - (s + k)), order, np)
    return B


def bias_field_reference(coef, shape, order):
    """coef gz x gy x gx -> b on D x H x W, float64, voxel by voxel over its support (no basis matrix)"""
    D, H, W = shape
    gz, gy, gx = coef.shape
    out = np.zeros(shape)
    sup = []
    for size, g in ((D, gz), (H, gy), (W, gx)):
        M = g - order
        rows = []
        for i in range(size):
            gc = i * M / (size - 1) + (order - 1) / 2
            s = min(int(np.floor(gc - (order - 1) / 2)), M - 1)
            rows.append((s, [float(_bspline_value(np.float64(gc - (s + k)), order, np)) for k in range(order + 1)]))
        sup.append(rows)
    for d in range(D):
        sz, wz = sup[0][d]
        for h in range(H):
            sy, wy = sup[1][h]
            for w in range(W):
                sx, wx = sup[2][w]
                blk = coef[sz:sz + order + 1, sy:sy + order + 1, sx:sx + order + 1]
                out[d, h, w] = np.einsum('a,b,c,abc->', wz, wy, wx, blk)
    return out


def noise_bits(seed, sample, n_elements, stream):
    """the hash bits of every element of one sample: oracle/datapath.py's restatement of the counter hash"""
    ctr = np.uint64(sample) * np.uint64(n_elements) + np.arange(n_elements, dtype=np.uint64)
    return oracle_datapath._synth_bits(seed, ctr, stream)


def noise_reference(seed, sample, n_elements):
    """standard normals, float64, Box-Muller from two 24-bit uniforms u = ((bits >> 8) + 0.5) 2^-24"""
    u1 = ((noise_bits(seed, sample, n_elements, ops.INTENSITY_STREAMS[0]) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((noise_bits(seed, sample, n_elements, ops.INTENSITY_STREAMS[1]) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def intensity_reference(img, params, coef=None, order=2, sample0=0):
    """float64; img N x C x D x H x W, params one dict per sample (None: untouched), coef N x gz x gy x gx or None"""
    x = np.asarray(img, dtype=np.float64).copy()
    N, C, D, H, W = x.shape
    for n, p in enumerate(params):
        if p is None:
            continue
        v = x[n]
        if coef is not None and p.get('bias', True):
            v = v * np.exp(bias_field_reference(np.asarray(coef[n], dtype=np.float32).astype(np.float64), (D, H, W), order))[None]
        if p.get('gamma') is not None:
            vc = np.clip(v, 0, 1)
            gm = np.float64(np.float32(p['gamma']))
            v = 1 - (1 - vc) ** gm if p.get('invert') else vc ** gm
        if p.get('gain') is not None or p.get('offset') is not None:
            gain = np.float64(np.float32(1.0 if p.get('gain') is None else p['gain']))
            off = np.float64(np.float32(0.0 if p.get('offset') is None else p['offset']))
            v = gain * v + off
        if p.get('noise_std') is not None:
            v = v + np.float64(np.float32(p['noise_std'])) * noise_reference(p.get('seed', 0), sample0 + n, C * D * H * W).reshape(C, D, H, W)
        if p.get('clamp'):
            v = np.clip(v, 0, 1)
        x[n] = v
    return x


def intensity_torch32(img, params, coef=None, order=2, sample0=0):
    """the same stages in float32 torch (basis-matrix B-spline, float32 uniforms, torch's log / cos / pow / exp)"""
    x = img.float().clone()
    N, C, D, H, W = x.shape
    f = lambda v: torch.tensor(np.float32(v))
    for n, p in enumerate(params):
        if p is None:
            continue
        v = x[n]
        if coef is not None and p.get('bias', True):
            cf = torch.from_numpy(np.asarray(coef[n], dtype=np.float32))
            gz, gy, gx = cf.shape
            Bz, By, Bx = (torch.from_numpy(bspline_basis(s, g - order, order).astype(np.float32)) for s, g in ((D, gz), (H, gy), (W, gx)))
            v = v * torch.exp(torch.einsum('da,hb,wc,abc->dhw', Bz, By, Bx, cf))[None]
        if p.get('gamma') is not None:
            vc = v.clamp(0, 1)
            v = 1 - (1 - vc) ** f(p['gamma']) if p.get('invert') else vc ** f(p['gamma'])
        if p.get('gain') is not None or p.get('offset') is not None:
            v = f(1.0 if p.get('gain') is None else p['gain']) * v + f(0.0 if p.get('offset') is None else p['offset'])
        if p.get('noise_std') is not None:
            E = C * D * H * W
            k1 = (noise_bits(p.get('seed', 0), sample0 + n, E, ops.INTENSITY_STREAMS[0]) >> np.uint32(8)).astype(np.float32)
            k2 = (noise_bits(p.get('seed', 0), sample0 + n, E, ops.INTENSITY_STREAMS[1]) >> np.uint32(8)).astype(np.float32)
            u1 = torch.from_numpy(k1) * f(2.0 ** -24) + f(2.0 ** -25)
            u2 = torch.from_numpy(k2) * f(2.0 ** -24) + f(2.0 ** -25)
            nrm = torch.sqrt(f(-2.0) * torch.log(u1)) * torch.cos(f(2.0 * np.pi) * u2)
            v = v + f(p['noise_std']) * nrm.reshape(C, D, H, W)
        if p.get('clamp'):
            v = v.clamp(0, 1)
        x[n] = v
    return x.numpy()


def bias_coefficients(N, shape, mesh, order, seed, scale=0.3):
    """random control-grid coefficients N x gz x gy x gx (float32 values) for a volume D x H x W with `mesh` (x, y, z) cells"""
    gx, gy, gz = (int(m) + order for m in mesh)
    return np.random.RandomState(seed).normal(0, scale / 2, (N, gz, gy, gx)).astype(np.float32)


def max_grid_mesh(order):
    """a mesh (x, y, z) whose control grid holds exactly DA_AUG_MAX_GRID_POINTS = 2048 = 16 x 16 x 8 points"""
    return (16 - order, 16 - order, 8 - order)


if __name__ == '__main__':                                       # the measured float32 distances quoted in the docstring
    for tname, taps in blur_taps().items():
        worst = 0.0
        for sname, shape in blur_shapes().items():
            img = rand_image(shape, 1)
            worst = max(worst, tolerance(blur_reference(img.numpy(), taps), blur_torch32(img, taps))[1])
        print('blur %-8s d32 %.2e' % (tname, worst))
    for name in bilateral_cases():
        _, _, guarded, tol, d32 = bilateral_expected(name)
        print('bilateral %-10s d32 %.2e tol %.2e left out %.4f' % (name, d32, tol, guarded.mean()))
    for stage, p in STAGES.items():
        shape = pointwise_shapes()['ragged']
        img = rand_image(shape, 2)
        coef = bias_coefficients(1, shape[2:], (2, 2, 2), 2, 9) if p.get('bias') else None
        ref = intensity_reference(img.numpy(), [p], coef)
        print('pointwise %-10s d32 %.2e' % (stage, tolerance(ref, intensity_torch32(img, [p], coef))[1]))
