"""Inputs and host references of the surface-distance tests (test_surface_reference.py on the CPU, test_gpu_surface.py on the GPU).  Nothing
here calls the code under test.

Definitions (medpy's conventions restated on scipy + numpy), for label maps P and T (N x D x H x W), a class c, a connectivity 6 / 18 / 26
(scipy.ndimage.generate_binary_structure(3, 1 / 2 / 3)) and a spacing (sD, sH, sW):
  * surface of c in L: the voxels with L == c that have a neighbour under the connectivity with L != c or outside the volume
    = A & ~binary_erosion(A, structure, border_value=0) for A = (L == c);
  * d_PT: for every surface voxel of P_c the Euclidean distance to the nearest surface voxel of T_c; d_TP the other way;
  * hd = max(max d_PT, max d_TP); asd_pt = mean d_PT, asd_tp = mean d_TP, assd their mean; hd_pct = numpy's linear percentile of the pooled
    d_PT and d_TP; a class absent from P or T of a sample: the five are NaN, the surface voxel counts are still reported.

References:
  * stats_scipy: binary_erosion + distance_transform_edt(~surface, sampling=spacing) + np.percentile, float64.  Columns as
    ops.SURFACE_STATS: n_pred, n_truth, hd, hd_pct, assd, asd_pred_truth, asd_truth_pred.
  * stats_exhaustive: the pairwise minimum over all surface voxels and the percentile formula written out, for the small cases; holds the
    oracle itself.
  * surface_neighbours: the neighbour form of the surface predicate, against the erosion form.

Tolerances at unit spacing: the counts and hd are exact (d^2 is an integer below 2^24 and its double root is scipy's own); hd_pct, assd and
the two asd get STAT_RTOL = 1e-12 relative: numpy's interpolation and its pairwise summation round differently from a fixed-order double
sum.  With another spacing the transform's own bound, edt_cases.ANISO_RTOL, carries over: max, mean and order statistics are 1-Lipschitz in
the sup norm."""
import functools

import numpy as np
from scipy import ndimage

from edt_cases import blocky_labels, rng, ANISO, ANISO_RTOL  # noqa: F401  (re-exported for the tests)

STATS = ('n_pred', 'n_truth', 'hd', 'hd_pct', 'assd', 'asd_pred_truth', 'asd_truth_pred')
CONNECTIVITIES = (6, 18, 26)
STAT_RTOL = 1e-12
NOISE_SHARE = 0.1
SHIFT = (1, 2, 3)


def structure(connectivity):
    return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])


# ---- references ---------------------------------------------------------------------------------------------------------------------
def surface_of(a, connectivity):
    """Surface of one boolean volume D x H x W, the erosion form."""
    return a & ~ndimage.binary_erosion(a, structure(connectivity), border_value=0)


def label_surface(labels, connectivity):
    """N x D x H x W bool: the voxel is a surface voxel of its own label."""
    out = np.zeros(labels.shape, dtype=bool)
    for n, lab in enumerate(labels):
        for c in np.unique(lab):
            out[n] |= surface_of(lab == c, connectivity)
    return out


def surface_neighbours(labels, connectivity):
    """The same by the definition: some neighbour under the connectivity carries another label or lies outside the volume."""
    order = {6: 1, 18: 2, 26: 3}[connectivity]
    lab = labels.astype(np.int64)
    pad = np.pad(lab, ((0, 0), (1, 1), (1, 1), (1, 1)), constant_values=lab.min() - 1)
    D, H, W = labels.shape[1:]
    out = np.zeros(labels.shape, dtype=bool)
    for dd in (-1, 0, 1):
        for dh in (-1, 0, 1):
            for dw in (-1, 0, 1):
                if not 0 < abs(dd) + abs(dh) + abs(dw) <= order:
                    continue
                out |= pad[:, 1 + dd:1 + dd + D, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W] != lab
    return out


def percentile_formula(x, p):
    """numpy's default (linear) percentile written out: rank h = p / 100 (n - 1), x[floor h] + (h - floor h)(x[ceil h] - x[floor h])."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    h = p / 100.0 * (len(x) - 1)
    lo, hi = int(np.floor(h)), int(np.ceil(h))
    return x[lo] + (h - lo) * (x[hi] - x[lo])


def _directed_scipy(sp, st, spacing):
    """(d_PT, d_TP) float64 of two non-empty surfaces."""
    dt = ndimage.distance_transform_edt(~st, sampling=spacing)
    dp = ndimage.distance_transform_edt(~sp, sampling=spacing)
    return dt[sp], dp[st]


def _directed_exhaustive(sp, st, spacing):
    s = np.asarray(spacing, dtype=np.float64)
    a = np.argwhere(sp).astype(np.float64) * s
    b = np.argwhere(st).astype(np.float64) * s
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return np.sqrt(d2.min(1)), np.sqrt(d2.min(0))


def _stats(pred, truth, classes, spacing, connectivity, percentile, directed, pct):
    spacing = tuple(float(s) for s in spacing)
    out = np.full((pred.shape[0], len(classes), len(STATS)), np.nan, dtype=np.float64)
    for n in range(pred.shape[0]):
        for j, c in enumerate(classes):
            sp, st = surface_of(pred[n] == c, connectivity), surface_of(truth[n] == c, connectivity)
            out[n, j, 0], out[n, j, 1] = sp.sum(), st.sum()
            if not sp.any() or not st.any():
                continue
            d_pt, d_tp = directed(sp, st, spacing)
            out[n, j, 2] = max(d_pt.max(), d_tp.max())
            out[n, j, 3] = pct(np.concatenate([d_pt, d_tp]), percentile)
            out[n, j, 5], out[n, j, 6] = d_pt.mean(), d_tp.mean()
            out[n, j, 4] = (out[n, j, 5] + out[n, j, 6]) / 2
    return out


def stats_scipy(pred, truth, classes, spacing=(1, 1, 1), connectivity=6, percentile=95.0):
    """N x K' x 7 float64, the reference of ops.surface_distance_stats."""
    return _stats(pred, truth, classes, spacing, connectivity, percentile, _directed_scipy, np.percentile)


def stats_exhaustive(pred, truth, classes, spacing=(1, 1, 1), connectivity=6, percentile=95.0):
    """The same from pairwise minima over the surface voxels and percentile_formula (small cases only: O(surface^2))."""
    return _stats(pred, truth, classes, spacing, connectivity, percentile, _directed_exhaustive, percentile_formula)


# ---- label maps ---------------------------------------------------------------------------------------------------------------------
def noisy(truth, n_labels, seed, share=NOISE_SHARE):
    """The truth with `share` of its voxels relabelled at random."""
    r = rng(seed)
    out = truth.copy()
    hit = r.rand(*truth.shape) < share
    out[hit] = r.randint(0, n_labels, size=int(hit.sum())).astype(truth.dtype)
    return out


def shifted(truth, shift=SHIFT):
    """The truth moved by `shift` voxels along (D, H, W) -- by at most extent - 1, so something stays -- background where nothing moves in."""
    out = np.zeros_like(truth)
    D, H, W = truth.shape[1:]
    sd, sh, sw = (min(s, e - 1) for s, e in zip(shift, (D, H, W)))
    out[:, sd:, sh:, sw:] = truth[:, :D - sd, :H - sh, :W - sw]
    return out


# name: (shape, N, n_class, what it is there for)
SURFACE_SHAPES = [(1, 1, 1), (1, 1, 9), (1, 8, 1), (7, 1, 1), (3, 5, 7), (5, 6, 70), (9, 70, 11)]
STAT_CASES = {
    'one':     ((1, 1, 1), 2, 3, 'a single voxel: every face of it is the border'),
    'row':     ((1, 1, 9), 2, 3, 'one row'),
    'col':     ((1, 8, 1), 2, 3, 'one line along H'),
    'stack':   ((7, 1, 1), 2, 3, 'one line along D'),
    'small':   ((3, 5, 7), 2, 4, 'the smallest volume with an interior; batch 2'),
    'chunks':  ((5, 6, 70), 2, 4, 'a row of two 64-lane chunks'),
    'tall':    ((9, 70, 11), 2, 4, 'lines along H longer than a wave'),
    'K32':     ((6, 9, 13), 2, 32, "the registry's class count"),
    'long':    ((3, 260, 5), 1, 4, 'a line longer than EDT_LINE_CHUNK'),
}
STAT_IDS = list(STAT_CASES)
KINDS = ('noisy', 'shifted')
BLOCK = (2, 3, 4)          # smaller blocks than edt_cases' default: every class of a small case has interior AND surface voxels


@functools.lru_cache(maxsize=None)
def case_maps(name, kind):
    """(pred, truth) uint8 N x D x H x W.  Never modified by a test."""
    shape, N, n_class, _ = STAT_CASES[name]
    seed = STAT_IDS.index(name)
    truth = blocky_labels(shape, n_class, block=BLOCK, seed=200 + seed, n=N)
    pred = noisy(truth, n_class, 300 + seed) if kind == 'noisy' else shifted(truth)
    pred.setflags(write=False)
    truth.setflags(write=False)
    return pred, truth


def case_classes(name):
    return list(range(1, STAT_CASES[name][2]))


@functools.lru_cache(maxsize=None)
def case_reference(name, kind, spacing=(1, 1, 1), connectivity=6, percentile=95.0):
    pred, truth = case_maps(name, kind)
    out = stats_scipy(pred, truth, case_classes(name), spacing, connectivity, percentile)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rank_conditions(percentile=95.0):
    """What the pooled segments of the cases cover: {'integral': a segment whose rank h = p / 100 (n - 1) is an integer, 'fractional': one
    whose rank is not, 'differ': one whose two order statistics x[floor h] and x[ceil h] differ, 'defined', 'undefined': segment counts}."""
    seen = {'integral': 0, 'fractional': 0, 'differ': 0, 'defined': 0, 'undefined': 0}
    for name in STAT_IDS:
        for kind in KINDS:
            pred, truth = case_maps(name, kind)
            for n in range(pred.shape[0]):
                for c in case_classes(name):
                    sp, st = surface_of(pred[n] == c, 6), surface_of(truth[n] == c, 6)
                    if not sp.any() or not st.any():
                        seen['undefined'] += 1
                        continue
                    seen['defined'] += 1
                    x = np.sort(np.concatenate(_directed_scipy(sp, st, (1.0, 1.0, 1.0))))
                    h = percentile / 100.0 * (len(x) - 1)
                    seen['integral' if h == np.floor(h) else 'fractional'] += 1
                    seen['differ'] += int(x[int(np.floor(h))] != x[int(np.ceil(h))])
    return seen


# ---- the group loop -----------------------------------------------------------------------------------------------------------------
# N = 2 at 96 x 128 x 160 with 9 classes: the class groups of da_edt_ws_bytes hold 128 MiB / (2 x 96 x 128 x 160 x 4 B) = 8 site sets, so the
# loop runs 8 + 1.  The scipy reference of two of the classes takes about 3 s on the host.
GROUP_SHAPE, GROUP_N, GROUP_CLASSES, GROUP_LABELS = (96, 128, 160), 2, list(range(1, 10)), 10
GROUP_CHECKED = (2, 9)     # the classes compared with scipy: one of the first group, and the one of the second


@functools.lru_cache(maxsize=None)
def group_maps():
    truth = blocky_labels(GROUP_SHAPE, GROUP_LABELS, block=(24, 32, 40), seed=77, n=GROUP_N)
    pred = shifted(noisy(truth, GROUP_LABELS, 78, share=0.001))
    pred.setflags(write=False)
    truth.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def group_reference():
    pred, truth = group_maps()
    return stats_scipy(pred, truth, list(GROUP_CHECKED))
