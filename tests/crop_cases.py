"""Inputs and numpy references of the crop kernels (csrc/crop.hip), shared by test_gpu_crop.py and its CPU companion
test_crop_reference.py.  TEST INFRASTRUCTURE ONLY: nothing here runs on the GPU."""
import functools

import numpy as np

from oracle.datapath import _synth_bits

CROP_STREAM = 4                                     # DA_CROP_STREAM (csrc/counter_hash.h)
THRESHOLDS = (0.01, 0.05, 0.2)

# (shape, window): odd sizes, a row longer than one wave (70), longer than two waves (130) and longer than a workgroup (300), a window equal
# to the volume (one start), windows of one voxel and of whole axes
COUNT_CASES = [((12, 20, 70), (4, 8, 33)), ((9, 17, 130), (8, 16, 64)), ((16, 16, 32), (16, 16, 32)), ((5, 6, 7), (1, 1, 1)),
               ((5, 6, 7), (5, 1, 7)), ((3, 4, 300), (2, 3, 257))]
MAIN = ((12, 20, 70), (4, 8, 33))                   # admissible sets neither empty nor the whole domain at every threshold
FALLBACK = ((9, 17, 130), (8, 16, 64))              # nothing admissible at 0.2
SINGLE = ((16, 16, 32), (16, 16, 32))               # one start


@functools.lru_cache(maxsize=None)
def ellipsoid_labels(shape, seed=0, n=1):
    """n label maps of `shape`: two ellipsoids of classes 1 and 2 plus 2 % of the voxels relabelled at random from {0, 1, 2}.  uint8,
    read-only (shared among the tests)."""
    rng = np.random.RandomState(1000 + seed)
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    out = np.zeros((n,) + tuple(shape), dtype=np.uint8)
    for k in range(n):
        lab = np.zeros(shape, dtype=np.uint8)
        for cls, (cz, cy, cx), (rz, ry, rx) in ((1, (0.35, 0.4, 0.3), (0.3, 0.26, 0.2)), (2, (0.65, 0.6, 0.7), (0.25, 0.25, 0.15))):
            cz, cy, cx = cz + 0.05 * rng.rand(), cy + 0.05 * rng.rand(), cx + 0.05 * rng.rand()
            inside = ((z / D - cz) / rz) ** 2 + ((y / H - cy) / ry) ** 2 + ((x / W - cx) / rx) ** 2 <= 1.0
            lab[inside] = cls
        flip = rng.rand(*shape) < 0.02
        lab[flip] = rng.randint(0, 3, size=int(flip.sum())).astype(np.uint8)
        out[k] = lab
    out.setflags(write=False)
    return out


def integral_counts(labels, window, cls):
    """Window counts of one class from a zero-padded integral image: labels [N][D][H][W] -> int64 [N][D - wd + 1][H - wh + 1][W - ww + 1]."""
    wd, wh, ww = window
    m = (np.asarray(labels) == cls).astype(np.int64)
    S = np.zeros((m.shape[0], m.shape[1] + 1, m.shape[2] + 1, m.shape[3] + 1), dtype=np.int64)
    S[:, 1:, 1:, 1:] = m.cumsum(1).cumsum(2).cumsum(3)
    a, b = S[:, wd:], S[:, :-wd]
    a, b = a[:, :, wh:] - a[:, :, :-wh], b[:, :, wh:] - b[:, :, :-wh]
    return (a[:, :, :, ww:] - a[:, :, :, :-ww]) - (b[:, :, :, ww:] - b[:, :, :, :-ww])


def brute_counts(labels, window, cls):
    """The same by the definition, one window at a time."""
    wd, wh, ww = window
    N, D, H, W = labels.shape
    out = np.zeros((N, D - wd + 1, H - wh + 1, W - ww + 1), dtype=np.int64)
    for n in range(N):
        for z in range(out.shape[1]):
            for y in range(out.shape[2]):
                for x in range(out.shape[3]):
                    out[n, z, y, x] = int((labels[n, z:z + wd, y:y + wh, x:x + ww] == cls).sum())
    return out


def domain(shape, window, include_last=False):
    return tuple((s - w + 1) if include_last else max(s - w, 1) for s, w in zip(shape, window))


def min_count(threshold, size):
    """Smallest integer n with n / size > threshold in float64, by search (the reference's comparison; crop_min_count is tested against it)."""
    for n in range(size + 2):
        if np.float64(n) / np.float64(size) > np.float64(threshold):
            return n
    return size + 1


def draw_bits(seed, sample0, n, p):
    ctr = np.asarray([np.uint64(sample0 + n) * np.uint64(65536) + np.uint64(p)], dtype=np.uint64)
    return int(_synth_bits(seed, ctr, CROP_STREAM)[0])


def ref_starts(labels, window, classes, min_counts, seed, sample0=0, include_last=False):
    """The definition of ops.sample_crop_starts, restated: (starts int32 [N][P][3], info int32 [N][P][2])."""
    labels = np.asarray(labels)
    N = labels.shape[0]
    dom = domain(labels.shape[1:], window, include_last)
    P = len(classes)
    starts = np.zeros((N, P, 3), dtype=np.int32)
    info = np.zeros((N, P, 2), dtype=np.int32)
    cache = {}
    for p, (c, m) in enumerate(zip(classes, min_counts)):
        if c is not None and c not in cache:
            cache[c] = integral_counts(labels, window, c)[:, :dom[0], :dom[1], :dom[2]]
        for n in range(N):
            bits = draw_bits(seed, sample0, n, p)
            if c is None:
                size = dom[0] * dom[1] * dom[2]
                k = (bits * size) >> 32
                starts[n, p] = np.unravel_index(k, dom)
                info[n, p] = (size, -1)
                continue
            cnt = cache[c][n].reshape(-1)
            adm = np.flatnonzero(cnt >= m)                                   # raster order
            flat = int(adm[(bits * adm.size) >> 32]) if adm.size else int(np.argmax(cnt))       # (argmax: the first of the largest)
            starts[n, p] = np.unravel_index(flat, dom)
            info[n, p] = (adm.size, cnt[flat])
    return starts, info


def rejection_loop(labels3, window, cls, threshold, rng, max_tries=100000):
    """The reference's loop (lib/transforms.py:445-457 with random_3d_coordinates :497-505) restated on a numpy label map D x H x W: draws a
    start per axis with randint(0, S - w) (0 where S - w is not positive), until the share of `cls` in the crop exceeds threshold.
    Returns ((z, y, x), number of tries)."""
    wd, wh, ww = window
    D, H, W = labels3.shape
    for tries in range(1, max_tries + 1):
        z, y, x = (int(rng.randint(0, r)) if r > 0 else 0 for r in (D - wd, H - wh, W - ww))
        crop = labels3[z:z + wd, y:y + wh, x:x + ww]
        if np.sum(crop == cls) / crop.size > threshold:
            return (z, y, x), tries
    raise RuntimeError('no admissible crop in %d tries' % max_tries)
