"""Shared by tests/test_gpu_blend.py (the kernels of blend.hip, the predictor, the experiment and predict_seg.py on the device) and
tests/test_blend_reference.py (the reference and the host-side pieces, no GPU): the cases, the float64 reference, the float32 torch evaluation
that sets the tolerance, and the guard band.  TEST INFRASTRUCTURE ONLY: nothing here runs on the GPU.

Reference (`reference`).  From the float32 tile logits: the softmax in float64; the covering sets from a plain restatement of Partition's
geometry -- the volume's voxel numbers are reflect-padded with numpy.pad and every tile is a slice of that padded index map, positions that
came from the padding take no part --; the weighted sums in float64 (the window = the float64 product of the float32 tables); argmax and
confidence of the sums.  A flip mask is applied by un-mirroring the logits first (numpy.flip).

Tolerance (`tolerance`).  The project's convention: 4 x the distance of the float32 torch evaluation of the same formula (`evaluate_f32`:
torch.softmax in float32, the float32 window product, float32 adds in ascending tile order) from the float64 reference ON THE SAME CASE.
Distances are the largest |acc - acc64| / (weight sum of the voxel) over voxels and classes.  It is never taken from the kernel's output.
Guard band: labels (and the confidence) are compared where the float64 margin between the two largest sums exceeds tolerance x the voxel's
weight sum; the excluded share must stay <= 0.1 % of the voxels of every case, which tests/test_blend_reference.py shows for the reference alone.

Measured (MI355X, all cases, both windows, flip masks 0 ... 7): see MEASURED below -- the worst ratio kernel distance / float32 torch
distance (1.87, against the factor 4) and the two distances at that case; over the other cases the ratio lies in 0.89 ... 1.59.

Plain module, no fixtures, no pytest settings."""
import functools

import numpy as np
import torch

SEED = 20261
FACTOR = 4.0                       # tolerance = FACTOR x the float32 torch evaluation's distance
MAX_EXCLUDED = 1e-3                # share of voxels the guard band may exclude, per case

# worst over all (case, K, window, flip): kernel distance / float32 torch distance, and the two distances there (filled in from the device run)
MEASURED = {'worst_ratio': 1.868, 'kernel_distance': 1.051e-07, 'torch_distance': 5.628e-08, 'case': 'shape 0, K = 256, constant window, flip 2'}

# (volume, tile, overlap) in (z, y, x); the smallest shapes at which the indexing can go wrong
SHAPES = [
    ((5, 7, 9), (4, 5, 6), (1, 1, 2)),           # 45 tiles, up to 12 tiles on a voxel, ragged last tiles on every axis
    ((8, 8, 8), (4, 4, 4), (0, 0, 0)),           # one tile per voxel
    ((6, 6, 6), (8, 8, 8), (1, 1, 1)),           # a single tile larger than the volume
    ((16, 16, 16), (8, 8, 8), (2, 2, 2)),        # overlap t / 4, 8 tiles on an interior voxel
]
KS = (2, 3, 5, 32, 33)
CASES = [(s, K) for s in range(len(SHAPES)) for K in KS] + [(0, 256)]
WINDOWS = ('gaussian', 'constant')
FLIPS = tuple(range(8))
FLIP_AXES = {1: 1, 2: 2, 4: 3}                   # flip bit -> axis of a [T][tz][ty][tx][K] array

BLOCK = 256
GRID_CAP = 256 * 16                # common.h da_grid's default cap


def da_grid(work_items, block=BLOCK, cap=GRID_CAP):
    """common.h da_grid: ceil(work / block) blocks, at least 1, at most `cap`."""
    return max(1, min(cap, -(-int(work_items) // block)))


def lanes(K):
    """blend.hip bd_lanes for 16-byte aligned tensors: lanes that share a voxel."""
    q = K // 4
    if K % 4 == 0 and q & (q - 1) == 0 and q <= 64:
        return q
    L = 2
    while L < K and L < 64:
        L *= 2
    return L


# one call whose work items exceed the capped grid, so that the kernel's grid-stride loop runs a second trip: 9 tiles of 16 x 32 x 32 at K = 32
BIG = ((16, 84, 84), (16, 32, 32), (0, 2, 2), 32)


def geometry(vol, tile, overlap):
    """(effective tile, tile grid, number of tiles)."""
    e = tuple(t - 2 * o for t, o in zip(tile, overlap))
    g = tuple(-(-s // a) for s, a in zip(vol, e))
    return e, g, g[0] * g[1] * g[2]


def chunkings(T):
    """Splits of T tiles into calls as (tile0, n): all in one call, one per call, chunks of 4."""
    return {'one call': [(0, T)], 'one per call': [(k, 1) for k in range(T)], 'chunks of 4': [(k, min(4, T - k)) for k in range(0, T, 4)]}


@functools.lru_cache(maxsize=None)
def tile_maps(vol, tile, overlap):
    """Per tile, in raster order: (voxel numbers [tz][ty][tx] of the volume, inside [tz][ty][tx] bool) -- slices of the reflect-padded index map."""
    e, g, T = geometry(vol, tile, overlap)
    pads = [(o, gi * ei + o - s) for o, gi, ei, s in zip(overlap, g, e, vol)]
    idx = np.pad(np.arange(int(np.prod(vol))).reshape(vol), pads, 'reflect')
    inside = np.pad(np.ones(vol, dtype=bool), pads, 'constant', constant_values=False)
    out = []
    for i in range(g[0]):
        for j in range(g[1]):
            for k in range(g[2]):
                sl = (slice(i * e[0], i * e[0] + tile[0]), slice(j * e[1], j * e[1] + tile[1]), slice(k * e[2], k * e[2] + tile[2]))
                out.append((idx[sl], inside[sl]))
    return out


def tables(tile, kind, sigma_scale=0.125):
    from deepatlas_amd.lib.transforms import importance_window
    return importance_window(tile, kind, sigma_scale)


def draw_logits(vol, tile, overlap, K, seed=SEED):
    """float32 [T][tz][ty][tx][K] ~ N(0, 4^2)."""
    _, _, T = geometry(vol, tile, overlap)
    rng = np.random.RandomState(seed + 7 * K + int(np.prod(vol)))
    return (rng.standard_normal((T,) + tuple(tile) + (K,)) * 4.0).astype(np.float32)


def lattice_logits(vol, tile, overlap, K, seed=SEED):
    """Multiples of 0.5, all distinct per voxel of a tile: a permutation of 0 ... K - 1 times 0.5."""
    _, _, T = geometry(vol, tile, overlap)
    rng = np.random.RandomState(seed + K)
    n = T * int(np.prod(tile))
    perm = np.argsort(rng.random_sample((n, K)), axis=1)
    return (perm.astype(np.float32) * 0.5).reshape((T,) + tuple(tile) + (K,))


def unmirror(logits, flip):
    axes = tuple(a for b, a in FLIP_AXES.items() if flip & b)
    return np.flip(logits, axes) if axes else logits


def reference(logits, vol, tile, overlap, win, flip=0, passes=1):
    """float64: (acc [V][K], weight sum [V]); `passes`: the tiles are accumulated that many times over (mirror passes of equal content)."""
    L = unmirror(logits, flip).astype(np.float64)
    z = L - L.max(-1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(-1, keepdims=True)
    w3 = (win[0].astype(np.float64)[:, None, None] * win[1].astype(np.float64)[None, :, None]) * win[2].astype(np.float64)[None, None, :]
    V, K = int(np.prod(vol)), logits.shape[-1]
    acc, wsum = np.zeros((V, K)), np.zeros(V)
    for t, (idx, inside) in enumerate(tile_maps(vol, tile, overlap)):
        v = idx[inside]                                  # every volume voxel appears at most once in a tile's inside part
        acc[v] += w3[inside][:, None] * p[t][inside]
        wsum[v] += w3[inside]
    return acc * passes, wsum * passes


def evaluate_f32(logits, vol, tile, overlap, win, flip=0, passes=1):
    """The same formula in float32 with torch on the host: acc [V][K] float32, tiles added in ascending order, pass after pass."""
    L = torch.from_numpy(np.ascontiguousarray(unmirror(logits, flip)))
    p = torch.softmax(L, -1)
    wz, wy, wx = (torch.from_numpy(np.ascontiguousarray(w)) for w in win)
    w3 = (wz[:, None, None] * wy[None, :, None]) * wx[None, None, :]
    V, K = int(np.prod(vol)), logits.shape[-1]
    acc = torch.zeros((V, K), dtype=torch.float32)
    for t, (idx, inside) in enumerate(tile_maps(vol, tile, overlap) * passes):
        t = t % p.shape[0]
        m = torch.from_numpy(inside)
        v = torch.from_numpy(idx[inside])
        acc[v] = acc[v] + w3[m][:, None] * p[t][m]
    return acc.numpy()


def distance(acc, acc64, wsum):
    """Largest |acc - acc64| / weight sum over voxels and classes."""
    return float((np.abs(acc.astype(np.float64) - acc64) / wsum[:, None]).max())


def labels_conf(acc64):
    """(first-maximum argmax uint8 [V], confidence [V], margin between the two largest sums [V])."""
    lab = acc64.argmax(1)
    top = np.sort(acc64, axis=1)
    return lab.astype(np.uint8), acc64[np.arange(len(lab)), lab] / acc64.sum(1), top[:, -1] - top[:, -2]


@functools.lru_cache(maxsize=None)
def case_data(shape_index, K, window, flip):
    """Everything a test needs of one case, computed once: logits, window tables, acc64, wsum, the tolerance and the float32 distance."""
    vol, tile, overlap = SHAPES[shape_index]
    logits = draw_logits(vol, tile, overlap, K)
    win = tables(tile, window)
    acc64, wsum = reference(logits, vol, tile, overlap, win, flip)
    d32 = distance(evaluate_f32(logits, vol, tile, overlap, win, flip), acc64, wsum)
    for a in (logits, acc64, wsum):
        a.setflags(write=False)
    return {'vol': vol, 'tile': tile, 'overlap': overlap, 'K': K, 'logits': logits, 'win': win, 'acc64': acc64, 'wsum': wsum,
            'd32': d32, 'tol': FACTOR * d32}


def guard(acc64, wsum, tol):
    """Voxels whose label the tolerance cannot change: the float64 margin exceeds the band tol x weight sum."""
    return labels_conf(acc64)[2] > tol * wsum


def running_weight_sums(vol, tile, overlap, win):
    """float32 [V]: the running float32 sum of the covering tiles' weights, in ascending tile order."""
    w3 = ((win[0][:, None, None] * win[1][None, :, None]) * win[2][None, None, :]).astype(np.float32)
    s = np.zeros(int(np.prod(vol)), dtype=np.float32)
    for idx, inside in tile_maps(vol, tile, overlap):
        v = idx[inside]
        s[v] = s[v] + w3[inside]
    return s


def tiles_of_volume(values, vol, tile, overlap):
    """[V][K] per-voxel values of a volume -> [T][tz][ty][tx][K]: what a pointwise function yields on Partition's reflect-padded tiles."""
    return np.stack([values[idx] for idx, _ in tile_maps(vol, tile, overlap)], 0)


def seg_config(tmp_path, flags):
    """The config train_seg.py builds for `flags`, shortened to one small epoch."""
    import train_seg
    seen = []

    class Capture(object):
        def __init__(self, config):
            seen.append(config)

        def train(self):
            pass

        def test(self):
            pass
    real = train_seg.SegmentationExperiment
    train_seg.SegmentationExperiment = Capture
    try:
        train_seg.main(['--num-samples', '2', '--num-epochs', '1', '--log-root', str(tmp_path / 'logs')] + flags)
    finally:
        train_seg.SegmentationExperiment = real
    cfg = seen[0]
    cfg.update(lr_mode='const', samples_per_epoch=4, print_batch_period=1)
    return cfg
