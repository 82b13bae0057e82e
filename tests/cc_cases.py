"""Cases and host references of the connected-component ops (deepatlas_amd/csrc/cc.hip), shared by test_cc_reference.py (CPU) and
test_gpu_cc.py.  Every result is an integer, every comparison exact.

Reference: per class scipy.ndimage.label(labels == c, structure), canonicalised by the smallest raster index of each component
(ndimage.minimum of an index volume), so that it does not depend on scipy's numbering: root map = 0 on background, elsewhere 1 + that
index; size map = the component's voxel count at its root's position.  The largest component of a class is np.unique(return_counts) +
argmax, whose first maximum is the smallest root.  A breadth-first flood fill in plain numpy (flood_fill_roots) holds this reference to the
definition on small shapes.
"""
import collections

import numpy as np
from scipy import ndimage

CONNECTIVITIES = (6, 18, 26)
_RANK = {6: 1, 18: 2, 26: 3}


def structure(connectivity):
    return ndimage.generate_binary_structure(3, _RANK[connectivity])


def classes_of(vol, n_class=None):
    """The class of every voxel: labels <= 0 and, with n_class, labels >= n_class are background."""
    lab = np.asarray(vol).astype(np.int64)
    lab[lab < 0] = 0
    if n_class:
        lab[lab >= n_class] = 0
    return lab


def ref_roots(vol, connectivity, n_class=None):
    """One sample D x H x W -> (root map, size map), both int32."""
    lab = classes_of(vol, n_class)
    idx = np.arange(lab.size, dtype=np.int64).reshape(lab.shape)
    roots = np.zeros(lab.shape, dtype=np.int32)
    sizes = np.zeros(lab.size, dtype=np.int32)
    for c in np.unique(lab):
        if c == 0:
            continue
        comp, k = ndimage.label(lab == c, structure(connectivity))
        mins = np.asarray(ndimage.minimum(idx, comp, index=np.arange(1, k + 1))).astype(np.int64).reshape(-1)
        m = comp > 0
        roots[m] = (mins[comp[m] - 1] + 1).astype(np.int32)
        sizes[mins] = np.bincount(comp.ravel(), minlength=k + 1)[1:]
    return roots, sizes.reshape(lab.shape)


def ref_compact(roots):
    """Components renumbered 1..K in the order of their roots."""
    uniq = np.unique(roots[roots > 0])
    out = np.zeros(roots.shape, dtype=np.int32)
    m = roots > 0
    out[m] = np.searchsorted(uniq, roots[m]).astype(np.int32) + 1
    return out


def ref_stats(vol, roots, n_class):
    """(stats int64 [n_class][3] = (components, largest size, voxels), winners {class: root map value of the largest component})."""
    lab = classes_of(vol, n_class)
    stats = np.zeros((n_class, 3), dtype=np.int64)
    winners = {}
    for c in range(1, n_class):
        r = roots[lab == c]
        if r.size == 0:
            continue
        u, cnt = np.unique(r, return_counts=True)
        k = int(np.argmax(cnt))                    # the first maximum: the smallest root among the largest
        winners[c] = int(u[k])
        stats[c] = (len(u), int(cnt[k]), r.size)
    return stats, winners


def ref_keep_largest(vol, roots, n_class):
    stats, winners = ref_stats(vol, roots, n_class)
    lab = classes_of(vol, n_class)
    out = np.zeros_like(np.asarray(vol))
    for c, win in winners.items():
        m = (lab == c) & (roots == win)
        out[m] = c
    return out, stats


def ref_remove_small(vol, roots, sizes, n_class, min_size):
    lab = classes_of(vol, n_class)
    out = np.zeros_like(np.asarray(vol))
    m = roots > 0
    size_of = np.zeros(lab.shape, dtype=np.int64)
    size_of[m] = sizes.reshape(-1)[roots[m] - 1]
    keep = m & (size_of >= min_size)
    out[keep] = lab[keep]
    return out


Reference = collections.namedtuple('Reference', 'roots sizes compact class_roots class_sizes largest stats')
_CACHE = {}


def reference(name, batch, connectivity, n_class):
    """Reference of a whole batch N x D x H x W (sample by sample), computed once per (case name, connectivity) and shared by the tests.
    roots / sizes / compact are those of connected_components (no n_class); class_roots / class_sizes the maps with labels >= n_class as
    background, largest / stats what keep_largest_component(n_class) returns."""
    key = (name, connectivity, n_class)
    if key not in _CACHE:
        per = []
        for vol in batch:
            roots, sizes = ref_roots(vol, connectivity)
            roots_c, sizes_c = ref_roots(vol, connectivity, n_class)
            largest, stats = ref_keep_largest(vol, roots_c, n_class)
            per.append((roots, sizes, ref_compact(roots), roots_c, sizes_c, largest, stats))
        ref = Reference(*[np.stack([p[i] for p in per]) for i in range(7)])
        for a in ref:
            a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def flood_fill_roots(vol, connectivity, n_class=None):
    """The definition itself: breadth-first search over the voxels in raster order; the first voxel of a component found is its smallest raster index."""
    lab = classes_of(vol, n_class)
    D, H, W = lab.shape
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
            if 0 < (a != 0) + (b != 0) + (c != 0) <= _RANK[connectivity]]
    roots = np.zeros(lab.shape, dtype=np.int32)
    sizes = np.zeros(lab.shape, dtype=np.int32)
    for d in range(D):
        for h in range(H):
            for w in range(W):
                if lab[d, h, w] == 0 or roots[d, h, w] != 0:
                    continue
                root = (d * H + h) * W + w + 1
                roots[d, h, w] = root
                queue = collections.deque([(d, h, w)])
                n = 0
                while queue:
                    z, y, x = queue.popleft()
                    n += 1
                    for a, b, c in offs:
                        p = (z + a, y + b, x + c)
                        if 0 <= p[0] < D and 0 <= p[1] < H and 0 <= p[2] < W and lab[p] == lab[d, h, w] and roots[p] == 0:
                            roots[p] = root
                            queue.append(p)
                sizes[d, h, w] = n
    return roots, sizes


# ------------------------------------------------------------------------------------------------
# case generators: every one returns a batch N x D x H x W
# ------------------------------------------------------------------------------------------------
def ragged_shape(tile):
    td, th, tw = tile
    return (2 * td + 1, 2 * th + 3, 2 * tw + 5)


def noise(shape, density, seed, n_labels=3, dtype=np.uint8):
    """Labels 1..n_labels on a `density` share of the voxels."""
    rng = np.random.default_rng(seed)
    vol = rng.integers(1, n_labels + 1, size=shape)
    vol[rng.random(shape) >= density] = 0
    return vol.astype(dtype)[None]


# offsets of a voxel pair that straddles a tile face / edge / corner, with the negative directions that following neighbours take
SEAM_OFFSETS = {
    'face': [(0, 0, 1), (0, 1, 0), (1, 0, 0)],
    'edge': [(0, 1, 1), (0, 1, -1), (1, 0, 1), (1, 0, -1), (1, 1, 0), (1, -1, 0)],
    'corner': [(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)],
}
SEAM_JOINED = {'face': (6, 18, 26), 'edge': (18, 26), 'corner': (26,)}


def seam_pairs(kind, tile, second_label=1):
    """One sample per offset of SEAM_OFFSETS[kind]: two voxels whose every non-zero offset component crosses a tile boundary, all else 0."""
    td, th, tw = tile
    shape = ragged_shape(tile)
    out = []
    for off in SEAM_OFFSETS[kind]:
        a = [td - 1 if off[0] >= 0 else td, th - 1 if off[1] >= 0 else th, tw - 1 if off[2] >= 0 else tw]
        b = [a[i] + off[i] for i in range(3)]
        for i, t in enumerate(tile):
            assert off[i] == 0 or a[i] // t != b[i] // t
        vol = np.zeros(shape, dtype=np.uint8)
        vol[tuple(a)] = 1
        vol[tuple(b)] = second_label
        out.append(vol)
    return np.stack(out)


def wrap_around(shape):
    """N = 2, one label: voxel pairs that are consecutive (or one row / plane apart) in the raster but not neighbours in the volume."""
    D, H, W = shape
    vol = np.zeros((2,) + tuple(shape), dtype=np.uint8)
    vol[0, 0, 0, W - 1] = 1
    vol[0, 0, 1, 0] = 1                   # w = W - 1 of one row, w = 0 of the next
    vol[0, 1, H - 1, 2] = 1
    vol[0, 2, 0, 2] = 1                   # h = H - 1 of one plane, h = 0 of the next
    vol[0, D - 1, H - 1, W - 1] = 1
    vol[1, 0, 0, 0] = 1                   # the last voxel of sample 0, the first of sample 1
    return vol


def serpentine_path(shape):
    """The voxels, in order, of a one-voxel-wide path from (0, 0, 0): every second row of every second plane, joined by single voxels at
    alternating ends.  Two parts of the path are never neighbours under any connectivity except along the path."""
    D, H, W = shape
    plane = []
    for k, h in enumerate(range(0, H, 2)):
        ws = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        plane += [(h, w) for w in ws]
        if h + 2 < H:
            plane.append((h + 1, plane[-1][1]))
    path = []
    for k, d in enumerate(range(0, D, 2)):
        pl = plane if k % 2 == 0 else plane[::-1]
        path += [(d, h, w) for h, w in pl]
        if d + 2 < D:
            path.append((d + 1,) + pl[-1])
    return path


def serpentine(shape, cut=False):
    path = serpentine_path(shape)
    vol = np.zeros((1,) + tuple(shape), dtype=np.uint8)
    for p in path:
        vol[(0,) + p] = 1
    if cut:
        mid = len(path) // 2
        while not (path[mid - 1][:2] == path[mid][:2] == path[mid + 1][:2]):         # inside a row: its neighbours on the path are its only ones
            mid += 1
        vol[(0,) + path[mid]] = 0
    return vol


def checkerboard(shape):
    d, h, w = np.indices(shape)
    return (((d + h + w) % 2) == 0).astype(np.uint8)[None]


def blobs(shape, corners, size, label=1, dtype=np.uint8):
    """Boxes of `size` = (sd, sh, sw) voxels of one class at the given corners, apart from each other."""
    vol = np.zeros((1,) + tuple(shape), dtype=dtype)
    for d, h, w in corners:
        vol[0, d:d + size[0], h:h + size[1], w:w + size[2]] = label
    return vol
