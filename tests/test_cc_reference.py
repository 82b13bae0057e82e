"""CPU: the host reference of the connected-component ops against the definition, the case generators against their names, the C ABI's
symbols, and every argument error (raised before anything touches the device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cc_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC_SYMBOLS = ('da_cc_ws_bytes', 'da_cc_label', 'da_cc_select', 'da_cc_filter')


@pytest.mark.parametrize('connectivity', cc.CONNECTIVITIES)
def test_scipy_reference_equals_flood_fill(connectivity):
    """The reference (scipy.ndimage.label per class, canonicalised by the smallest raster index) against a breadth-first flood fill."""
    for shape, density, seed in (((3, 5, 7), 0.31, 1), ((6, 7, 8), 0.12, 2), ((6, 7, 8), 0.6, 3), ((1, 1, 9), 0.6, 4), ((2, 1, 3), 1.0, 5)):
        vol = cc.noise(shape, density, seed)[0]
        for n_class in (None, 3):                                  # label 3 is background with n_class = 3
            roots, sizes = cc.ref_roots(vol, connectivity, n_class)
            f_roots, f_sizes = cc.flood_fill_roots(vol, connectivity, n_class)
            assert np.array_equal(roots, f_roots) and np.array_equal(sizes, f_sizes), (shape, density, n_class)
            assert int(sizes.sum()) == int((cc.classes_of(vol, n_class) > 0).sum())
        # scipy numbers the components of one label in the order of their first voxel: what compact=True is compared with
        from scipy import ndimage
        one = (vol == 1)
        comp, k = ndimage.label(one, cc.structure(connectivity))
        assert np.array_equal(cc.ref_compact(cc.ref_roots(one, connectivity)[0]), comp)


def test_case_generators_yield_what_their_names_say():
    from deepatlas_amd import ops
    tile = ops.CC_TILE
    td, th, tw = tile
    shape = cc.ragged_shape(tile)
    assert shape == (2 * td + 1, 2 * th + 3, 2 * tw + 5)
    # seam pairs: two voxels in different tiles, joined exactly under the connectivities of their kind; two labels never
    for kind, offs in cc.SEAM_OFFSETS.items():
        batch = cc.seam_pairs(kind, tile)
        assert batch.shape == (len(offs),) + shape and all(int(v.sum()) == 2 for v in batch)
        for vol in batch:
            pts = np.argwhere(vol > 0)
            assert any(pts[0][i] // tile[i] != pts[1][i] // tile[i] for i in range(3))
            for conn in cc.CONNECTIVITIES:
                n_comp = len(np.unique(cc.ref_roots(vol, conn)[0])) - 1
                assert n_comp == (1 if conn in cc.SEAM_JOINED[kind] else 2), (kind, conn)
        for vol in cc.seam_pairs(kind, tile, second_label=2):
            assert all(len(np.unique(cc.ref_roots(vol, conn)[0])) - 1 == 2 for conn in cc.CONNECTIVITIES)
    # wrap-around: six voxels, six components under every connectivity
    for shp in ((3, 5, 7), shape):
        w = cc.wrap_around(shp)
        assert w.shape[0] == 2 and int(w.sum()) == 6
        for conn in cc.CONNECTIVITIES:
            assert sum(len(np.unique(cc.ref_roots(v, conn)[0])) - 1 for v in w) == 6
    # the serpentine is one component rooted at its first voxel, spanning more than one tile in each axis; cut, it is two
    for shp in ((9, 8, 130), shape):
        path = cc.serpentine_path(shp)
        assert path[0] == (0, 0, 0) and len(set(path)) == len(path)
        for i in range(3):                         # ... in every axis along which the shape has more than one tile
            assert max(p[i] for p in path) // tile[i] == (shp[i] - 1) // tile[i]
        assert all((s - 1) // t >= 1 for s, t in zip(shape, tile))
        whole, cut = cc.serpentine(shp)[0], cc.serpentine(shp, cut=True)[0]
        assert int(whole.sum()) == len(path) and int(cut.sum()) == len(path) - 1
        for conn in cc.CONNECTIVITIES:
            roots, sizes = cc.ref_roots(whole, conn)
            assert set(np.unique(roots)) == {0, 1} and int(sizes[0, 0, 0]) == len(path)
            roots, sizes = cc.ref_roots(cut, conn)
            assert len(np.unique(roots)) == 3 and int(roots[0, 0, 0]) == 1 and int(sizes.sum()) == len(path) - 1
    # checkerboard: every voxel its own component under 6, the set half one component under 26
    board = cc.checkerboard((5, 6, 7))[0]
    assert len(np.unique(cc.ref_roots(board, 6)[0])) - 1 == int(board.sum())
    assert len(np.unique(cc.ref_roots(board, 26)[0])) - 1 == 1
    # ties: equal blobs, the one with the smallest root wins
    tie = cc.blobs((9, 19, 69), [(5, 10, 40), (0, 0, 0), (0, 12, 3)], (2, 3, 4))[0]
    roots, _ = cc.ref_roots(tie, 6)
    stats, winners = cc.ref_stats(tie, roots, 4)
    assert tuple(stats[1]) == (3, 24, 72) and winners == {1: 1} and not stats[2:].any()
    kept, _ = cc.ref_keep_largest(tie, roots, 4)
    assert int(kept.sum()) == 24 and kept[0, 0, 0] == 1


def test_symbols_in_header_signatures_and_library():
    import __graft_entry__ as ge
    from deepatlas_amd import _native
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    declared = set(re.findall(r'\b(da_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(ge.build())
    for name in CC_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert 'cc.hip' in ge.HIP_SOURCES
    from deepatlas_amd import ops
    m = {k: int(v) for k, v in re.findall(r'#define DA_CC_(TILE_[DHW]|MAX_CLASSES) (\d+)', header)}
    assert ops.CC_TILE == (m['TILE_D'], m['TILE_H'], m['TILE_W']) and ops.CC_MAX_CLASSES == m['MAX_CLASSES']
    # the entry points refuse bad arguments before any launch (no GPU needed)
    L = _native.lib()
    fake = ctypes.c_void_p(0x1000)
    assert L.da_cc_ws_bytes(2, 3, 5, 7) >= 2 * 3 * 5 * 7 * 4
    assert L.da_cc_label(fake, 1, 1, 3, 5, 7, 0, 5, fake, fake, fake, 1 << 20, None) == -1          # connectivity 5
    assert L.da_cc_label(fake, 2, 1, 3, 5, 7, 0, 6, fake, fake, fake, 1 << 20, None) == -1          # 2-byte labels
    assert L.da_cc_label(fake, 1, 1, 3, 5, 7, 0, 6, fake, fake, fake, 16, None) == -2               # short workspace
    assert L.da_cc_label(fake, 1, 1, 2048, 1024, 1024, 0, 6, fake, fake, fake, 1 << 20, None) == -3  # 2^31 voxels
    assert L.da_cc_select(fake, 1, fake, 1, 100, 0, fake, fake, None) == -1                         # n_class 0
    assert L.da_cc_select(fake, 1, fake, 1, 100, 1025, fake, fake, None) == -3
    assert L.da_cc_filter(fake, 1, fake, fake, None, 1, 100, 4, 0, 1, fake, None) == -1             # largest without the winners
    assert L.da_cc_filter(fake, 1, fake, fake, fake, 1, 100, 4, 1, 0, fake, None) == -1             # min_size 0
    assert L.da_cc_filter(fake, 1, fake, fake, fake, 1, 100, 4, 2, 1, fake, None) == -1             # unknown mode


def test_argument_errors_are_raised_before_the_device():
    from deepatlas_amd import ops, _native
    lab = torch.zeros((1, 3, 5, 7), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.connected_components(lab, connectivity=5)
    with pytest.raises(ValueError):
        ops.connected_components(lab.float())
    with pytest.raises(ValueError):
        ops.keep_largest_component(lab.float(), 4)
    with pytest.raises(ValueError):
        ops.connected_components(lab[0])                                            # not N x D x H x W
    huge = torch.zeros(1, dtype=torch.uint8).expand(1, 2048, 1024, 1024)          # 2^31 voxels, zero strides: nothing allocated
    for fn in (lambda: ops.connected_components(huge), lambda: ops.keep_largest_component(huge, 4),
               lambda: ops.remove_small_components(huge, 4, 10)):
        with pytest.raises(ValueError, match='2\\^31'):
            fn()
    with pytest.raises(ValueError):
        ops.connected_components(torch.empty((1, 2048, 1024, 1024), dtype=torch.uint8, device='meta'))
    with pytest.raises(ValueError):
        ops.remove_small_components(lab, 4, 0)
    with pytest.raises(ValueError):
        ops.remove_small_components(lab, 4, 10, connectivity=7)
    with pytest.raises(ValueError):
        ops.keep_largest_component(lab, 0)
    with pytest.raises(ValueError):
        ops.keep_largest_component(lab, ops.CC_MAX_CLASSES + 1)
    # ... and a well-formed call on a host tensor fails loudly: there is no CPU path
    with pytest.raises(_native.NativeError):
        ops.connected_components(lab)
    with pytest.raises(_native.NativeError):
        ops.keep_largest_component(lab, 4)


def test_postprocess_config_parsing():
    from deepatlas_amd.lib import evalMetrics as metrics
    assert metrics.parse_postprocess(None) is None
    assert metrics.parse_postprocess('largest_cc') == {'mode': 'largest_cc', 'connectivity': 6, 'min_size': None}
    assert metrics.parse_postprocess({'mode': 'largest_cc', 'connectivity': 26}) == {'mode': 'largest_cc', 'connectivity': 26, 'min_size': None}
    assert metrics.parse_postprocess({'mode': 'min_size', 'connectivity': 18, 'min_size': 50}) == {'mode': 'min_size', 'connectivity': 18, 'min_size': 50}
    for bad in ('largest', {'mode': 'min_size'}, {'mode': 'min_size', 'min_size': 0}, {'mode': 'largest_cc', 'connectivity': 4},
                {'mode': 'largest_cc', 'min_size': 5}, {'mode': 'largest_cc', 'size': 5}, {}, 6):
        with pytest.raises(ValueError):
            metrics.parse_postprocess(bad)


def test_train_seg_flags_parse_into_the_config(monkeypatch):
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    seen = []

    class Fake(object):
        def __init__(self, config):
            seen.append(config)

        def train(self):
            pass

        def test(self):
            pass
    monkeypatch.setattr(train_seg, 'SegmentationExperiment', Fake)
    train_seg.main(['--postprocess', 'largest-cc'])
    train_seg.main(['--postprocess', 'min-size', '--cc-connectivity', '26', '--cc-min-size', '30'])
    train_seg.main(['--postprocess', 'min-size'])
    train_seg.main([])
    assert seen[0]['postprocess'] == {'mode': 'largest_cc', 'connectivity': 6}
    assert seen[1]['postprocess'] == {'mode': 'min_size', 'connectivity': 26, 'min_size': 30}
    assert seen[2]['postprocess'] == {'mode': 'min_size', 'connectivity': 6, 'min_size': 64}
    assert 'postprocess' not in seen[3]
    for c in seen:
        assert not {'cc_connectivity', 'cc_min_size'} & set(c)
    # the key takes no part in the experiment's name
    assert SegmentationExperiment.experiment_name(seen[0]) == SegmentationExperiment.experiment_name(seen[3])
