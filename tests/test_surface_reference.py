"""CPU checks of the surface-distance references (surface_cases.py), of the cases' coverage, and of everything of the feature that needs no
GPU: the symbols, the argument errors of the ops, the config parsing and the train_seg.py flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import surface_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['one', 'row', 'col', 'stack', 'small', 'K32']          # few enough surface voxels for the pairwise minimum
SURFACE_SYMBOLS = ('da_label_surface', 'da_surface_dist_ws_bytes', 'da_surface_dist_stats')


def _close(got, want, rtol):
    """Counts and the NaN pattern equal; the five metrics within rtol, relative."""
    assert np.array_equal(got[..., :2], want[..., :2])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= rtol * np.abs(want[ok])), np.abs(got[ok] - want[ok]).max()


@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('name', SMALL)
def test_scipy_equals_the_exhaustive_minimum(name, kind):
    pred, truth = sc.case_maps(name, kind)
    for spacing, rtol in (((1, 1, 1), sc.STAT_RTOL), (sc.ANISO, 1e-12)):
        for connectivity in sc.CONNECTIVITIES:
            a = sc.stats_scipy(pred, truth, sc.case_classes(name), spacing, connectivity)
            b = sc.stats_exhaustive(pred, truth, sc.case_classes(name), spacing, connectivity)
            _close(a, b, rtol)
            if spacing == (1, 1, 1):                                   # the root of an integer: both references take the same one
                assert np.array_equal(a[..., 2], b[..., 2], equal_nan=True)


@pytest.mark.parametrize('connectivity', sc.CONNECTIVITIES)
def test_erosion_form_of_the_surface_equals_the_neighbour_form(connectivity):
    for shape in sc.SURFACE_SHAPES:
        labels = sc.blocky_labels(shape, 4, block=sc.BLOCK, seed=5, n=2)
        assert np.array_equal(sc.label_surface(labels, connectivity), sc.surface_neighbours(labels, connectivity)), shape
    one = np.ones((1, 4, 5, 6), dtype=np.uint8)                        # a class filling the volume: its surface is the volume's shell
    shell = sc.label_surface(one, connectivity)
    assert shell.sum() == 4 * 5 * 6 - 2 * 3 * 4 and not shell[0, 1:-1, 1:-1, 1:-1].any()


def test_percentile_formula_is_numpys():
    r = sc.rng(3)
    for n in (1, 2, 3, 20, 21, 101, 1000):
        x = np.sqrt(r.randint(0, 50, size=n).astype(np.float64))
        for p in (50.0, 95.0, 100.0, 2.5):
            got, want = sc.percentile_formula(x, p), np.percentile(x, p)
            assert abs(got - want) <= sc.STAT_RTOL * abs(want), (n, p, got, want)
        assert sc.percentile_formula(x, 100.0) == x.max()


def test_cases_cover_what_they_are_there_for():
    seen = sc.rank_conditions()
    assert seen['integral'] > 0 and seen['fractional'] > 0 and seen['differ'] > 0, seen
    assert seen['undefined'] > 0 and seen['defined'] >= 100, seen      # (the 32 classes of 'K32' cannot all occur in 702 voxels)
    # the predictions are non-trivial: distances beyond 0 and 1 occur in both kinds, and a noisy prediction is not its truth
    for kind in sc.KINDS:
        ref = sc.case_reference('small', kind)
        assert np.nanmax(ref[..., 2]) > 1.5 and np.nanmin(ref[..., 4]) >= 0.0
    assert sc.STAT_CASES['long'][0][1] > 256 and sc.STAT_CASES['chunks'][0][2] > 64
    pred, truth = sc.case_maps('small', 'shifted')
    assert np.array_equal(pred[:, 1:, 2:, 3:], truth[:, :-1, :-2, :-3]) and not pred[:, 0].any()
    # identical maps: every defined metric is 0
    same = sc.stats_scipy(truth, truth, sc.case_classes('small'))
    assert np.all(same[..., 2:][~np.isnan(same[..., 2:])] == 0.0) and np.array_equal(same[..., 0], same[..., 1])
    # two single voxels: the closed form
    a, b = np.zeros((1, 4, 5, 6), dtype=np.uint8), np.zeros((1, 4, 5, 6), dtype=np.uint8)
    a[0, 0, 0, 0] = b[0, 3, 4, 5] = 1
    far = sc.stats_scipy(a, b, [1], spacing=sc.ANISO)
    d = np.sqrt((3 * sc.ANISO[0]) ** 2 + (4 * sc.ANISO[1]) ** 2 + (5 * sc.ANISO[2]) ** 2)
    assert np.allclose(far[0, 0], [1, 1, d, d, d, d, d], rtol=1e-15)


def test_group_case_spans_two_groups_and_its_reference_is_affordable():
    import time
    V = int(np.prod(sc.GROUP_SHAPE))
    per_group = (128 << 20) // (sc.GROUP_N * V * 4)                    # edt_group of csrc/edt.hip
    assert 1 <= per_group < len(sc.GROUP_CLASSES)
    t0 = time.time()
    ref = sc.group_reference()
    took = time.time() - t0
    print('the two-class scipy reference of the group case took %.2f s' % took)
    assert not np.isnan(ref).any() and ref[..., 2].min() > 1.0


def test_symbols_in_header_signatures_and_library():
    import __graft_entry__ as ge
    from deepatlas_amd import _native, ops
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    declared = set(re.findall(r'\b(da_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(ge.build())
    for name in SURFACE_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert ops.SURFACE_STATS == sc.STATS
    # the entry points refuse bad arguments before any launch (no GPU needed)
    L = _native.lib()
    fake = ctypes.c_void_p(0x1000)
    big = 1 << 40
    ws = L.da_surface_dist_ws_bytes(2, 3, 3, 5, 7)
    assert ws >= L.da_edt_ws_bytes(2, 3, 3, 5, 7) + 2 * 2 * 105 * 4 and L.da_surface_dist_ws_bytes(1, 0, 3, 5, 7) == 0
    assert L.da_surface_dist_ws_bytes(1, 1, 4096, 1, 1) == 0

    def stats(pred=fake, pb=1, truth=fake, tb=8, classes=fake, Kp=3, N=2, D=3, H=5, W=7, sp=(1.0, 1.0, 1.0), conn=6, pct=95.0, out=fake,
              wsp=fake, wsb=big):
        return L.da_surface_dist_stats(pred, pb, truth, tb, classes, Kp, N, D, H, W, sp[0], sp[1], sp[2], conn, pct, out, wsp, wsb, None)
    assert stats(pb=2) == -1 and stats(tb=3) == -1 and stats(conn=4) == -1 and stats(conn=0) == -1
    assert stats(pct=0.0) == -1 and stats(pct=100.5) == -1 and stats(pct=float('nan')) == -1
    assert stats(pred=None) == -1 and stats(truth=None) == -1 and stats(classes=None) == -1 and stats(out=None) == -1 and stats(wsp=None) == -1
    assert stats(Kp=0) == -1 and stats(N=0) == -1 and stats(sp=(1.0, 0.0, 1.0)) == -1
    assert stats(wsb=ws - 1) == -2
    assert stats(D=1, H=1, W=4096) == -3 and stats(Kp=70000) == -3
    assert L.da_label_surface(fake, 1, 1, 3, 5, 7, 5, fake, None) == -1
    assert L.da_label_surface(fake, 2, 1, 3, 5, 7, 6, fake, None) == -1
    assert L.da_label_surface(fake, 1, 1, 3, 5, 7, 6, None, None) == -1
    assert L.da_label_surface(fake, 1, 1, 1, 1, 4096, 6, fake, None) == -3


def test_argument_errors_are_raised_before_the_device():
    from deepatlas_amd import ops, _native
    p = torch.zeros((1, 3, 5, 7), dtype=torch.uint8)
    t = torch.zeros((1, 3, 5, 7), dtype=torch.int64)
    for conn in (4, 8, 27, None, '6'):
        with pytest.raises(ValueError, match='connectivity'):
            ops.surface_distance_stats(p, t, 4, connectivity=conn)
        with pytest.raises(ValueError, match='connectivity'):
            ops.label_surface(p, conn)
    for pct in (0, -1.0, 100.0001, float('nan'), 'x'):
        with pytest.raises(ValueError, match='percentile'):
            ops.surface_distance_stats(p, t, 4, percentile=pct)
    with pytest.raises(ValueError, match='shapes'):
        ops.surface_distance_stats(p, t[:, :, :, :6], 4)
    with pytest.raises(ValueError, match='pred must be'):
        ops.surface_distance_stats(p.float(), t, 4)
    with pytest.raises(ValueError, match='truth must be'):
        ops.surface_distance_stats(p, t.to(torch.int16), 4)
    with pytest.raises(ValueError, match='labels must be'):
        ops.label_surface(p.bool())
    with pytest.raises(ValueError, match='pred must be N x D x H x W'):
        ops.surface_distance_stats(p[0], t[0], 4)
    with pytest.raises(ValueError, match='spacing'):
        ops.surface_distance_stats(p, t, 4, spacing=(1, 0, 1))
    with pytest.raises(ValueError, match='classes'):
        ops.surface_distance_stats(p, t, 4, classes=[1, 4])
    with pytest.raises(ValueError):
        ops.surface_distance_stats(p, t, 1)
    long_row = torch.zeros(1, dtype=torch.uint8).expand(1, 1, 1, 4096)              # zero strides: nothing allocated
    with pytest.raises(ValueError, match='2\\^24'):
        ops.surface_distance_stats(long_row, long_row, 4)
    # n_class has no bound of its own: 256 and more are accepted up to the device check
    with pytest.raises(_native.NativeError):
        ops.surface_distance_stats(p, t, 300)
    # ... and a well-formed call on a host tensor fails loudly: there is no CPU path
    with pytest.raises(_native.NativeError):
        ops.surface_distance_stats(p, t, 4)
    with pytest.raises(_native.NativeError):
        ops.label_surface(p)


def test_surface_metrics_config_parsing():
    from deepatlas_amd.lib import evalMetrics as metrics
    assert metrics.parse_surface_metrics(None) is None
    default = {'spacing': (1.0, 1.0, 1.0), 'connectivity': 6, 'percentile': 95.0, 'classes': None}
    assert metrics.parse_surface_metrics(True) == default and metrics.parse_surface_metrics({}) == default
    got = metrics.parse_surface_metrics({'spacing': [1, 0.7, 2.5], 'connectivity': 26, 'percentile': 50, 'classes': (1, 3)})
    assert got == {'spacing': (1.0, 0.7, 2.5), 'connectivity': 26, 'percentile': 50.0, 'classes': [1, 3]}
    with pytest.raises(ValueError, match='unknown keys'):
        metrics.parse_surface_metrics({'percentil': 95})
    for bad in ('hd95', 6, {'connectivity': 4}, {'percentile': 0}, {'percentile': 101}, {'spacing': (1, 1)}, {'spacing': (1, -1, 1)}):
        with pytest.raises(ValueError):
            metrics.parse_surface_metrics(bad)


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
    train_seg.main(['--surface-metrics'])
    train_seg.main(['--surface-metrics', '--surface-spacing', '1', '0.7', '2.5', '--surface-percentile', '90'])
    train_seg.main(['--surface-percentile', '50'])
    train_seg.main([])
    assert seen[0]['surface_metrics'] == {'spacing': [1.0, 1.0, 1.0], 'percentile': 95.0}
    assert seen[1]['surface_metrics'] == {'spacing': [1.0, 0.7, 2.5], 'percentile': 90.0}
    assert seen[2]['surface_metrics'] == {'spacing': [1.0, 1.0, 1.0], 'percentile': 50.0}
    assert 'surface_metrics' not in seen[3]
    for c in seen:
        assert not {'surface_spacing', 'surface_percentile'} & set(c)
    # the key takes no part in the experiment's name
    assert SegmentationExperiment.experiment_name(seen[1]) == SegmentationExperiment.experiment_name(seen[3])
    # and without it the experiment's suffixes are empty whatever eval_extra holds of the other options
    exp = SegmentationExperiment.__new__(SegmentationExperiment)
    exp.eval_extra = {}
    assert exp._surface_suffix() == '' and exp._post_suffix() == ''
    exp.eval_extra = {'hd95_avg': 1.234, 'assd_avg': 0.5}
    assert exp._surface_suffix() == ', HD95 Avg: 1.23, ASSD Avg: 0.50' and exp._post_suffix() == ''
