"""CPU: the references of edt_cases.py hold each other, and the host side of the distance-transform feature (registry, symbols, argument
checks, config parsing).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import edt_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDT_SYMBOLS = ['da_edt_ws_bytes', 'da_edt_sq', 'da_signed_distance_maps', 'da_boundary_loss_ws_bytes', 'da_boundary_loss_fwd', 'da_boundary_loss_bwd']
SMALL = [(1, 1, 1), (1, 1, 9), (3, 5, 7), (1, 6, 4), (4, 1, 5)]


@pytest.mark.parametrize('shape', SMALL)
def test_scipy_equals_the_exhaustive_minimum(shape):
    for name, sites in ec.site_patterns(shape, seed=3):
        mask = (~sites)[None].astype(np.uint8)
        want = ec.edt_sq_exhaustive(mask)
        assert np.array_equal(ec.edt_sq_scipy(mask), want), (shape, name)
        if not sites.any():
            assert np.isinf(want).all()
        a64 = ec.edt_sq_scipy(mask, ec.ANISO)
        ex = ec.edt_sq_exhaustive(mask, ec.ANISO)
        fin = np.isfinite(ex)
        assert np.array_equal(fin, np.isfinite(a64)) and np.allclose(a64[fin], ex[fin], rtol=1e-12, atol=0), (shape, name)


def test_rint_of_the_squared_distance_is_the_integer_from_the_indices():
    """np.rint(d^2) of scipy's float64 distances equals the squared distance computed in integers from return_indices: exact comparison of
    the squared transform at unit spacing is justified."""
    for shape, seed in (((3, 5, 7), 1), ((9, 17, 130), 2), ((40, 3, 33), 3)):
        for name, sites in ec.site_patterns(shape, seed=seed):
            if not sites.any():
                continue
            d, idx = ndimage.distance_transform_edt(~sites, return_indices=True)
            grid = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing='ij'))
            d2 = ((grid.astype(np.int64) - idx.astype(np.int64)) ** 2).sum(0)
            assert np.array_equal(np.rint(d * d).astype(np.int64), d2), (shape, name)
            assert np.array_equal(ec.edt_sq_scipy((~sites)[None].astype(np.uint8))[0], d2.astype(np.float64))
            assert d2.max() < 2 ** 24


def test_signed_maps_reference():
    lab = ec.blocky_labels((6, 9, 13), 4, seed=5, n=2)
    lab[1] = 2                                                   # sample 1: class 2 fills it, the others are absent
    phi = ec.signed_maps(lab, [1, 2, 3])
    assert not phi[1].any()
    for j, c in enumerate([1, 2, 3]):
        inside = lab[0] == c
        assert inside.any() and not inside.all()
        assert (phi[0, j][inside] <= -1).all() and (phi[0, j][~inside] >= 1).all()
    # a one-voxel structure: -1 inside (the nearest outside voxel is a face neighbour), the Euclidean distance outside
    one = np.zeros((1, 3, 4, 5), dtype=np.uint8)
    one[0, 1, 2, 3] = 1
    p = ec.signed_maps(one, [1])[0, 0]
    assert p[1, 2, 3] == -1 and p[1, 2, 0] == 3 and p[0, 0, 0] == np.sqrt(1 + 4 + 9)


@pytest.mark.parametrize('name', ['K4', 'K8', 'K5', 'K32'])
def test_float64_boundary_loss_against_the_hand_written_gradient(name):
    z, phi = ec.loss_inputs(name)
    cl = ec.case_classes(name)
    l64, g64 = ec.loss_reference(name)
    want = ec.boundary_grad_formula(z, phi, cl)
    assert float((g64 - want).abs().max()) <= 1e-13 * float(want.abs().max()) + 1e-300
    # the value, written out
    p = torch.softmax(z.double(), 1)
    N, K = z.shape[:2]
    total = sum(float((p[:, c] * phi[:, j].double()).sum()) for j, c in enumerate(cl))
    assert abs(l64 - total / (N * len(cl) * z[0, 0].numel())) <= 1e-13 * abs(l64)
    assert float(z.abs().max()) == ec.LOGIT_MAX
    lb, gb = ec.loss_bounds(name)
    assert ec.LOSS_FLOOR <= lb < 1e-5 and ec.GRAD_FLOOR <= gb < 1e-4


def test_registry_lists_are_unchanged_and_boundary_is_reachable():
    from deepatlas_amd.lib import loss
    assert loss.get_available_losses() == ['ncc', 'lncc', 'mse', 'gradient', 'bendingEnergy', 'dice', 'L2', 'focal', 'cross_entropy', 'soft_cross_entropy']
    assert loss.get_extension_losses() == ['mi']
    assert loss.get_regulariser_losses() == ['jacobian']
    assert loss.get_field_pair_losses() == ['inverse_consistency']
    assert loss.get_label_distance_losses() == ['boundary']
    assert loss.get_loss_function('boundary') is loss.BoundaryLoss
    crit = loss.BoundaryLoss(5)
    assert crit.classes == [1, 2, 3, 4] and crit.spacing == (1.0, 1.0, 1.0)
    assert loss.BoundaryLoss(5, classes=[0, 3], spacing=(1, 0.5, 2)).classes == [0, 3]
    for bad in (dict(n_class=1), dict(n_class=4, classes=[1, 1]), dict(n_class=4, classes=[4]), dict(n_class=4, classes=[]),
                dict(n_class=4, spacing=(1, 0, 1)), dict(n_class=4, spacing=(1, 1)), dict(n_class=4, spacing=(1, float('inf'), 1))):
        with pytest.raises(ValueError):
            loss.BoundaryLoss(**bad)


def test_symbols_in_header_signatures_and_library():
    import __graft_entry__ as ge
    from deepatlas_amd import _native, ops
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    declared = set(re.findall(r'\b(da_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(ge.build())
    for name in EDT_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert 'edt.hip' in ge.HIP_SOURCES
    assert ops.EDT_LINE_CHUNK == int(re.search(r'#define DA_EDT_LINE_CHUNK (\d+)', header).group(1))
    # the entry points refuse bad arguments before any launch (no GPU needed)
    L = _native.lib()
    fake = ctypes.c_void_p(0x1000)
    big = 1 << 40
    assert L.da_edt_ws_bytes(2, 1, 3, 5, 7) >= 2 * 2 * 3 * 5 * 7 * 4
    assert L.da_edt_ws_bytes(1, 3, 3, 5, 7) >= 2 * 3 * 3 * 5 * 7 * 4
    assert L.da_edt_ws_bytes(1, 1, 4096, 1, 1) == 0 and L.da_edt_ws_bytes(1, 0, 3, 5, 7) == 0
    assert L.da_edt_sq(fake, 2, 1, 3, 5, 7, 1.0, 1.0, 1.0, 0, fake, fake, big, None) == -1           # 2-byte mask
    assert L.da_edt_sq(fake, 1, 1, 3, 5, 7, 1.0, 0.0, 1.0, 0, fake, fake, big, None) == -1           # spacing 0
    assert L.da_edt_sq(fake, 1, 1, 3, 5, 7, 1.0, 1.0, float('nan'), 0, fake, fake, big, None) == -1
    assert L.da_edt_sq(fake, 1, 0, 3, 5, 7, 1.0, 1.0, 1.0, 0, fake, fake, big, None) == -1
    assert L.da_edt_sq(None, 1, 1, 3, 5, 7, 1.0, 1.0, 1.0, 0, fake, fake, big, None) == -1
    assert L.da_edt_sq(fake, 1, 1, 3, 5, 7, 1.0, 1.0, 1.0, 0, fake, fake, 16, None) == -2            # short workspace
    assert L.da_edt_sq(fake, 1, 1, 1, 1, 4096, 1.0, 1.0, 1.0, 0, fake, fake, big, None) == -3        # W^2 = 2^24
    assert L.da_edt_sq(fake, 1, 1, 2365, 2365, 2365, 1.0, 1.0, 1.0, 0, fake, fake, big, None) == -3  # 3 x 2365^2 >= 2^24
    assert L.da_edt_sq(fake, 1, 1, 1300, 1300, 1300, 1.0, 1.0, 1.0, 0, fake, fake, big, None) == -3  # 2^31 voxels below the extent bound
    assert L.da_signed_distance_maps(fake, 1, fake, 0, 1, 3, 5, 7, 1.0, 1.0, 1.0, fake, fake, big, None) == -1     # no class
    assert L.da_signed_distance_maps(fake, 1, None, 2, 1, 3, 5, 7, 1.0, 1.0, 1.0, fake, fake, big, None) == -1
    assert L.da_signed_distance_maps(fake, 3, fake, 2, 1, 3, 5, 7, 1.0, 1.0, 1.0, fake, fake, big, None) == -1
    assert L.da_signed_distance_maps(fake, 1, fake, 2, 1, 3, 5, 7, 1.0, 1.0, 1.0, fake, fake, 16, None) == -2
    assert L.da_signed_distance_maps(fake, 1, fake, 2, 1, 4000, 1000, 1, 1.0, 1.0, 1.0, fake, fake, big, None) == -3
    assert L.da_boundary_loss_ws_bytes(2) >= 2 * 8 and L.da_boundary_loss_ws_bytes(0) == 0
    assert L.da_boundary_loss_fwd(fake, fake, fake, 1, 100, 8, 9, fake, fake, big, None) == -1       # more chosen classes than channels
    assert L.da_boundary_loss_fwd(fake, fake, None, 1, 100, 8, 7, fake, fake, big, None) == -1
    assert L.da_boundary_loss_fwd(fake, fake, fake, 1, 100, 8, 7, fake, fake, 8, None) == -2
    assert L.da_boundary_loss_fwd(fake, fake, fake, 1, 100, 65, 7, fake, fake, big, None) == -3
    assert L.da_boundary_loss_fwd(fake, fake, fake, 1, 2 ** 31, 8, 7, fake, fake, big, None) == -3
    assert L.da_boundary_loss_bwd(fake, fake, fake, None, 1, 100, 8, 7, fake, None) == -1
    assert L.da_boundary_loss_bwd(fake, fake, fake, fake, 1, 100, 8, 0, fake, None) == -1
    assert L.da_boundary_loss_bwd(fake, fake, fake, fake, 1, 100, 65, 7, fake, None) == -3


def test_argument_errors_are_raised_before_the_device():
    from deepatlas_amd import ops, _native
    m = torch.zeros((1, 3, 5, 7), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.distance_transform_edt(m.float())
    with pytest.raises(ValueError):
        ops.distance_transform_edt(m[0])
    with pytest.raises(ValueError):
        ops.distance_transform_edt(m, spacing=(1, 1))
    with pytest.raises(ValueError):
        ops.distance_transform_edt(m, spacing=(1, -1, 1))
    long_row = torch.zeros(1, dtype=torch.uint8).expand(1, 1, 1, 4096)              # zero strides: nothing allocated
    with pytest.raises(ValueError, match='2\\^24'):
        ops.distance_transform_edt(long_row)
    with pytest.raises(ValueError, match='2\\^24'):
        ops.signed_distance_maps(long_row, 4)
    with pytest.raises(ValueError):
        ops.signed_distance_maps(m.float(), 4)
    with pytest.raises(ValueError):
        ops.signed_distance_maps(m, 4, classes=[4])
    with pytest.raises(ValueError):
        ops.signed_distance_maps(m, 1)
    z, phi = torch.zeros((1, 4, 3, 5, 7)), torch.zeros((1, 3, 3, 5, 7))
    with pytest.raises(ValueError):
        ops.BoundaryLossFn.apply(z, phi[:, :2], None)
    with pytest.raises(ValueError):
        ops.BoundaryLossFn.apply(z.double(), phi, None)
    # ... and a well-formed call on a host tensor fails loudly: there is no CPU path
    with pytest.raises(_native.NativeError):
        ops.distance_transform_edt(m)
    with pytest.raises(_native.NativeError):
        ops.signed_distance_maps(m, 4)
    with pytest.raises(_native.NativeError):
        ops.BoundaryLossFn.apply(z, phi, None)


def test_lambda_boundary_config_parsing(monkeypatch):
    import train_seg
    from deepatlas_amd.models import segmentation as seg
    seen = []

    class Fake(object):
        def __init__(self, config):
            seen.append(config)

        def train(self):
            pass

        def test(self):
            pass
    monkeypatch.setattr(train_seg, 'SegmentationExperiment', Fake)
    train_seg.main([])
    train_seg.main(['--lambda-boundary', '0'])
    train_seg.main(['--lambda-boundary', '0.5'])
    assert 'lambda_boundary' not in seen[0] and seen[1]['lambda_boundary'] == 0.0 and seen[2]['lambda_boundary'] == 0.5
    name = seg.SegmentationExperiment.experiment_name
    assert name(seen[0]) == name(seen[1]) and 'boundary' not in name(seen[0])
    assert name(seen[2]) == name(seen[0]) + '_boundary0.5'
    assert seg.check_boundary_term(seen[0]) == (0.0, {}) and seg.check_boundary_term(seen[2]) == (0.5, {})
    cfg = dict(seen[2], boundary_settings={'classes': [1, 2], 'spacing': (1, 1, 2)})
    assert seg.check_boundary_term(cfg) == (0.5, {'classes': [1, 2], 'spacing': (1, 1, 2)})
    for bad in (dict(lambda_boundary=-1.0), dict(lambda_boundary=float('inf')), dict(lambda_boundary='1'), dict(lambda_boundary=True),
                dict(lambda_boundary=1.0, boundary_settings={'radius': 2}), dict(lambda_boundary=0.0, boundary_settings={'classes': [32]}),
                dict(lambda_boundary=1.0, boundary_settings={'spacing': (0, 1, 1)})):
        with pytest.raises(ValueError):
            seg.check_boundary_term(dict(seen[0], **bad))
