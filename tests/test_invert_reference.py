"""CPU companion of test_gpu_invert.py: the conditions on the inputs of tests/invert_cases.py, the recorded float32 distances, the derivable
early-exit bound, the rigid field against its closed-form inverse, and what the feature adds that needs no GPU (host-side argument checks of
the two ops, the C-ABI table and header, the config checks)."""
import os
import re

import pytest
import torch

import invert_cases as iv
import warp_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('combo', iv.COMBOS, ids=iv.COMBO_IDS)
def test_inputs_meet_the_conditions_and_the_fp32_distance_fits(combo):
    name, lip, kind = combo
    u = iv.field(*combo)
    vol = iv.CASES[name][0]
    assert u.dtype == torch.float32 and tuple(u.shape) == (iv.CASES[name][1], 3) + vol
    b = iv.lipschitz_bound(u)
    assert lip * (1 - 1e-4) <= b <= lip, b
    ref = iv.reference(*combo)
    assert float(ref['last'].max()) <= 1e-9, 'the float64 iteration has not converged after %d updates: %.2e voxel' % (iv.MAX_ITERS, float(ref['last'].max()))
    assert int(ref['iters'].min()) >= 1
    if name in iv.EXACT_OUTSIDE:
        assert iv.face_distance(ref['coords'], vol) >= wc.DELTA and float(iv.near_face(ref['coords'], vol).sum()) == 0
    d = iv.measure_fp32(*combo)
    print('%s: float32 torch is %.2e voxel from float64 (recorded %.2e, kernel bound %.2e)' % ('%s-lip%g-%s' % combo, d, iv.FP32_DISTANCE[combo], iv.bound(*combo)))
    assert d <= 2.0 * iv.FP32_DISTANCE[combo] + 1e-9 and d <= iv.bound(*combo)
    assert iv.bound(*combo) >= iv.floor_vox(vol) > 0


@pytest.mark.parametrize('combo', iv.SMALL_COMBOS, ids=iv.SMALL_IDS)
@pytest.mark.parametrize('tol', iv.TOLS)
def test_early_exit_is_within_the_contraction_bound(combo, tol):
    name, lip, kind = combo
    m = iv.masked_reference(name, lip, kind, tol)
    d = iv.vox_distance(m['v'], iv.reference(*combo)['v'])
    assert d <= iv.early_exit_bound(tol, lip), (d, iv.early_exit_bound(tol, lip))
    assert float(m['last'].max()) <= tol and int(m['iters'].max()) < iv.MAX_ITERS


@pytest.mark.parametrize('name', iv.RIGID_IDS)
def test_rigid_field_against_the_closed_form_inverse(name):
    u, inv, mask = iv.rigid(name)
    assert iv.lipschitz_bound(u) < 0.5
    share = float(mask.double().mean())
    assert abs(share - iv.RIGID_FP32_DISTANCE[name][1]) < 2e-3 and share > 0.03
    d64 = iv.rigid_distance(iv.dense(u, torch.float64)['v'], name)
    d32 = iv.rigid_distance(iv.dense(u, torch.float32)['v'], name)
    print('%s rigid: float64 %.2e, float32 %.2e voxel from the closed form (recorded %.2e) on %.1f %% of the voxels' % (name, d64, d32, iv.RIGID_FP32_DISTANCE[name][0], 100 * share))
    assert d64 <= 1e-6 and d32 <= 2.0 * iv.RIGID_FP32_DISTANCE[name][0] and d32 <= iv.rigid_bound(name)


def test_point_transport_reference_agrees_with_the_dense_reference_at_the_nodes():
    """the float64 point iteration started at the grid nodes is the dense inverse: the two entry points have one definition"""
    name = '5x7x29'
    u = iv.field(name, 0.5)
    vol = iv.CASES[name][0]
    nodes = iv._nodes(vol).reshape(3, -1).t().unsqueeze(0).float()
    x = iv.transport_ref(u, nodes, True)
    v = ((x - nodes.double()).permute(0, 2, 1).reshape(1, 3, *vol)) / iv.scales(vol)
    assert iv.vox_distance(v, iv.reference(name, 0.5)['v']) <= 1e-12
    # forward(inverse(q)) = q
    q = iv.points(name, 1, 63, -2.0)
    back = iv.transport_ref(u, iv.transport_ref(u, q, True).float(), False)
    assert float((back - q.double()).abs().max()) <= 1e-5


# ---- what fails without the feature ------------------------------------------------------------------------------------------------------
def test_host_side_value_errors_of_the_two_ops():
    from deepatlas_amd import ops
    assert ops.FIELDINV_STATS == 4
    good = torch.zeros(1, 3, 4, 5, 6)
    pts = torch.zeros(1, 2, 3)
    for bad in (torch.zeros(1, 2, 4, 5, 6), torch.zeros(3, 4, 5, 6), good.double(), torch.zeros(1, 3, 1, 5, 6), torch.zeros(1, 3, 4, 5, 1)):
        with pytest.raises(ValueError):
            ops.invert_field(bad)
        with pytest.raises(ValueError):
            ops.transport_points(bad, pts)
    for mi in (0, 256, -1, 2.5):
        with pytest.raises(ValueError):
            ops.invert_field(good, max_iters=mi)
        with pytest.raises(ValueError):
            ops.transport_points(good, pts, inverse=True, max_iters=mi)
    for tol in (-1.0, float('nan')):
        with pytest.raises(ValueError):
            ops.invert_field(good, tol_vox=tol)
    for bad_pts in (torch.zeros(1, 2, 2), torch.zeros(2, 2, 3), torch.zeros(2, 3), torch.zeros(1, 0, 3), pts.double()):
        with pytest.raises(ValueError):
            ops.transport_points(good, bad_pts)


def test_entry_points_are_declared_in_the_table_and_the_header():
    from deepatlas_amd import _native
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    want = {'da_field_invert_ws_bytes': 4, 'da_field_invert': 13, 'da_field_points_ws_bytes': 2, 'da_field_transport_points': 15}
    for name, nargs in want.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs, name
        m = re.search(r'\b(size_t|int) %s\(([^;]*)\);' % name, header)
        assert m, name
        assert len(m.group(2).split(',')) == nargs, (name, m.group(2))
    import __graft_entry__ as g
    assert 'fieldinv.hip' in g.HIP_SOURCES


def test_report_tre_config_checks_and_names():
    import argparse
    import train_reg
    from deepatlas_amd.models import registration as reg
    assert reg.check_report_tre({}) is None and reg.check_report_tre({'report_tre': None}) is None
    assert reg.check_report_tre({'report_tre': {'amp_vox': 3}}) == {'amp_vox': 3.0, 'points': 1000}
    assert reg.check_report_tre({'report_tre': {'amp_vox': 2.5, 'points': 64}}) == {'amp_vox': 2.5, 'points': 64}
    for bad in (3.0, {}, {'points': 5}, {'amp_vox': 0}, {'amp_vox': float('inf')}, {'amp_vox': 3, 'points': 0}, {'amp_vox': 3, 'n': 1}):
        with pytest.raises(ValueError):
            reg.check_report_tre({'report_tre': bad})
    with pytest.raises(ValueError):
        reg.check_report_tre({'report_tre': {'amp_vox': 3}, 'affine_init': 'rigid'})
    assert reg.tre_text({}) == ''
    assert reg.tre_text({'tre_mean_vox': 1.234, 'tre_initial_mean_vox': 2.5}) == ', TRE 1.23 (initial 2.50) vox'
    parser = train_reg.add_tre_arguments(train_reg.add_affine_arguments(train_reg.add_inverse_consistency_arguments(train_reg.add_common_arguments(argparse.ArgumentParser()))))
    plain = train_reg.build_config(parser.parse_args([]))
    probed = train_reg.build_config(parser.parse_args(['--report-tre', '3']))
    assert 'report_tre' not in plain and probed['report_tre'] == {'amp_vox': 3.0}
    assert reg.RegistrationExperiment.experiment_name(plain) == reg.RegistrationExperiment.experiment_name(probed)
