"""CPU: the inverse-consistency penalty, everything that needs no GPU -- the loss is registered in its own group (the three existing lists stay
as they are), the C entries are declared, built and refuse bad arguments, the weight and the report switch reach the config and leave the
defaults exactly as they were, a CPU tensor is refused; and the cases of tests/invcons_cases.py are what test_gpu_invcons.py assumes: both
fields off the lattice, float32 distances as recorded, the lattice / translation / non-finite cases what they claim, the descent true of the
float64 reference."""
import argparse
import math
import os

import pytest
import torch

import invcons_cases as ic
import warp_cases as wc
from deepatlas_amd import ops
from deepatlas_amd.lib.loss import InverseConsistencyLoss
from deepatlas_amd.models.joint import make_ic_penalty

assert ops.InverseConsistencyFn and InverseConsistencyLoss and make_ic_penalty          # this file is about the feature: without it, it does not import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ns(**kw):
    base = dict(device='0', debug=False, num_samples=4, num_epochs=3, lr=1e-3, test_only=False, data_root='./data', log_root='./logs',
                shape=[16, 16, 32])
    base.update(kw)
    return argparse.Namespace(**base)


# ---- registry, validation, C ABI -------------------------------------------------------------------------------------------------------
def test_inverse_consistency_is_registered_in_its_own_group():
    from deepatlas_amd.lib import loss as L
    assert L.get_loss_function('inverse_consistency') is L.InverseConsistencyLoss and L.loss_dict['inverse_consistency'] is L.InverseConsistencyLoss
    assert L.get_field_pair_losses() == ['inverse_consistency'] and list(L.FIELD_PAIR_LOSSES) == ['inverse_consistency']
    assert L.get_regulariser_losses() == ['jacobian']
    assert L.get_extension_losses() == ['mi']
    # the reference's registry, in its order (lib/loss.py:739-761)
    assert L.get_available_losses() == ['ncc', 'lncc', 'mse', 'gradient', 'bendingEnergy', 'dice', 'L2', 'focal', 'cross_entropy', 'soft_cross_entropy']
    m = L.get_loss_function('inverse_consistency')()
    assert m.symmetric is True and not list(m.parameters())
    assert L.InverseConsistencyLoss(symmetric=False).symmetric is False


def test_op_refuses_bad_shapes_and_cpu_tensors():
    from deepatlas_amd import _native, ops
    from deepatlas_amd.lib import evalMetrics
    from deepatlas_amd.lib.loss import InverseConsistencyLoss
    good = torch.zeros(1, 3, 2, 3, 4)
    for bad in (torch.zeros(1, 2, 2, 3, 4), torch.zeros(3, 2, 3, 4), torch.zeros(1, 3, 2, 3, 4, 1), torch.zeros(2, 3, 2, 3, 4), torch.zeros(1, 3, 2, 3, 5)):
        for a, b in ((good, bad), (bad, good)):
            with pytest.raises(ValueError):
                ops.InverseConsistencyFn.apply(a, b)
            with pytest.raises(ValueError):
                ops.inverse_consistency_stats(a, b)
    with pytest.raises(_native.NativeError):          # valid arguments, CPU tensors: there is no CPU route
        ops.InverseConsistencyFn.apply(good, good)
    with pytest.raises(_native.NativeError):
        ops.inverse_consistency_stats(good, good)
    with pytest.raises(_native.NativeError):
        evalMetrics.inverse_consistency(good, good)
    for sym in (True, False):
        with pytest.raises(_native.NativeError):
            InverseConsistencyLoss(symmetric=sym)(good, good)


def test_entries_are_declared_and_built():
    import __graft_entry__ as ge
    assert 'invcons.hip' in ge.HIP_SOURCES
    ge.build()
    from deepatlas_amd import _native
    L = _native.lib()
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    for name in ('da_invcons_ws_bytes', 'da_invcons_fwd', 'da_invcons_bwd'):
        assert name + '(' in header, name
        assert name in _native.SIGNATURES and hasattr(L, name), name
    blob = open(ge.LIB, 'rb').read()
    for kernel in (b'invcons_fwd_kernel', b'invcons_finalize_kernel', b'invcons_bwd_kernel', b'invcons_scatter_kernel'):
        assert kernel in blob, kernel


def test_c_abi_rejects_bad_arguments_before_touching_the_device():
    from ctypes import c_void_p
    from deepatlas_amd import _native
    L = _native.lib()
    fake = c_void_p(0x1000)          # never dereferenced on the host
    BAD, SMALL, UNSUPPORTED = -1, -2, -3
    ok = (2, 8, 9, 10)
    need = L.da_invcons_ws_bytes(*ok)
    assert need >= 2 * 2048 * 4 * 8                                  # four doubles per partial row
    det_need = L.da_warp_bwd_dsrc_det_ws_bytes(*ok, 3)
    fwd, bwd = L.da_invcons_fwd, L.da_invcons_bwd
    for dims in ((0, 8, 9, 10), (-1, 8, 9, 10), (65536, 8, 9, 10), (2, 1, 9, 10), (2, 8, 1, 10), (2, 8, 9, 1), (2, 0, 9, 10)):      # N <= 0, an extent < 2
        assert fwd(fake, fake, *dims, fake, fake, fake, fake, 1 << 30, None) == BAD, dims
        for det in (0, 1):
            assert bwd(fake, fake, fake, fake, fake, fake, *dims, det, fake, 1 << 30, None) == BAD, dims
    assert fwd(None, fake, *ok, fake, None, None, fake, need, None) == BAD
    assert fwd(fake, None, *ok, fake, None, None, fake, need, None) == BAD
    assert fwd(fake, fake, *ok, None, None, None, fake, need, None) == BAD                # null loss
    assert fwd(fake, fake, *ok, fake, None, None, None, need, None) == BAD                # null workspace
    assert fwd(fake, fake, *ok, fake, None, None, fake, need - 1, None) == SMALL
    for k in range(4):                                                                    # a null input of the backward
        args = [fake] * 4
        args[k] = None
        assert bwd(*args, fake, fake, *ok, 0, None, 0, None) == BAD
    assert bwd(fake, fake, fake, fake, fake, fake, *ok, 1, None, 1 << 30, None) == BAD    # the deterministic route needs its workspace
    assert bwd(fake, fake, fake, fake, fake, fake, *ok, 1, fake, det_need - 1, None) == SMALL
    assert bwd(fake, fake, fake, fake, None, None, *ok, 0, None, 0, None) == 0            # no gradient wanted: nothing to do
    big = (1, 1024, 1024, 512)                                       # 2^29 voxels: 32-bit element offsets inside a sample would overflow
    assert fwd(fake, fake, *big, fake, None, None, fake, 1 << 30, None) == UNSUPPORTED
    assert bwd(fake, fake, fake, fake, fake, fake, *big, 0, None, 0, None) == UNSUPPORTED


def test_weight_and_report_reach_the_config_and_the_defaults_stay():
    import train_reg
    import train_joint
    from deepatlas_amd.models.registration import RegistrationExperiment, check_ic_penalty
    from deepatlas_amd.models.joint import make_ic_penalty, RegistrationStep
    from deepatlas_amd.lib.loss import InverseConsistencyLoss
    # a Namespace without the new attributes (what every earlier caller builds): penalty and report off, the name and the config as they were
    c0 = train_reg.build_config(_ns())
    assert 'lambda_ic' not in c0 and 'report_ic' not in c0
    assert check_ic_penalty(c0) == (0.0, False)
    name0 = RegistrationExperiment.experiment_name(c0)
    assert '_ic' not in name0
    c1 = train_reg.build_config(_ns(lambda_ic=0.0, report_ic=False))
    assert c1 == c0 and RegistrationExperiment.experiment_name(c1) == name0
    c2 = train_reg.build_config(_ns(lambda_ic=2.5, report_ic=False))
    assert c2['lambda_ic'] == 2.5 and 'report_ic' not in c2 and check_ic_penalty(c2) == (2.5, True)       # the report follows the penalty
    assert RegistrationExperiment.experiment_name(c2) == name0 + '_ic2.5'
    assert RegistrationExperiment.experiment_name(dict(c2, lambda_jac=0.5)) == name0 + '_jac0.5_ic2.5'
    c3 = train_reg.build_config(_ns(report_ic=True))
    assert 'lambda_ic' not in c3 and c3['report_ic'] is True and check_ic_penalty(c3) == (0.0, True)
    assert RegistrationExperiment.experiment_name(c3) == name0
    assert check_ic_penalty(dict(c2, report_ic=False)) == (2.5, False)
    for bad in (-1.0, float('inf'), float('nan'), float('-inf')):
        with pytest.raises(ValueError):
            check_ic_penalty(dict(c0, lambda_ic=bad))
        with pytest.raises(ValueError):
            RegistrationExperiment(dict(c0, lambda_ic=bad))
        with pytest.raises(ValueError):
            make_ic_penalty(bad)
        with pytest.raises(ValueError):
            RegistrationStep(None, None, lam_ic=bad)
    exp = RegistrationExperiment(dict(c2))
    assert (exp.lambda_ic, exp.report_ic) == (2.5, True)
    exp = RegistrationExperiment(dict(c0))
    assert (exp.lambda_ic, exp.report_ic) == (0.0, False)
    # the flags belong to train_reg.py alone: the joint experiment has no inverse-consistency term
    parser = train_reg.add_inverse_consistency_arguments(train_reg.add_common_arguments(argparse.ArgumentParser()))
    a = parser.parse_args([])
    assert (a.lambda_ic, a.report_ic) == (0.0, False)
    a = parser.parse_args(['--lambda-ic', '1', '--report-ic'])
    assert (a.lambda_ic, a.report_ic) == (1.0, True)
    with pytest.raises(SystemExit):
        train_reg.add_common_arguments(argparse.ArgumentParser()).parse_args(['--lambda-ic', '1'])
    cj = train_joint.build_config(_ns())
    assert 'lambda_ic' not in cj and 'report_ic' not in cj
    # the step: no module without a weight
    assert make_ic_penalty() == (0.0, None) and make_ic_penalty(0.0) == (0.0, None) and make_ic_penalty(None) == (0.0, None)
    lam, mod = make_ic_penalty(0.5)
    assert lam == 0.5 and isinstance(mod, InverseConsistencyLoss) and mod.symmetric
    step = RegistrationStep(None, None)
    assert step.ic is None and step.lam_ic == 0.0
    assert isinstance(RegistrationStep(None, None, lam_ic=1.0).ic, InverseConsistencyLoss)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def test_cases_are_the_listed_ones():
    want = [((2, 2, 2), 1), ((2, 3, 5), 2), ((5, 2, 3), 1), ((7, 9, 66), 1), ((5, 7, 29), 1), ((17, 30, 22), 3), ((33, 47, 61), 2), ((80, 96, 80), 1)]
    assert [c[:2] for c in ic.CASES.values()] == want
    assert ic.AMPS == (0.3, 2.0, 8.0) and len(ic.COMBOS) == 24 and set(ic.FP32_DISTANCE) == set(ic.COMBOS)
    assert 80 * 96 * 80 > 2048 * 256                                  # the grid-stride loops of the 2048 x 256 launches run more than once
    assert (5 * 7 * 29 + 255) // 256 == 4 and (17 * 30 * 22 + 255) // 256 == 44 and (33 * 47 * 61 + 255) // 256 == 370      # plain loop; 40; 368
    assert (ic.FACTOR, ic.LOSS_FLOOR, ic.POINT_FLOOR) == (4.0, 5e-7, 2e-6)


@pytest.mark.parametrize('name,amp', ic.COMBOS, ids=ic.COMBO_IDS)
def test_case_is_admissible(name, amp):
    shape, n, why = ic.CASES[name]
    u_a, u_b = ic.fields(name, amp)
    for u in (u_a, u_b):
        assert u.dtype == torch.float32 and tuple(u.shape) == (n, 3) + tuple(shape) and bool(torch.isfinite(u).all()) and why
        # the conditioning rule: no sample coordinate within DELTA of an integer (0 and size - 1 included), in either direction
        assert wc.lattice_distance(u, tuple(shape)) >= wc.DELTA, (name, amp)
    ab, sym = ic.reference(name, amp)
    V = shape[0] * shape[1] * shape[2]
    outside = float(ab['stats'][:, 3].sum()) / (n * V)
    print('%s amp %g: L = %.4g, L_sym = %.4g, %.1f %% of the samples outside' % (name, amp, ab['loss'], sym['loss'], 100 * outside))
    assert ab['loss'] > 0.0 and sym['loss'] > 0.0
    assert abs(float(ab['stats'][:, 0].sum()) / (n * V) - ab['loss']) <= 1e-12 * ab['loss']
    if amp == 8.0 and V <= 30:
        assert outside > 0.5                                         # most samples of the small shapes leave the volume


@pytest.mark.parametrize('name,amp', ic.COMBOS, ids=ic.COMBO_IDS)
def test_float32_distance_is_as_recorded(name, amp):
    """The float32 torch evaluation against the float64 reference: re-measured here, it must itself fit the bounds the kernels are given
    (4 x the recorded distance, or the floor) -- a recorded figure that were too small would fail this before it fails the kernels --
    and the recorded distance must be within 4 x the re-measured one wherever it can set a bound."""
    one, sym = ic.measure_fp32(name, amp)
    rec_one, rec_sym = ic.FP32_DISTANCE[(name, amp)]
    print('%s amp %g: float32 one way %s symmetric %s' % (name, amp, ' '.join('%.2e' % v for v in one), ' '.join('%.2e' % v for v in sym)))
    for keys, got, rec, symmetric in ((ic.ONE_WAY, one, rec_one, False), (ic.SYMMETRIC, sym, rec_sym, True)):
        b = ic.bounds(name, amp, symmetric)
        for k, g, r in zip(keys, got, rec):
            assert g <= b[k], (k, g, b[k])
            # ... and the other way round: a recorded figure far too large would widen the kernels' bound unnoticed.  Where 4 x it stays below
            # the floor it sets no bound.
            assert r <= max(ic.FACTOR * g, ic.FLOOR[k] / ic.FACTOR), (k, r, g)
            assert r <= 2e-5, (k, r)                                 # nothing ill-conditioned: the suite's ceiling for a warp gradient is 1e-4


def test_zero_fields_are_exactly_consistent_in_the_reference():
    u_a, u_b = ic.lattice_fields('zero')
    r = ic.evaluate(u_a, u_b, torch.float64)
    assert r['loss'] == 0.0 and not bool(r['stats'].any()) and not bool(r['resid'].any()) and not bool(r['d_a'].any()) and not bool(r['d_b'].any())


def test_lattice_case_samples_the_lattice():
    u_a, u_b = ic.lattice_fields('ua0')
    assert not bool(u_a.any()) and wc.lattice_distance(u_a, ic.LATTICE_VOL) == 0.0
    r = ic.evaluate(u_a, u_b, torch.float64)
    assert float((r['resid'] - u_b.double()).abs().max()) <= 1e-12 and not bool(r['stats'][:, 3].any())      # T[u_b] = u_b at the lattice
    left, right = ic.lattice_sides(u_a, u_b)
    assert float((left - right).abs().max()) > 1e-3 * float(left.abs().max())          # d u_a does jump there


def test_translation_pair_in_the_reference():
    u_a, u_b = ic.translation_fields()
    D, H, W = ic.TRANSLATION_VOL
    cx = wc.voxel_coords(u_a, ic.TRANSLATION_VOL)[:, 0]
    assert float(((cx - cx.round()).abs() - 0.5).abs().max()) < 1e-6          # half-way between two columns: nowhere near a jump along x
    r = ic.evaluate(u_a, u_b, torch.float64)
    s = ic.scales(ic.TRANSLATION_VOL, torch.float64)
    e = (r['resid'] * s).abs().amax(1)                                # N x D x H x W, voxels
    assert float(e[..., :W - 2].max()) <= 1e-12 and float(e[..., W - 2:].min()) >= 0.7
    assert r['stats'][:, 3].tolist() == [2.0 * D * H] * ic.TRANSLATION_N


@pytest.mark.parametrize('value', ic.NONFINITE_VALUES)
def test_nonfinite_fields_hold_one_bad_voxel(value):
    u_a, u_b = ic.nonfinite_fields(value)
    bad = wc.bad_voxels(u_a, (2, 3, 5))
    assert int(bad.sum()) == 1 and bool(torch.isfinite(u_b).all())
    assert int((~torch.isfinite(u_a)).sum()) == (1 if math.isnan(value) else 0)


def test_descent_makes_the_float64_reference_consistent():
    """What test_gpu_invcons.py asks of the device, with the margin it is given: in float64 L_sym ends below a QUARTER of DESCENT_RATIO x the
    initial loss, at the figures recorded in invcons_cases.DESCENT_MEASURED."""
    a, b = ic.descent_start()
    losses = ic.descent(ic.sym_loss, a.double(), b.double())
    print('L_sym %.4g -> %.4g (ratio %.4f)' % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert len(losses) == ic.DESCENT_STEPS + 1
    assert losses[-1] < ic.DESCENT_RATIO / 4 * losses[0]
    assert abs(losses[0] - ic.DESCENT_MEASURED[0]) < 0.01 * losses[0] and abs(losses[-1] - ic.DESCENT_MEASURED[1]) < 0.05 * losses[-1]
