"""CPU: the Jacobian folding penalty, everything that needs no GPU -- the loss is registered as a regulariser (the two existing lists stay as
they are), arguments are validated before a device is touched, the three C entries are declared, built and refuse bad arguments, the weight
and the settings reach the configs and leave the defaults exactly as they were; and the cases of tests/jacpen_cases.py are what
test_gpu_jacpen.py assumes: guard band empty, folds present, float32 distances as recorded, the reference's determinant that of
regeval_cases.jacobian_np, the descent true of the float64 reference."""
import argparse
import os

import numpy as np
import pytest
import torch

import jacpen_cases as jc
import regeval_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ns(**kw):
    base = dict(device='0', debug=False, num_samples=4, num_epochs=3, lr=1e-3, test_only=False, data_root='./data', log_root='./logs',
                shape=[16, 16, 32])
    base.update(kw)
    return argparse.Namespace(**base)


# ---- registry, validation, C ABI -------------------------------------------------------------------------------------------------------
def test_jacobian_penalty_is_registered_as_a_regulariser():
    from deepatlas_amd.lib import loss as L
    assert L.get_loss_function('jacobian') is L.JacobianFoldingLoss and L.loss_dict['jacobian'] is L.JacobianFoldingLoss
    assert L.get_regulariser_losses() == ['jacobian']
    assert L.get_extension_losses() == ['mi']
    # the reference's registry, in its order (lib/loss.py:739-761)
    assert L.get_available_losses() == ['ncc', 'lncc', 'mse', 'gradient', 'bendingEnergy', 'dice', 'L2', 'focal', 'cross_entropy', 'soft_cross_entropy']
    m = L.get_loss_function('jacobian')()
    assert (m.eps, m.power) == (0.0, 1) and not list(m.parameters())
    m = L.JacobianFoldingLoss(eps=0.25, power=2)
    assert (m.eps, m.power) == (0.25, 2)
    for bad in (dict(power=0), dict(power=3), dict(power=1.5), dict(power=None), dict(power=True), dict(eps=-0.01), dict(eps=1.01),
                dict(eps=float('nan')), dict(eps=float('inf'))):
        with pytest.raises(ValueError):
            L.JacobianFoldingLoss(**bad)


def test_op_validates_its_arguments_before_touching_a_device():
    from deepatlas_amd import _native, ops
    good = torch.zeros(1, 3, 2, 3, 4)
    for bad in (torch.zeros(1, 2, 2, 3, 4), torch.zeros(3, 2, 3, 4), torch.zeros(1, 3, 2, 3, 4, 1), torch.zeros(1, 1, 2, 3, 4), good.double()):
        with pytest.raises(ValueError):
            ops.JacobianPenaltyFn.apply(bad)
        with pytest.raises(ValueError):
            ops.jacobian_penalty_stats(bad)
    for eps, power in ((0.0, 0), (0.0, 3), (0.0, 1.5), (0.0, None), (-0.1, 1), (1.5, 1), (float('nan'), 1)):
        with pytest.raises(ValueError):
            ops.JacobianPenaltyFn.apply(good, eps, power)
    with pytest.raises(_native.NativeError):          # valid arguments, a CPU tensor: there is no CPU route
        ops.JacobianPenaltyFn.apply(good)
    from deepatlas_amd.lib.loss import JacobianFoldingLoss
    with pytest.raises(ValueError):
        JacobianFoldingLoss()(good[:, :2])


def test_entries_are_declared_and_built():
    import __graft_entry__ as ge
    assert 'jacpen.hip' in ge.HIP_SOURCES
    ge.build()
    from deepatlas_amd import _native
    L = _native.lib()
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    for name in ('da_jacdet_penalty_ws_bytes', 'da_jacdet_penalty_fwd', 'da_jacdet_penalty_bwd'):
        assert name + '(' in header, name
        assert name in _native.SIGNATURES and hasattr(L, name), name
    blob = open(ge.LIB, 'rb').read()
    for kernel in (b'jacdet_penalty_fwd_kernel', b'jacdet_penalty_finalize_kernel', b'jacdet_penalty_bwd_kernel'):
        assert kernel in blob, kernel


def test_c_abi_rejects_bad_arguments_before_touching_the_device():
    from ctypes import c_void_p
    from deepatlas_amd import _native
    L = _native.lib()
    fake = c_void_p(0x1000)          # never dereferenced on the host
    BAD, SMALL, UNSUPPORTED = -1, -2, -3
    need = L.da_jacdet_penalty_ws_bytes(2, 8, 9, 10)
    assert need >= 2 * 2048 * 2 * 8                                  # two doubles per partial row
    fwd, bwd = L.da_jacdet_penalty_fwd, L.da_jacdet_penalty_bwd
    ok = (2, 8, 9, 10)
    for dims, eps, power in (((0, 8, 9, 10), 0.0, 1), ((2, 0, 9, 10), 0.0, 1), ((2, 8, 0, 10), 0.0, 1), ((2, 8, 9, 0), 0.0, 1), ((65536, 8, 9, 10), 0.0, 1),
                             (ok, 0.0, 0), (ok, 0.0, 3), (ok, -0.01, 1), (ok, 1.01, 1), (ok, float('nan'), 1), (ok, float('inf'), 2)):
        assert fwd(fake, *dims, eps, power, fake, fake, fake, fake, 1 << 30, None) == BAD, (dims, eps, power)
        assert bwd(fake, fake, fake, fake, *dims, eps, power, None) == BAD, (dims, eps, power)
    assert fwd(None, *ok, 0.0, 1, fake, fake, fake, fake, need, None) == BAD
    assert fwd(fake, *ok, 0.0, 1, None, fake, fake, fake, need, None) == BAD              # null loss
    assert fwd(fake, *ok, 0.0, 1, fake, fake, None, fake, need, None) == BAD              # null det
    assert fwd(fake, *ok, 0.0, 1, fake, fake, fake, None, need, None) == BAD              # null workspace
    assert fwd(fake, *ok, 0.0, 1, fake, fake, fake, fake, need - 1, None) == SMALL
    for k in range(4):
        args = [fake] * 4
        args[k] = None
        assert bwd(*args, *ok, 0.0, 1, None) == BAD
    big = (1, 1024, 1024, 512)                                       # 2^29 voxels: 32-bit element offsets inside a sample would overflow
    assert fwd(fake, *big, 0.0, 1, fake, fake, fake, fake, 1 << 30, None) == UNSUPPORTED
    assert bwd(fake, fake, fake, fake, *big, 0.0, 1, None) == UNSUPPORTED


def test_weight_and_settings_reach_the_configs_and_the_defaults_stay():
    import train_reg
    import train_joint
    from deepatlas_amd.models.registration import RegistrationExperiment, check_jac_penalty
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    from deepatlas_amd.models.joint import make_jac_penalty
    from deepatlas_amd.lib.loss import JacobianFoldingLoss
    for mod, exp in ((train_reg, RegistrationExperiment), (train_joint, DeepAtlasExperiment)):
        # a Namespace without the new attributes (what every earlier caller builds): penalty off, the name as it was
        c0 = mod.build_config(_ns())
        assert c0['lambda_jac'] == 0.0 and c0['jac_settings'] == {} and 'jac_eps' not in c0 and 'jac_power' not in c0
        assert check_jac_penalty(c0) == (0.0, {})
        name0 = exp.experiment_name(c0)
        assert '_jac' not in name0
        bare = {k: v for k, v in c0.items() if k not in ('lambda_jac', 'jac_settings')}
        assert exp.experiment_name(bare) == name0 and check_jac_penalty(bare) == (0.0, {})
        c1 = mod.build_config(_ns(lambda_jac=0.0, jac_eps=None, jac_power=None))
        assert exp.experiment_name(c1) == name0 and c1['jac_settings'] == {}
        c2 = mod.build_config(_ns(lambda_jac=2.5, jac_eps=0.1, jac_power=2))
        assert c2['lambda_jac'] == 2.5 and c2['jac_settings'] == {'eps': 0.1, 'power': 2}
        assert check_jac_penalty(c2) == (2.5, {'eps': 0.1, 'power': 2})
        assert exp.experiment_name(c2) == name0 + '_jac2.5'
        for bad in (dict(lambda_jac=-1.0), dict(lambda_jac=float('inf')), dict(lambda_jac=float('nan')), dict(jac_settings={'eps': 2.0}),
                    dict(jac_settings={'power': 3}), dict(jac_settings={'margin': 0.1})):
            with pytest.raises(ValueError):
                check_jac_penalty(dict(c0, **bad))
            with pytest.raises(ValueError):
                exp(dict(c0, **bad))
    parser = train_reg.add_common_arguments(argparse.ArgumentParser())
    a = parser.parse_args([])
    assert (a.lambda_jac, a.jac_eps, a.jac_power) == (0.0, None, None)
    a = parser.parse_args(['--lambda-jac', '1', '--jac-eps', '0.2', '--jac-power', '2'])
    assert (a.lambda_jac, a.jac_eps, a.jac_power) == (1.0, 0.2, 2)
    with pytest.raises(SystemExit):
        parser.parse_args(['--jac-power', '3'])
    # the steps: no module without a weight
    assert make_jac_penalty() == (0.0, None) and make_jac_penalty(0.0, {'eps': 0.5}) == (0.0, None)
    lam, mod_ = make_jac_penalty(0.5, {'eps': 0.5, 'power': 2})
    assert lam == 0.5 and isinstance(mod_, JacobianFoldingLoss) and (mod_.eps, mod_.power) == (0.5, 2)
    with pytest.raises(ValueError):
        make_jac_penalty(-0.5)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def test_cases_are_the_listed_ones():
    want = [((2, 2, 2), 1, 0.5, 0.3), ((2, 3, 5), 2, 1.0, 0.3), ((5, 2, 3), 1, 1.0, 0.3), ((1, 4, 6), 1, 1.0, 0.3), ((7, 9, 66), 1, 1.5, 0.35),
            ((17, 30, 22), 3, 1.5, 0.35), ((33, 47, 61), 2, 1.5, 0.25), ((80, 96, 80), 1, 1.5, 0.3)]
    assert [c[:4] for c in jc.CASES.values()] == want
    assert jc.EPS_VALUES == (0.0, 0.25) and jc.POWERS == (1, 2) and len(jc.COMBOS) == 32 and set(jc.FP32_DISTANCE) == set(jc.COMBOS)
    assert 80 * 96 * 80 > 2048 * 256                                  # the grid-stride loop of the 2048 x 256 launch runs more than once
    assert (jc.FACTOR, jc.LOSS_FLOOR, jc.GRAD_FLOOR) == (4.0, 5e-7, 1e-6)


@pytest.mark.parametrize('name', jc.IDS)
def test_case_is_admissible(name):
    shape, n, _, _, why = jc.CASES[name]
    f = jc.field(name)
    assert f.dtype == torch.float32 and tuple(f.shape) == (n, 3) + tuple(shape) and bool(torch.isfinite(f).all()) and why
    det = jc.det64(name)
    # the reference's determinant is regeval_cases.jacobian_np's (an axis of extent 1 doubled for numpy.gradient: every copy holds the same values)
    det_np = rc.jacobian_np(jc.numpy_field(name))
    for dim, extent in zip((1, 2, 3), shape):
        if extent == 1:
            det_np = np.take(det_np, [0], axis=dim)
    assert det_np.shape == det.shape and float(np.abs(det_np - det).max()) <= 1e-12 * max(1.0, float(np.abs(det).max()))
    # guard band: no voxel within the float32 evaluation's error of the threshold, at either eps; the allowed share is zero
    gb = jc.guard_bound(name)
    assert 0.0 < gb < 1e-3
    for eps in jc.EPS_VALUES:
        assert jc.in_guard_band(name, eps) == 0, (name, eps, gb)
        share = jc.folding_share(name, eps)
        print('%s eps %g: %.4f %% of the voxels active, guard band +-%.2e' % (name, eps, 100 * share, gb))
        assert 0.0 < share < 1.0
        for p in jc.POWERS:
            assert jc.reference(name, eps, p)[0] > 0.0
    assert 5e-4 <= jc.folding_share(name) <= 0.65


@pytest.mark.parametrize('name,eps,p', jc.COMBOS, ids=jc.COMBO_IDS)
def test_float32_distance_is_as_recorded(name, eps, p):
    """The float32 torch evaluation against the float64 reference: re-measured here, it must itself fit the bound the kernels are given
    (4 x the recorded distance, or the floor) -- a recorded figure that were too small would fail this before it fails the kernels --
    and the recorded distance must be within 4 x the re-measured one wherever it can set a bound."""
    loss_d, grad_d = jc.measure_fp32(name, eps, p)
    lb, gb = jc.bounds(name, eps, p)
    print('%s eps %g p %d: float32 loss %.2e gradient %.2e (recorded %s)' % (name, eps, p, loss_d, grad_d, jc.FP32_DISTANCE[(name, eps, p)]))
    assert loss_d <= lb and grad_d <= gb
    # ... and the other way round: a recorded figure far too large would widen the kernels' bound unnoticed.  Where 4 x it stays below the
    # floor it sets no bound, and a distance of a few 1e-9 is a chance cancellation that another host's float32 kernels need not repeat.
    rec_l, rec_g = jc.FP32_DISTANCE[(name, eps, p)]
    assert rec_l <= max(jc.FACTOR * loss_d, jc.LOSS_FLOOR / jc.FACTOR) and rec_g <= max(jc.FACTOR * grad_d, jc.GRAD_FLOOR / jc.FACTOR)
    assert jc.FP32_DISTANCE[(name, eps, p)][0] <= 5e-7 and jc.FP32_DISTANCE[(name, eps, p)][1] <= 1e-6        # a few ulp: nothing ill-conditioned


def test_identity_field_has_no_penalty_and_no_gradient_in_the_reference():
    z = torch.zeros(2, 3, 4, 5, 6)
    for eps in (0.0, 0.25):
        for p in jc.POWERS:
            loss, grad = jc.evaluate(z, eps, p, torch.float64)
            assert loss == 0.0 and not bool(grad.any())


def test_descent_removes_folds_in_the_float64_reference():
    """What test_gpu_jacpen.py asks of the device, with the margin it is given: in float64 the loss falls at every step and the folding
    count ends below a QUARTER of the first one (the device: below half)."""
    losses, folds = jc.descent_twin()
    print(['%.4e' % v for v in losses], folds)
    assert len(losses) == jc.DESCENT_STEPS + 1
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert folds[0] > 1000 and folds[-1] < folds[0] / 4
