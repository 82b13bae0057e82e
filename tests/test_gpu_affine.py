"""GPU: the affine pre-alignment kernels (affine.hip) against the float64 reference of tests/affine_cases.py, the optimiser of lib/affine.py
against a float64 twin and on a known misalignment, and the stage inside the registration experiment.  Every bound comes from
affine_cases.bound_of(): 4 x the float32 torch evaluation's own distance from float64 (relative max norm), or, where that distance is exactly
zero, 8 float32 ulps of the output's largest entry.

Measured on one MI355X (distance from float64 / its bound; the float32 torch evaluation's own distance for comparison):
    forward, 14 combinations          1.4e-08 - 4.3e-08     bounds 4.1e-07 - 5.5e-05     float32 torch 1.0e-07 - 1.4e-05
    d_theta, 14 combinations          1.1e-08 - 4.6e-08     bounds 2.9e-07 - 5.6e-05     float32 torch 7.3e-08 - 1.4e-05
    affine_disp (with / without u)    3.0e-08 - 5.6e-08     bounds 4.2e-07 - 3.4e-06
    WarpFn by the affine field        3.9e-07, 6.9e-07, 4.2e-07, 8.3e-06     bounds 2.4e-06, 7.2e-07, 7.9e-07, 1.5e-05
    three Adam iterations             7.1e-04 from the float64 twin (float32 twin 3.1e-03, bound 1.2e-02)
    recovery, NCC                     loss 0.363 -> 0.143, corner error 3.86 -> 1.38 voxels
    recovery, MI on an inverted image loss -0.433 -> -1.099, corner error 3.86 -> 0.15 voxels
    one epoch, misalign (10, 3)       identity Dice 0.191, affine Dice 0.792, composed Dice 0.548
"""
import argparse
import math

import pytest
import torch
import torch.nn.functional as F

import affine_cases as ac
from deepatlas_amd import ops as _ops

assert _ops.AffineWarpFn and _ops.affine_disp          # this file is about the feature: without it, it does not import

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def _device_eval(src, theta, g):
    """forward and d_theta on the device: dict(out, d_theta) as CPU tensors"""
    from deepatlas_amd import ops
    th = theta.to(dev()).requires_grad_(True)
    out = ops.AffineWarpFn.apply(src.to(dev()), th)
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == src.shape and th.grad.dtype == torch.float32 and th.grad.shape == theta.shape
    return dict(out=out.detach().cpu(), d_theta=th.grad.cpu())


# ---- the kernels against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kind', ac.COMBOS, ids=ac.COMBO_IDS)
def test_forward_and_d_theta_against_float64(name, kind):
    src, theta, g = ac.inputs(name, kind)
    ref, bound, fp32 = ac.reference(name, kind), ac.bounds(name, kind), ac.measure_fp32(name, kind)
    got = _device_eval(src, theta, g)
    d = {k: ac.rel_max(got[k], ref[k]) for k in ('out', 'd_theta')}
    print('%s %s: out %.2e (bound %.2e, float32 torch %.2e)  d_theta %.2e (bound %.2e, float32 torch %.2e)'
          % (name, kind, d['out'], bound['out'], fp32['out'], d['d_theta'], bound['d_theta'], fp32['d_theta']))
    for k in d:
        assert d[k] <= bound[k], '%s %s: %s is %.3e from float64 (bound %.1e)' % (name, kind, k, d[k], bound[k])


def test_identity_returns_the_source_bit_for_bit_and_a_zero_cotangent_exact_zeros():
    from deepatlas_amd.lib.affine import identity_theta
    for name in ('5x6x7', '4x9x13', '2x2x2', '96x96x64'):
        src, _, g = ac.inputs(name, ac.KINDS[0] if name != '96x96x64' else ac.BIG_KINDS[0])
        n = src.shape[0]
        got = _device_eval(src, identity_theta(n), torch.zeros_like(g))
        assert torch.equal(got['out'], src), name
        assert torch.equal(got['d_theta'], torch.zeros(n, 3, 4)), name
    # ... and a zero cotangent under a general theta
    src, theta, g = ac.inputs('6x5x9', 'affine')
    assert torch.equal(_device_eval(src, theta, torch.zeros_like(g))['d_theta'], torch.zeros(5, 3, 4))


def test_whole_voxel_translation_is_bit_exact_with_zeros_where_it_leaves():
    gen = torch.Generator().manual_seed(5)
    src = torch.randn((2, 3) + ac.TRANSLATION_VOL, generator=gen)
    got = _device_eval(src, ac.translation_theta(2), torch.zeros_like(src))['out']
    want = ac.shifted(src, ac.TRANSLATION_SHIFT)
    assert torch.equal(got, want)
    assert float((want == 0).double().mean()) > 0.3 and float((got == 0).double().mean()) == float((want == 0).double().mean())


def test_two_runs_are_bit_identical():
    for name, kind in (('6x5x9', 'rigid'), ('96x96x64', 'dyadic')):
        src, theta, g = ac.inputs(name, kind)
        a, b = _device_eval(src, theta, g), _device_eval(src, theta, g)
        assert torch.equal(a['out'], b['out']) and torch.equal(a['d_theta'], b['d_theta']), name


def test_nan_theta_poisons_its_own_sample_only():
    src, theta, g = ac.inputs('6x5x9', 'rigid')
    ref, bound = ac.reference('6x5x9', 'rigid'), ac.bounds('6x5x9', 'rigid')
    for value in (float('nan'), 1e12):
        th = theta.clone()
        th[2, 1, 3] = value
        got = _device_eval(src, th, g)
        assert torch.isnan(got['d_theta'][2]).all(), value
        keep = [0, 1, 3, 4]
        assert torch.isfinite(got['d_theta'][keep]).all() and torch.isfinite(got['out']).all()
        assert ac.rel_max(got['d_theta'][keep], ref['d_theta'][keep]) <= bound['d_theta']
        assert ac.rel_max(got['out'][keep], ref['out'][keep]) <= bound['out']
        assert torch.equal(got['out'][2], torch.zeros_like(got['out'][2]))          # a refused coordinate samples nothing


# ---- the displacement field of an affine map -------------------------------------------------------------------------------------------
def _compose_bound(theta, disp, vol):
    want = ac.compose_ref(theta, disp, vol)
    return want, ac.bound_of(ac.rel_max(ac.compose_ref(theta, disp, vol, torch.float32), want))


@pytest.mark.parametrize('name,kind', [('5x6x7', 'rigid'), ('4x9x13', 'affine'), ('2x2x2', 'outside'), ('6x5x9', 'outside'), ('96x96x64', 'dyadic')])
def test_affine_disp_against_its_formula(name, kind):
    from deepatlas_amd import ops
    vol, n = ac.CASES[name][0], ac.CASES[name][1]
    theta = ac.inputs(name, kind)[1]
    want, bound = _compose_bound(theta, None, vol)
    got = ops.affine_disp(theta.to(dev()), size=vol)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3) + vol
    d = ac.rel_max(got, want)
    print('%s %s: affine_disp %.2e from float64 (bound %.2e)' % (name, kind, d, bound))
    assert d <= bound
    # composed with a smooth field of 2 voxels
    u = ac.smooth_disp(vol, n, 2.0)
    want, bound = _compose_bound(theta, u, vol)
    d = ac.rel_max(ops.affine_disp(theta.to(dev()), u.to(dev())), want)
    print('%s %s: affine_disp with a field %.2e from float64 (bound %.2e)' % (name, kind, d, bound))
    assert d <= bound
    # the identity composed with a field is the field, bit for bit
    from deepatlas_amd.lib.affine import identity_theta
    assert torch.equal(ops.affine_disp(identity_theta(n).to(dev()), u.to(dev())).cpu(), u)
    assert torch.equal(ops.affine_disp(identity_theta(n).to(dev()), size=vol).cpu(), torch.zeros((n, 3) + vol))


@pytest.mark.parametrize('name,kind', [('5x6x7', 'rigid'), ('4x9x13', 'affine'), ('6x5x9', 'outside'), ('96x96x64', 'dyadic')])
def test_warp_by_the_affine_field_samples_where_the_affine_warp_does(name, kind):
    """WarpFn(src, affine_disp(theta)) against AffineWarpFn(src, theta).  The yardstick is the same pair in float32 torch on the CPU:
    grid_sample at identity + (theta x_n - x_n) against grid_sample at affine_grid(theta); the device pair may be 4 x as far apart."""
    from deepatlas_amd import ops
    src, theta, _ = ac.inputs(name, kind)
    vol = ac.CASES[name][0]
    u32 = ac.compose_ref(theta, None, vol, torch.float32)
    grid32 = (u32 + ac.identity_norm(vol, torch.float32)).permute(0, 2, 3, 4, 1)
    a32 = F.grid_sample(src, grid32, mode='bilinear', padding_mode='zeros', align_corners=True)
    b32 = ac.warp(src, theta)
    bound = ac.bound_of(ac.rel_max(a32, b32.double()))
    s = src.to(dev())
    via_field = ops.WarpFn.apply(s, ops.affine_disp(theta.to(dev()), size=vol))[0]
    direct = ops.AffineWarpFn.apply(s, theta.to(dev()))
    d = ac.rel_max(via_field, direct.cpu().double())
    print('%s %s: WarpFn by the affine field is %.2e from AffineWarpFn (bound %.2e)' % (name, kind, d, bound))
    assert d <= bound


# ---- bad arguments ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    from deepatlas_amd import _native, ops
    from deepatlas_amd.lib.affine import identity_theta
    src, th = torch.zeros(2, 1, 4, 5, 6, device=dev()), identity_theta(2).to(dev())
    calls = _native.n_calls
    for bad_src in (torch.zeros(2, 4, 5, 6, device=dev()), torch.zeros(2, 1, 1, 5, 6, device=dev()), torch.zeros(2, 1, 4, 1, 6, device=dev()),
                    torch.zeros(2, 1, 4, 5, 1, device=dev()), src.half(), src.double()):
        with pytest.raises(ValueError):
            ops.AffineWarpFn.apply(bad_src, th)
    for bad_th in (identity_theta(3).to(dev()), torch.zeros(2, 4, 4, device=dev()), torch.zeros(2, 12, device=dev()), th.half(), th.double()):
        with pytest.raises(ValueError):
            ops.AffineWarpFn.apply(src, bad_th)
        with pytest.raises(ValueError):
            ops.affine_disp(bad_th, torch.zeros(2, 3, 4, 5, 6, device=dev()))
    with pytest.raises(ValueError):
        ops.affine_disp(th)
    with pytest.raises(ValueError):
        ops.affine_disp(th, size=(4, 1, 6))
    with pytest.raises(ValueError):
        ops.affine_disp(th, torch.zeros(2, 3, 4, 5, 6, device=dev()).half())
    with pytest.raises(_native.NativeError):
        ops.AffineWarpFn.apply(src.cpu(), th)
    with pytest.raises(_native.NativeError):
        ops.AffineWarpFn.apply(src, th.cpu())
    with pytest.raises(_native.NativeError):
        ops.affine_disp(th.cpu(), size=(4, 5, 6))
    assert _native.n_calls == calls                                   # nothing reached the library
    # the gradient with respect to the source volume is out of scope, and says so
    s = src.clone().requires_grad_(True)
    out = ops.AffineWarpFn.apply(s, th.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        out.sum().backward()


# ---- the optimiser ---------------------------------------------------------------------------------------------------------------------
def _twin_pair():
    from deepatlas_amd.lib import affine as A
    fixed = ac.blob_volume(ac.TWIN_VOL, ac.TWIN_N, seed=1)
    known = A.rigid_theta(torch.tensor([[7.0, -6.0, 8.0], [-8.0, 6.0, 7.0]], dtype=torch.float64) * math.pi / 180,
                          torch.tensor([[2.5, -2.0, 1.5], [-1.5, 2.2, -2.4]], dtype=torch.float64), ac.TWIN_VOL)
    moving = ac.warp(fixed.double(), known).float()
    return moving, fixed


def test_three_adam_iterations_against_a_float64_twin():
    """affine_register(levels=(1,), iters=(3,)) against the same loop in torch on the CPU in float64: the parameters stay within 4 x the
    float32 twin's distance (max norm over the largest parameter).  Three steps: longer runs diverge chaotically."""
    from deepatlas_amd.lib import affine as A
    moving, fixed = _twin_pair()
    theta_fn = lambda p: A.theta_from_params(p, 'rigid', ac.TWIN_VOL)
    p64 = ac.twin_register(moving, fixed, theta_fn, torch.float64)
    p32 = ac.twin_register(moving, fixed, theta_fn, torch.float32)
    bound = ac.bound_of(ac.rel_max(p32, p64))
    theta, p = A.affine_register(moving.to(dev()), fixed.to(dev()), mode='rigid', sim='ncc', levels=(1,), iters=(ac.TWIN_STEPS,), lr=ac.TWIN_LR,
                                 return_params=True)
    torch.cuda.synchronize()
    d = ac.rel_max(p, p64)
    print('three Adam iterations: parameters %.2e from the float64 twin (float32 twin %.2e, bound %.2e); p = %s'
          % (d, ac.rel_max(p32, p64), bound, p.cpu().numpy().round(4).tolist()))
    # a condition on the inputs: every parameter moved the same way in all three steps (Adam steps by about lr each time), so that no gradient
    # sits at a sign change, where the last bits of the similarity decide the direction of a whole step
    assert float(p64.abs().min()) > 2.5 * ac.TWIN_LR
    assert d <= bound
    assert torch.equal(theta.cpu(), A.theta_from_params(p.cpu(), 'rigid', ac.TWIN_VOL))


RECOVERY_VOL = (24, 28, 32)
# A rigid map in general position: 8 degrees about an axis near (1, -1, 1) / sqrt(3) (Euler angles of 4.68 degrees each give a rotation of 8.0
# degrees) and 2 voxels along (1, -1, 1) (1.2, -1.2, 1.1: 2.02 voxels).  General position on purpose: the blocky volume of structured_labels
# steps by ONE intensity level from block to block along x, so a motion confined to the (x, y) planes (a rotation about z with a shift along x
# was tried first) changes a 32-bin joint histogram only within neighbouring bins, and mutual information is flat around the identity there;
# NCC recovers that case too, MI stays at the identity.
RECOVERY_ANGLES_DEG, RECOVERY_SHIFT_VOX = (4.68, -4.68, 4.68), (1.2, -1.2, 1.1)


def _recovery_pair(remap=None):
    from deepatlas_amd import ops
    from deepatlas_amd.lib import affine as A
    from deepatlas_amd.lib.datasets import structured_labels, SyntheticRegDataset
    lab = structured_labels(RECOVERY_VOL, 32, seed=0).float() / 31.0
    fixed = F.avg_pool3d(lab.view(1, 1, *RECOVERY_VOL), 3, 1, 1).to(dev())
    known = A.rigid_theta(torch.tensor([RECOVERY_ANGLES_DEG], dtype=torch.float64) * math.pi / 180, torch.tensor([RECOVERY_SHIFT_VOX], dtype=torch.float64),
                          RECOVERY_VOL).float().to(dev())
    moving = ops.AffineWarpFn.apply(fixed, known)
    if remap:
        moving = SyntheticRegDataset.remap_intensity(moving, remap)
    return moving.contiguous(), fixed, known


@pytest.mark.parametrize('sim,remap', [('ncc', None), ('mi', 'invert')])
def test_default_registration_recovers_a_known_rigid_misalignment(sim, remap):
    """moving(x) = fixed(known x), so the aligning map is known^-1.  Loose conditions, not measurements: the similarity ends below its value at
    the identity and the largest displacement error over the eight corners of the volume falls below half of what the identity leaves.
    Measured on one MI355X: see DESIGN.md 4.25."""
    from deepatlas_amd import ops
    from deepatlas_amd.lib import affine as A
    moving, fixed, known = _recovery_pair(remap)
    theta = A.affine_register(moving, fixed, mode='rigid', sim=sim)
    crit = A.make_sim(sim, None, dev())
    with torch.no_grad():
        before = float(crit(moving, fixed))
        after = float(crit(ops.AffineWarpFn.apply(moving, theta), fixed))
    want = A.invert_theta(known)
    err0 = float(A.corner_error_vox(A.identity_theta(1).to(dev()), want, RECOVERY_VOL))
    err = float(A.corner_error_vox(theta, want, RECOVERY_VOL))
    print('recovery (%s%s): similarity loss %.5f -> %.5f, corner error %.3f -> %.3f voxels' % (sim, ', inverted moving image' if remap else '', before, after, err0, err))
    assert tuple(theta.shape) == (1, 3, 4) and theta.dtype == torch.float32 and torch.isfinite(theta).all()
    assert after < before
    assert err < 0.5 * err0


# ---- the experiment --------------------------------------------------------------------------------------------------------------------
SHAPE = (32, 32, 32)


class _SameAnatomyPairs(torch.utils.data.Dataset):
    """Pairs of two noisy images of ONE synthetic volume (two sessions of one subject): the only geometric difference of a pair is the
    misalignment the experiment adds, so the Dice of the labels measures alignment.  (The pairs of SyntheticRegDataset join different
    volumes, whose label maps are disjoint by construction when aligned: their identity Dice says nothing about a global misalignment.)"""

    def __init__(self, n, seed):
        from deepatlas_amd.lib.datasets import SyntheticSegDataset
        self.a, self.b, self.n = SyntheticSegDataset(n, SHAPE, 32, seed), SyntheticSegDataset(n, SHAPE, 32, seed + 500), n
        self.seg = self.a

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        im, sm, _ = self.a[i]
        it, st_, _ = self.b[i]
        return im, it, sm, st_, True, 'session_a_%d_to_session_b_%d' % (i, i)


def _experiment(tmp_path, monkeypatch, extra, loaders):
    from torch.utils.data import DataLoader
    import train_reg
    from deepatlas_amd.models.registration import RegistrationExperiment
    monkeypatch.chdir(tmp_path)
    ns = argparse.Namespace(device='0', debug=False, num_samples=3, num_epochs=1, lr=1e-3, test_only=False, data_root='./data', log_root='logs',
                            shape=list(SHAPE))
    cfg = train_reg.build_config(ns)
    cfg.update(extra)
    train, valid = loaders()
    cfg['training_data_loader'] = DataLoader(train, batch_size=1, shuffle=False)
    cfg['validation_data_loader'] = DataLoader(valid, batch_size=1, shuffle=False)
    cfg.update(lr_mode='const', samples_per_epoch=2, print_batch_period=1)
    torch.manual_seed(11)
    exp = RegistrationExperiment(cfg)
    losses = []
    step = exp.train_step

    def recording(*a, **kw):
        r = step(*a, **kw)
        losses.append(float(r[0].item()))
        return r
    exp.train_step = recording
    exp.train()
    return exp, losses


def test_one_epoch_with_misalignment_and_rigid_pre_alignment(tmp_path, monkeypatch, capsys):
    exp, losses = _experiment(tmp_path, monkeypatch, dict(misalign=(10.0, 3.0), affine_init='rigid'),
                              lambda: (_SameAnatomyPairs(3, 230), _SameAnatomyPairs(2, 1230)))
    out = capsys.readouterr().out
    res = exp.last_validation
    assert exp.exp_name.endswith('_misalign10.0_3.0_affinerigid') and len(losses) == 2 and all(math.isfinite(l) for l in losses)
    assert 'affine_dice_avg' in res and len(res['affine_dice_per_class']) == 31
    print('one epoch at 32^3, misalign (10, 3): identity Dice %.4f, affine Dice %.4f, composed Dice %.4f'
          % (res['identity_dice_avg'], res['affine_dice_avg'], res['dice_avg']))
    assert math.isfinite(res['affine_dice_avg']) and math.isfinite(res['dice_avg']) and math.isfinite(res['nonpos_frac'])
    assert res['affine_dice_avg'] > res['identity_dice_avg']
    valid = [l for l in out.splitlines() if l.startswith('Validation:')]
    assert len(valid) == 1 and ', affine ' in valid[0]


def test_without_the_keys_nothing_changes(tmp_path, monkeypatch, capsys):
    """affine_init=None and misalign=None spelled out against a config that never mentions them: the same result keys, the same first loss,
    bit for bit, and no trace of the stage in the printed lines."""
    from deepatlas_amd.lib.datasets import SyntheticRegDataset
    loaders = lambda: (SyntheticRegDataset(3, SHAPE, 32, seed=230), SyntheticRegDataset(2, SHAPE, 32, seed=1230))
    plain, losses0 = _experiment(tmp_path, monkeypatch, {}, loaders)
    assert 'affine_init' not in plain.config and 'misalign' not in plain.config
    spelled, losses1 = _experiment(tmp_path, monkeypatch, dict(affine_init=None, misalign=None, affine_settings=None), loaders)
    out = capsys.readouterr().out
    assert list(plain.last_validation) == list(spelled.last_validation) and 'affine_dice_avg' not in plain.last_validation
    assert len(losses0) == 2 and len(losses1) == 2 and losses0[0] == losses1[0]
    assert plain.exp_name == spelled.exp_name and 'affine' not in out and 'misalign' not in out
