"""csrc/fieldinv.hip on the GPU: ops.invert_field / ops.transport_points against the float64 definition of tests/invert_cases.py (inputs,
references and the derivation of every bound are there), the metrics built on them (lib/evalMetrics.py) and the report_tre probe of
RegistrationExperiment.  No test times a kernel."""
import argparse
import math
import re

import numpy as np
import pytest
import torch

import invert_cases as iv
import invcons_cases as ic
import warp_cases as wc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPE = (32, 32, 32)


def _ops():
    from deepatlas_amd import ops
    return ops


def _nodes(vol, n):
    """N x V x 3 float32 voxel coordinates (x, y, z) of the grid nodes, voxel order"""
    return iv._nodes(vol).reshape(3, -1).t().unsqueeze(0).expand(n, -1, -1).float().contiguous()


# ---- dense inverse -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('combo', iv.COMBOS, ids=iv.COMBO_IDS)
def test_dense_inverse_against_float64(combo):
    name, lip, kind = combo
    vol, n, _ = iv.CASES[name]
    V = vol[0] * vol[1] * vol[2]
    ref = iv.reference(*combo)
    v, stats, iters = _ops().invert_field(iv.field(*combo).to(DEV), max_iters=iv.MAX_ITERS, tol_vox=0.0, return_stats=True, return_iters=True)
    assert tuple(v.shape) == (n, 3) + vol and v.dtype == torch.float32 and tuple(stats.shape) == (n, 4) and tuple(iters.shape) == (n,) + vol
    b = iv.bound(*combo)
    d = iv.vox_distance(v, ref['v'])
    print('%s: %.2e voxel from float64 (bound %.2e)' % ('%s-lip%g-%s' % combo, d, b))
    assert d <= b
    got, want = stats.cpu(), iv.stats_of(ref, vol, 0.0)
    # the final update is the difference of two iterates, each within the bound of the float64 one
    assert bool((got[:, 0] <= want[:, 0] + 2 * b).all()), (got[:, 0], want[:, 0])
    it = iters.cpu().long()
    assert int(it.min()) >= 1 and int(it.max()) <= iv.MAX_ITERS
    assert torch.equal(got[:, 2], it.reshape(n, -1).sum(1).double())                   # (tol 0 stops early only on an update of exactly 0)
    assert bool((got[:, 1] >= 0).all()) and bool((got[:, 1] <= V).all())
    near = iv.near_face(ref['coords'], vol)
    assert bool(((got[:, 3] - want[:, 3]).abs() <= near).all()), (got[:, 3], want[:, 3], near)


@pytest.mark.parametrize('combo', iv.SMALL_COMBOS, ids=iv.SMALL_IDS)
@pytest.mark.parametrize('tol', iv.TOLS)
def test_early_exit(combo, tol):
    name, lip, kind = combo
    vol, n, _ = iv.CASES[name]
    v, stats, iters = _ops().invert_field(iv.field(*combo).to(DEV), max_iters=iv.MAX_ITERS, tol_vox=tol, return_stats=True, return_iters=True)
    d = iv.vox_distance(v, iv.reference(*combo)['v'])
    assert d <= iv.early_exit_bound(tol, lip) + iv.bound(*combo), d
    s = stats.cpu()
    assert bool((s[:, 1] == 0).all()) and bool((s[:, 0] <= tol).all())
    it = iters.cpu().long()
    masked = iv.masked_reference(name, lip, kind, tol)
    assert bool((it <= masked['iters'] + 1).all()) and int(it.min()) >= 1
    assert torch.equal(s[:, 2], it.reshape(n, -1).sum(1).double())
    assert int(it.max()) < iv.MAX_ITERS                                           # every voxel stops on its own


@pytest.mark.parametrize('name', ['2x2x2', '5x7x29', '17x30x22', '33x47x61'])
def test_one_update_is_the_negated_sample_at_the_identity(name):
    u = iv.field(name, 0.5)
    vol = iv.CASES[name][0]
    v, iters = _ops().invert_field(u.to(DEV), max_iters=1, tol_vox=0.0, return_iters=True)
    assert iv.vox_distance(v, iv.dense(u, torch.float64, 1)['v']) <= iv.bound(name, 0.5)
    assert bool((iters == 1).all())
    # -B[u](identity), not -u: the float32 identity is rounded, so the sample is not taken at the node exactly
    assert iv.vox_distance(v, -u.double()) <= iv.bound(name, 0.5)


def test_zero_field_and_whole_voxel_translation():
    ops = _ops()
    vol, n = (5, 7, 11), 2
    V = vol[0] * vol[1] * vol[2]
    v, stats, iters = ops.invert_field(torch.zeros((n, 3) + vol, device=DEV), max_iters=iv.MAX_ITERS, tol_vox=0.0, return_stats=True, return_iters=True)
    assert torch.equal(v, torch.zeros_like(v)) and not bool(torch.signbit(v).any())
    assert bool((iters == 1).all())
    assert torch.equal(stats.cpu(), torch.tensor([[0.0, 0.0, V, 0.0]] * n, dtype=torch.float64))
    shift = wc.build_field(dict(n=n, vol=vol, field='shift', shift=(1, -1, 2)))
    w, stats = ops.invert_field(shift.to(DEV), return_stats=True)
    assert iv.vox_distance(w, -shift.double()) <= iv.floor_vox(vol)
    assert bool((stats[:, 1] == 0).all())


@pytest.mark.parametrize('name', iv.RIGID_IDS)
def test_rigid_field_against_the_closed_form_inverse(name):
    u, _, _ = iv.rigid(name)
    v = _ops().invert_field(u.to(DEV), max_iters=iv.MAX_ITERS, tol_vox=0.0)
    d = iv.rigid_distance(v, name)
    print('%s rigid: %.2e voxel from the closed form (bound %.2e)' % (name, d, iv.rigid_bound(name)))
    assert d <= iv.rigid_bound(name)


def test_non_finite_voxels_poison_only_what_samples_them():
    ops = _ops()
    name = '17x30x22'
    vol, n, _ = iv.CASES[name]
    D, H, W = vol
    V = D * H * W
    clean = iv.field(name, 0.5)
    bad = clean.clone()
    flat = bad.reshape(n, 3, V)
    hit = []
    for i, (vox, val) in enumerate(zip((0, V // 3, V // 2, V - 1), wc.NONFINITE)):
        flat[i % n, :, vox] = torch.tensor(val)
        hit.append((i % n, vox))
    v_clean = ops.invert_field(clean.to(DEV)).cpu()
    v_bad, stats = ops.invert_field(bad.to(DEV), return_stats=True)
    v_bad, stats = v_bad.cpu(), stats.cpu()
    # every iterate x + v_k lies within max |u| voxels of x (v_k = -u somewhere) and its taps one voxel further
    reach = int(math.ceil(float((clean.double() * iv.scales(vol)).abs().max()))) + 2
    far = torch.ones((n, D, H, W), dtype=torch.bool)
    for s, vox in hit:
        d, h, w = vox // (H * W), (vox // W) % H, vox % W
        assert bool(torch.isnan(v_bad[s, :, d, h, w]).all()), (s, vox, v_bad[s, :, d, h, w])
        far[s, max(d - reach, 0):d + reach + 1, max(h - reach, 0):h + reach + 1, max(w - reach, 0):w + reach + 1] = False
    assert float(far.double().mean()) > 0.5
    sel = far.unsqueeze(1).expand_as(v_bad)
    assert torch.equal(v_bad[sel], v_clean[sel]) and bool(torch.isfinite(v_bad[sel]).all())
    for s in range(n):
        assert stats[s, 0] == float('inf') and stats[s, 1] >= sum(1 for t, _ in hit if t == s)


def test_repeats_are_bit_identical():
    ops = _ops()
    u = iv.field('33x47x61', 0.8).to(DEV)
    a = ops.invert_field(u, return_stats=True, return_iters=True)
    b = ops.invert_field(u, return_stats=True, return_iters=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(a[1][:, 2].min()) > u[0, 0].numel()                    # more than one update per voxel, fewer than max_iters each
    p = iv.points('17x30x22', 3, 1000).to(DEV)
    w = iv.point_field('17x30x22', 3).to(DEV)
    c = ops.transport_points(w, p, inverse=True, return_stats=True)
    d = ops.transport_points(w, p, inverse=True, return_stats=True)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


# ---- points ------------------------------------------------------------------------------------------------------------------------------
def point_bound(vol):
    """The dense floor (the float32 sample coordinate, amplified) plus the output's own two roundings, a product and a sum of magnitude below
    the largest extent, 2 x 2^-24 x extent voxels."""
    return iv.floor_vox(vol) + 2.0 ** -23 * max(vol)


@pytest.mark.parametrize('case', iv.POINT_CASES, ids=iv.POINT_IDS)
def test_points_forward_inverse_and_round_trip(case):
    ops = _ops()
    name, n, P = case
    vol = iv.CASES[name][0]
    u, p = iv.point_field(name, n), iv.points(name, n, P)
    b = point_bound(vol)
    ud, pd = u.to(DEV), p.to(DEV)
    fwd, fstats = ops.transport_points(ud, pd, return_stats=True)
    assert tuple(fwd.shape) == (n, P, 3) and fwd.dtype == torch.float32
    assert float((fwd.cpu().double() - iv.transport_ref(u, p, False)).abs().max()) <= b
    assert torch.equal(fstats[:, 1:3].cpu(), torch.tensor([[0.0, P]] * n, dtype=torch.float64))
    inv, stats = ops.transport_points(ud, pd, inverse=True, max_iters=iv.MAX_ITERS, tol_vox=0.0, return_stats=True)
    assert float((inv.cpu().double() - iv.transport_ref(u, p, True)).abs().max()) <= b
    assert bool((stats[:, 0] <= 2 * b).all())
    # x is within b of the exact solution, the forward map has a Lipschitz constant below 1 + LIP < 2, and the forward transport its own b
    back = ops.transport_points(ud, inv)
    assert float((back.cpu().double() - p.double()).abs().max()) <= 3 * b


@pytest.mark.parametrize('name,n', [('5x7x29', 1), ('17x30x22', 3)])
@pytest.mark.parametrize('tol', [0.0, 1e-3])
def test_inverse_transport_of_the_grid_nodes_is_the_dense_inverse_bit_for_bit(name, n, tol):
    ops = _ops()
    vol = iv.CASES[name][0]
    D, H, W = vol
    u = iv.point_field(name, n).to(DEV)
    nodes = _nodes(vol, n).to(DEV)
    v, vstats = ops.invert_field(u, max_iters=iv.MAX_ITERS, tol_vox=tol, return_stats=True)
    x, xstats = ops.transport_points(u, nodes, inverse=True, max_iters=iv.MAX_ITERS, tol_vox=tol, return_stats=True)
    s = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], dtype=torch.float32, device=DEV)
    vv = v.permute(0, 2, 3, 4, 1).reshape(n, -1, 3)
    want = nodes + s * vv                                               # a rounded product, then a rounded sum, as the kernel forms them
    assert torch.equal(x, want), 'largest difference %.3e voxel at %d of %d elements' % (float((x - want).abs().max()), int((x != want).sum()), x.numel())
    assert torch.equal(vstats, xstats)


def test_points_outside_the_volume_follow_the_border_rule():
    ops = _ops()
    name, n, P = '17x30x22', 3, 1000
    vol = iv.CASES[name][0]
    D, H, W = vol
    u = iv.point_field(name, n)
    p = iv.points(name, n, P, 3.0)
    hi = torch.tensor([W - 1.0, H - 1.0, D - 1.0])
    outside = ((p < 0) | (p > hi)).any(-1)
    assert 0.3 < float(outside.double().mean()) < 0.9
    fwd, stats = ops.transport_points(u.to(DEV), p.to(DEV), return_stats=True)
    b = point_bound(vol) + 2.0 ** -23 * 3
    assert float((fwd.cpu().double() - iv.transport_ref(u, p, False)).abs().max()) <= b
    assert torch.equal(stats[:, 3].cpu(), outside.sum(1).double())
    # the displacement of a point outside is that of the nearest point of the volume
    clamped = torch.minimum(torch.maximum(p, torch.zeros(3)), hi)
    at_face = ops.transport_points(u.to(DEV), clamped.to(DEV)).cpu()
    assert float(((fwd.cpu().double() - p.double()) - (at_face.double() - clamped.double())).abs().max()) <= 2 * b


def test_a_nan_point_gives_a_nan_row_only():
    ops = _ops()
    name, n, P = '5x7x29', 3, 65
    u = iv.point_field(name, n).to(DEV)
    p = iv.points(name, n, P)
    q = p.clone()
    q[1, 7, 2] = float('nan')
    q[2, 64, 0] = float('inf')
    for inverse in (False, True):
        good = ops.transport_points(u, p.to(DEV), inverse=inverse).cpu()
        got, stats = ops.transport_points(u, q.to(DEV), inverse=inverse, return_stats=True)
        got, stats = got.cpu(), stats.cpu()
        assert bool(torch.isnan(got[1, 7]).all()) and bool(torch.isnan(got[2, 64]).all())
        keep = torch.ones((n, P), dtype=torch.bool)
        keep[1, 7] = keep[2, 64] = False
        assert torch.equal(got[keep], good[keep]) and bool(torch.isfinite(got[keep]).all())
        assert math.isfinite(float(stats[0, 0])) and stats[0, 1] == 0
        assert stats[1, 0] == float('inf') and stats[2, 0] == float('inf') and stats[1, 1] >= 1 and stats[2, 1] >= 1


# ---- the composed field ----------------------------------------------------------------------------------------------------------------
def test_composition_with_the_inverse_is_the_identity():
    """v solves v(x) = -u(x + v(x)) at the nodes, so the residual of the pair (v, u), v(x) + u(x + v(x)), vanishes wherever the sample stays
    inside the volume (the composition pads with zeros, the inverse with the border value: the faces differ).  Interior mean: below 1 % of that
    of the pair (-u, u); over the whole volume only the rms is compared, which the faces dominate for both.
    The other order, u(x) + v(x + u(x)), samples the INTERPOLATED inverse between its nodes and is not small: on the float64 reference itself
    the interior mean is 0.0052 voxel against 0.0245 for -u on this field (the inverse of a piecewise trilinear map is not piecewise
    trilinear).  That order is held to the float64 reference's own value instead."""
    ops = _ops()
    combo = ('33x47x61', 0.5, 'smooth')
    vol = iv.CASES[combo[0]][0]
    u = iv.field(*combo)
    ud = u.to(DEV)
    v = ops.invert_field(ud, max_iters=iv.MAX_ITERS, tol_vox=0.0)
    s = iv.scales(vol)
    m = int(math.ceil(float((u.double() * s).abs().max()))) + 1

    def interior_mean(resid):
        e = (resid.detach().cpu().double() * s).pow(2).sum(1).sqrt()
        return float(e[:, m:-m, m:-m, m:-m].mean())
    with_inv = interior_mean(ops.inverse_consistency_forward(v, ud)[2])
    with_neg = interior_mean(ops.inverse_consistency_forward(-ud, ud)[2])
    print('interior mean residual: %.3e voxel with the inverse, %.3e with -u' % (with_inv, with_neg))
    assert with_inv < 0.01 * with_neg
    assert bool((ops.inverse_consistency_stats(v, ud)['rms_vox'] < ops.inverse_consistency_stats(-ud, ud)['rms_vox']).all())          # per sample
    other = interior_mean(ops.inverse_consistency_forward(ud, v)[2])
    want = interior_mean(ic.residual(u.double(), iv.reference(*combo)['v']))
    print('the other order: %.6e voxel, float64 reference %.6e' % (other, want))
    assert abs(other - want) <= 2 * iv.bound(*combo)


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------
def test_target_registration_error_against_numpy():
    from deepatlas_amd.lib import evalMetrics as metrics
    vol, n, P = (9, 10, 11), 2, 40
    t = (1.5, -2.0, 0.5)
    disp = wc.build_field(dict(n=n, vol=vol, field='shift', shift=t)).to(DEV)
    g = torch.Generator().manual_seed(5)
    f = 2.0 + torch.rand((n, P, 3), generator=g) * torch.tensor([6.0, 5.0, 4.0])
    m = f + torch.tensor(t) + 0.3 * torch.randn((n, P, 3), generator=g)
    f[0, 3, 1] = float('nan')
    m[1, 11, 0] = float('nan')
    skip = np.zeros((n, P), dtype=bool)
    skip[0, 3] = skip[1, 11] = True
    f64, m64 = f.double().numpy(), m.double().numpy()
    for spacing in ((1, 1, 1), (0.5, 2.0, 3.0)):
        res = metrics.target_registration_error(disp, f.to(DEV), m, spacing=spacing)
        sp = np.asarray(spacing, dtype=np.float64)
        for k in range(n):
            e = np.sqrt((((f64[k] + np.asarray(t) - m64[k]) * sp) ** 2).sum(-1))[~skip[k]]
            e0 = np.sqrt((((f64[k] - m64[k]) * sp) ** 2).sum(-1))[~skip[k]]
            for key, want in (('tre_mean', e.mean()), ('tre_std', e.std()), ('tre_max', e.max()), ('initial_mean', e0.mean()), ('initial_max', e0.max())):
                assert res[key].dtype == np.float64 and abs(res[key][k] - want) <= 1e-5 * max(sp), (key, res[key][k], want)
    one = metrics.target_registration_error(disp, f.to(DEV), m)
    two = metrics.target_registration_error(disp, f.to(DEV), m, spacing=(2, 2, 2))
    for key in one:
        assert np.allclose(two[key], 2 * one[key], rtol=1e-12, atol=0)


def test_invert_deformation_reports_the_statistics():
    from deepatlas_amd.lib import evalMetrics as metrics
    combo = ('17x30x22', 0.5, 'noisy')
    vol, n, _ = iv.CASES[combo[0]]
    inv, info = metrics.invert_deformation(iv.field(*combo).to(DEV), tol_vox=1e-3)
    assert iv.vox_distance(inv, iv.reference(*combo)['v']) <= iv.early_exit_bound(1e-3, 0.5) + iv.bound(*combo)
    masked = iv.masked_reference(combo[0], combo[1], combo[2], 1e-3)
    assert sorted(info) == ['max_update_vox', 'mean_iters', 'outside_frac', 'unconverged_frac']
    assert all(a.dtype == np.float64 and a.shape == (n,) for a in info.values())
    assert (info['unconverged_frac'] == 0).all() and (info['max_update_vox'] <= 1e-3).all()
    want = masked['iters'].reshape(n, -1).double().mean(1).numpy()
    assert (np.abs(info['mean_iters'] - want) <= 1.0).all() and (info['mean_iters'] > 1).all()
    assert (info['outside_frac'] > 0).all() and (info['outside_frac'] < 0.3).all()


def test_known_deformation_probe_pins_the_direction():
    from deepatlas_amd.lib import evalMetrics as metrics
    n, names = 2, ['first', 'second']
    g = torch.Generator().manual_seed(3)
    image = torch.nn.functional.interpolate(torch.rand((n, 1, 6, 6, 6), generator=g), size=SHAPE, mode='trilinear', align_corners=True).to(DEV)
    field = metrics.known_deformation_field(names, SHAPE, 3.0, 0.5, DEV)
    assert iv.lipschitz_bound(field.cpu()) <= 0.5 * (1 + 1e-5)
    assert float((field.cpu().double() * iv.scales(SHAPE)).pow(2).sum(1).sqrt().max()) <= 3.0 * (1 + 1e-5)
    assert torch.equal(field, metrics.known_deformation_field(names, SHAPE, 3.0, 0.5, DEV)) and not torch.equal(field[0], field[1])
    exact = iv.dense(field.cpu(), torch.float64, 64)['v'].float().to(DEV)                # the float64 inverse of the known field
    seen = []

    def exact_model(moving, fixed):
        seen.append((moving, fixed))
        return (exact,)
    res = metrics.known_deformation_tre(exact_model, image, names, amp_vox=3.0, n_points=1000)
    assert len(seen) == 1 and seen[0][1] is image
    assert torch.allclose(seen[0][0], _ops().WarpFn.apply(image, field)[0])
    assert sorted(res) == ['tre_initial_mean_vox', 'tre_max_vox', 'tre_mean_vox', 'truth_unconverged_frac']
    print('exact inverse: TRE mean %s max %s, initial %s' % (res['tre_mean_vox'], res['tre_max_vox'], res['tre_initial_mean_vox']))
    assert (res['tre_mean_vox'] <= 10 * iv.floor_vox(SHAPE)).all() and (res['truth_unconverged_frac'] == 0).all()
    assert (res['tre_initial_mean_vox'] > 0.3).all()
    zero = metrics.known_deformation_tre(lambda moving, fixed: (torch.zeros_like(field),), image, names, amp_vox=3.0, n_points=1000)
    assert (zero['tre_mean_vox'] == zero['tre_initial_mean_vox']).all() and (zero['tre_initial_mean_vox'] == res['tre_initial_mean_vox']).all()
    # the wrong direction, u = g itself, is worse than doing nothing
    wrong = metrics.known_deformation_tre(lambda moving, fixed: (field,), image, names, amp_vox=3.0, n_points=1000)
    assert (wrong['tre_mean_vox'] > 1.5 * zero['tre_mean_vox']).all()


# ---- experiment --------------------------------------------------------------------------------------------------------------------------
def _config(tmp_path, monkeypatch, extra):
    from torch.utils.data import DataLoader
    import train_reg
    from deepatlas_amd.lib.datasets import SyntheticRegDataset
    monkeypatch.chdir(tmp_path)
    ns = argparse.Namespace(device='0', debug=False, num_samples=3, num_epochs=1, lr=1e-3, test_only=False, data_root='./data', log_root='logs',
                            shape=list(SHAPE))
    cfg = train_reg.build_config(ns)
    cfg.update(extra)
    cfg['training_data_loader'] = DataLoader(SyntheticRegDataset(3, SHAPE, 32, seed=230), batch_size=1, shuffle=False)
    cfg['validation_data_loader'] = DataLoader(SyntheticRegDataset(2, SHAPE, 32, seed=1230), batch_size=1, shuffle=False)
    cfg.update(lr_mode='const', samples_per_epoch=2, print_batch_period=1)
    return cfg


def _experiment(tmp_path, monkeypatch, extra):
    from deepatlas_amd.models.registration import RegistrationExperiment
    cfg = _config(tmp_path, monkeypatch, extra)
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


def test_one_epoch_with_the_tre_report(tmp_path, monkeypatch, capsys):
    exp, losses = _experiment(tmp_path, monkeypatch, dict(report_tre={'amp_vox': 3.0, 'points': 200}))
    out = capsys.readouterr().out
    res = exp.last_validation
    assert len(losses) == 2 and all(math.isfinite(l) for l in losses)
    for k in ('tre_mean_vox', 'tre_max_vox', 'tre_initial_mean_vox'):
        assert k in res and math.isfinite(res[k]), k
    assert res['tre_initial_mean_vox'] > 0 and res['tre_max_vox'] >= res['tre_mean_vox'] > 0
    valid = [l for l in out.splitlines() if l.startswith('Validation:')]
    assert len(valid) == 1 and ', TRE %.2f (initial %.2f) vox' % (res['tre_mean_vox'], res['tre_initial_mean_vox']) in valid[0]
    assert 'tre' not in exp.exp_name.lower()


def test_without_the_key_nothing_changes(tmp_path, monkeypatch, capsys):
    from deepatlas_amd.models.registration import RegistrationExperiment
    plain, losses0 = _experiment(tmp_path, monkeypatch, {})
    assert 'report_tre' not in plain.config
    spelled, losses1 = _experiment(tmp_path, monkeypatch, dict(report_tre=None))
    out = capsys.readouterr().out
    assert list(plain.last_validation) == list(spelled.last_validation) and not any(k.startswith('tre') for k in plain.last_validation)
    assert len(losses0) == 2 and len(losses1) == 2 and losses0[0] == losses1[0]
    assert plain.exp_name == spelled.exp_name and 'TRE' not in out
    # the same lines in the same order, number for number in shape (the values of a later step depend on the order of float atomics)
    shape_of = lambda text: [re.sub(r'[0-9][0-9.e+:/-]*', '#', l) for l in text.splitlines()]
    lines = shape_of(out)
    assert len(lines) % 2 == 0 and lines[:len(lines) // 2] == lines[len(lines) // 2:]
    assert sum(l.startswith('Validation:') for l in lines) == 2
    with pytest.raises(ValueError):
        RegistrationExperiment(_config(tmp_path, monkeypatch, dict(report_tre={'amp_vox': 3.0}, affine_init='rigid')))
