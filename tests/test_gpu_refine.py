"""GPU: the instance-refinement kernels (refine.hip) against the float64 reference of tests/refine_cases.py, refine_field against float64 and
float32 twins and on a known field, and the refinement inside the predictor, the experiment and predict_reg.py.  Every bound on a gradient, a
statistic or a trajectory comes from refine_cases (affine_cases.bound_of: 4 x the float32 torch evaluation's own distance from float64, floored at
8 float32 ulps); the update given a gradient is held to datapath_cases.adam_p_excess, the rule da_adam_step is held to.

Measured on one MI355X (distance from float64 / its bound):
    gradient, 5 cases                 7.3e-07 - 6.1e-06     bounds 3.8e-06 - 2.5e-05
    statistics                        at most 0.01 of their bounds (refine_cases.stats_bound); 1 - NCC off by 1.4e-09 - 6.2e-08
    five iterations, fused            5x6x7 7.6e-06 (4.3e-05), 1x9x40 4.6e-05 (9.4e-05), 12x20x36 1.0e-04 (2.4e-04), 16x16x24o 2.3e-04 (2.6e-03)
    their histories                   7.4e-08 - 1.7e-07     bounds 1.3e-07 - 3.4e-06
    composed against fused            5.4e-06, 1.0e-04, 2.8e-05 (the same bounds; 1x9x40 has no composed route: da_warp_fwd refuses an extent of 1)
    recovery                          1 - NCC 0.0607 -> 0.00012, endpoint error 0.900 -> 0.267 voxels (float64 twin 0.265); history 3.7e-04 (1.4e-03)
    one epoch at 16 x 16 x 32         Dice 0.0344 -> refined 0.0503, 1 - NCC 0.4147 -> 0.2412 (an untrained net, 5 iterations)
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datapath_cases as dc
import refine_cases as rc
from deepatlas_amd import ops as _ops
from deepatlas_amd.lib import refine as _refine

assert _ops.refine_ncc_grad and _refine.refine_field          # this file is about the feature: without it, it does not import

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device('cuda:0')


def _up(*ts):
    return [t.to(dev()) for t in ts]


def _moments(mv, fx, disp):
    """stats N x 8 of da_refine_moments as a CPU tensor"""
    from deepatlas_amd import ops
    a, b, N, D, H, W = ops.refine_args(mv, fx, disp)
    return ops.refine_moments(a, b, ops.ndhwc(disp)).cpu()


# ---- gradient, loss and statistics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(rc.CASES))
def test_gradient_loss_and_stats_against_float64(name):
    from deepatlas_amd import ops
    mv, fx, disp = _up(*rc.inputs(name))
    ref, gb, sb = rc.reference(name), rc.grad_bound(name), rc.stats_bound(name)
    loss, grad = ops.refine_ncc_grad(mv, fx, disp, lambda_sim=rc.LAMBDA_SIM)
    stats = _moments(mv, fx, disp)
    torch.cuda.synchronize()
    assert grad.shape == disp.shape and grad.dtype == torch.float32 and loss.shape == ()
    dg = rc.rel_max(grad, ref['grad'])
    ds = (stats[:, :6] - ref['stats'][:, :6]).abs()
    dl = abs(float(loss) - float(ref['sim']))
    print('%s: gradient %.2e (bound %.2e)  stats, worst share of their bounds %s  1 - NCC off by %.2e' % (name, dg, gb, ['%.2f' % float(x) for x in (ds / sb).max(0).values], dl))
    assert dg <= gb, '%s: gradient is %.3e from float64 (bound %.1e)' % (name, dg, gb)
    assert (ds <= sb).all(), '%s: stats are %s from float64 (bounds %s)' % (name, ds.tolist(), sb.tolist())
    assert dl <= float(sb[:, 5].max()) + 2.0 ** -23, (name, dl)               # the loss is 1 - mean ncc, stored in float32
    assert torch.equal(stats[:, 6], torch.full((mv.shape[0],), float(np.prod(rc.CASES[name][0])), dtype=torch.float64)) and float(stats[:, 7].abs().max()) == 0


@pytest.mark.parametrize('name', [n for n in rc.CASES if rc.CASES[n][0][0] > 1])
def test_stats_are_ncc_fwd_on_the_materialised_warp(name):
    """da_ncc_fwd on WarpFn's output (da_warp_fwd refuses an extent of 1: that case has the float64 reference alone), to its own rounding: the two
    sample the warp in float32 independently, so each may be refine_cases.stats_bound from the exact value"""
    from deepatlas_amd import ops
    mv, fx, disp = _up(*rc.inputs(name))
    got = _moments(mv, fx, disp)
    warped = ops.WarpFn.apply(mv, disp)[0]
    a, b = ops.ndhwc(warped), ops.ndhwc(fx)
    N, V = a.shape[0], a.numel() // a.shape[0]
    want = torch.empty((N, 8), dtype=torch.float64, device=dev())
    loss = torch.empty((1,), dtype=torch.float32, device=dev())
    wp, wn = ops._ws(ops.nat.lib().da_ncc_ws_bytes(N, V), a)
    ops.call('da_ncc_fwd', ops.ptr(a), ops.ptr(b), N, V, ops.ptr(loss), ops.ptr(want), wp, wn, ops.stream())
    want = want.cpu()
    sb = rc.stats_bound(name)
    d = (got[:, :6] - want[:, :6]).abs()
    assert (d <= 2 * sb).all(), '%s: stats are %s from da_ncc_fwd (bounds %s)' % (name, d.tolist(), (2 * sb).tolist())
    assert torch.equal(got[:, 6:], want[:, 6:])


@pytest.mark.parametrize('k', range(len(rc.LATTICE_SHIFTS)))
def test_lattice_fields_take_warp_bwd_side_of_the_derivative(k):
    from deepatlas_amd import ops
    mv, fx, disp = _up(*rc.lattice_inputs(k))
    _, grad = ops.refine_ncc_grad(mv, fx, disp, lambda_sim=rc.LAMBDA_SIM)
    u = disp.clone().requires_grad_(True)
    loss = ops.NCCFn.apply(ops.WarpFn.apply(mv, u)[0], fx)             # da_ncc_bwd's cotangent through WarpFn.backward
    loss.backward()
    want = rc.LAMBDA_SIM * u.grad
    d = rc.rel_max(grad, want.cpu().double())
    assert float(want.abs().max()) > 0
    assert d <= rc.lattice_bound(k), 'shift %r: %.3e from WarpFn.backward (bound %.1e)' % (rc.LATTICE_SHIFTS[k], d, rc.lattice_bound(k))


def test_non_finite_displacement_poisons_its_own_voxel_and_sample_only():
    from deepatlas_amd import ops
    mv, fx, disp = _up(*rc.inputs('12x20x36'))
    clean_stats = _moments(mv, fx, disp)
    _, clean = ops.refine_ncc_grad(mv, fx, disp)
    for bad in (float('nan'), float('inf')):
        d = disp.clone()
        d[1, 0, 3, 4, 5] = bad
        stats = _moments(mv, fx, d)
        loss, grad = ops.refine_ncc_grad(mv, fx, d)
        assert torch.isnan(stats[1, [0, 2, 3, 5]]).all() and torch.equal(stats[0], clean_stats[0]) and torch.equal(stats[2], clean_stats[2])
        assert torch.isnan(loss)                                             # the mean over the batch holds the poisoned sample
        assert torch.equal(grad[0], clean[0]) and torch.equal(grad[2], clean[2])
        assert torch.isnan(grad[1]).all()                                    # through the sample's statistics
        # the step kernel alone, given clean statistics: the voxel's own three elements and nothing else
        a, b, N, D, H, W = ops.refine_args(mv, fx, d)
        out = torch.empty_like(ops.ndhwc(d))
        state = ops.refine_host_state((0, 0, 0), rc.BETAS, rc.EPS, 1, 1.0, 1.0, 0).to(dev())
        ops.refine_step(a, b, ops.ndhwc(d), clean_stats.to(dev()), state, grad_out=out)
        isn = torch.isnan(ops.ncdhw(out))
        assert isn[1, :, 3, 4, 5].all() and int(isn.sum()) == 3
        assert torch.equal(ops.ncdhw(out)[~isn], clean[~isn])


def test_repeats_are_bit_identical():
    from deepatlas_amd import ops
    for name in ('12x20x36', '65x90x90'):
        mv, fx, disp = _up(*rc.inputs(name))
        l0, g0 = ops.refine_ncc_grad(mv, fx, disp)
        s0 = _moments(mv, fx, disp)
        for _ in range(3):
            l1, g1 = ops.refine_ncc_grad(mv, fx, disp)
            assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(s0, _moments(mv, fx, disp))


# ---- the update ------------------------------------------------------------------------------------------------------------------------
def _device_steps(name, steps, lr_vox=0.1, with_extra=True):
    """`steps` launches of da_refine_moments + da_refine_step(update = 1) with grad_out: (disp, m, v after each step, the gradients), CPU N x 3 x D x H x W"""
    from deepatlas_amd import ops
    mv, fx, disp = _up(*rc.inputs(name))
    a, b, N, D, H, W = ops.refine_args(mv, fx, disp)
    u = ops.ndhwc(disp).clone()
    m, v, g = torch.zeros_like(u), torch.zeros_like(u), torch.empty_like(u)
    gen = torch.Generator().manual_seed(5)
    extra = (torch.randn(u.shape, generator=gen) * 1e-6).to(dev()) if with_extra else None
    lr3, gs = ops.refine_lr3(lr_vox, (D, H, W)), float(D * H * W)
    hist = torch.full((steps,), -1.0, device=dev())
    path, grads, free = [], [], []
    for k in range(steps):
        stats = ops.refine_moments(a, b, u)
        ops.refine_step(a, b, u, stats, ops.refine_host_state((0, 0, 0), rc.BETAS, rc.EPS, 1, 1.0, rc.LAMBDA_SIM, 0).to(dev()), g_extra=extra, grad_out=g)
        free.append(ops.ncdhw(g).cpu().clone())
        state = ops.refine_host_state(lr3, rc.BETAS, rc.EPS, k + 1, gs, rc.LAMBDA_SIM, k).to(dev())
        ops.refine_step(a, b, u, stats, state, g_extra=extra, m=m, v=v, grad_out=g, hist=hist, update=True)
        grads.append(ops.ncdhw(g).cpu().clone())
        path.append(tuple(ops.ncdhw(t).cpu().clone() for t in (u, m, v)))
    torch.cuda.synchronize()
    return path, grads, free, hist.cpu(), lr3, gs


@pytest.mark.parametrize('name', rc.SMALL)
def test_update_follows_float64_adam_given_the_gradient(name):
    tol = dc.TOL['adam']
    path, grads, free, hist, lr3, gs = _device_steps(name, 3)
    for k in range(3):
        assert torch.equal(grads[k], free[k]), 'grad_out of the updating launch differs from update = 0 at step %d' % (k + 1)
    disp0 = rc.inputs(name)[2]
    ref = rc.adam_path(disp0, grads, lr3, gs)
    for k in (1, 3):
        e = dc.adam_p_excess(path[k - 1][0].numpy(), disp0.numpy(), ref, k)
        assert e <= tol['p'], '%s: disp after %d steps: %.3e of max|update| beyond the store term (tolerance %.1e)' % (name, k, e, tol['p'])
        for j, what in ((1, 'm'), (2, 'v')):
            e = dc.dist(path[k - 1][j], ref[k - 1][j])
            assert e <= tol[what], '%s: %s after %d steps: %.3e (tolerance %.1e)' % (name, what, k, e, tol[what])
    assert (hist >= 0).all() and hist[1] < hist[0]                  # every slot written by its own launch
    if rc.CASES[name][0][0] == 1:                                   # an extent of 1 leaves its channel untouched
        assert torch.equal(path[2][0][:, 2], disp0[:, 2])


# ---- trajectories ----------------------------------------------------------------------------------------------------------------------
def _field(name, iters, **kw):
    from deepatlas_amd.lib.refine import refine_field
    mv, fx, disp = _up(*rc.inputs(name))
    keep = disp.clone()
    out = refine_field(mv, fx, disp, iters=iters, lr_vox=rc.TRAJ_LR, lambda_sim=rc.LAMBDA_SIM, lambda_reg=rc.reg_of(name), return_history=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(disp, keep), 'refine_field modified disp0'
    return out[0].cpu(), out[1].cpu()


@pytest.mark.parametrize('name', rc.TRAJ_CASES)
def test_five_iterations_against_the_float64_twin(name):
    t = rc.trajectory(name)
    disp0 = rc.inputs(name)[2]
    fused, hist = _field(name, rc.TRAJ_ITERS)
    d, dh = rc.traj_dist(fused, t['ref']['disp'], disp0, t['keep']), rc.rel_max(hist, t['ref']['hist'])
    print('%s: field %.2e (bound %.2e, %.2f %% left out)  history %.2e (bound %.2e)' % (name, d, t['bound_disp'], 100 * t['left_out'], dh, t['bound_hist']))
    assert d <= t['bound_disp'], '%s: refined field is %.3e from the float64 twin (bound %.1e)' % (name, d, t['bound_disp'])
    assert dh <= t['bound_hist'], '%s: history is %.3e from the float64 twin (bound %.1e)' % (name, dh, t['bound_hist'])
    if min(rc.CASES[name][0]) < 2:                     # da_warp_fwd refuses an extent of 1, so the composition says so; the fused route is the one that takes it
        with pytest.raises(ValueError, match='extent of 1'):
            _field(name, 1, fused=False)
        return
    composed, hist_c = _field(name, rc.TRAJ_ITERS, fused=False)
    dc_ = rc.traj_dist(composed, t['ref']['disp'], disp0, t['keep'])
    df = rc.traj_dist(composed, fused.double(), disp0, t['keep'])
    print('%s: composed %.2e from float64, %.2e from fused' % (name, dc_, df))
    assert df <= t['bound_disp'], '%s: fused=False is %.3e from fused=True after 5 iterations (bound %.1e)' % (name, df, t['bound_disp'])
    assert rc.rel_max(hist_c, hist.double()) <= t['bound_hist']
    one = rc.trajectory(name, 1)
    f1, c1 = _field(name, 1)[0], _field(name, 1, fused=False)[0]
    assert rc.traj_dist(c1, f1.double(), disp0, one['keep']) <= one['bound_disp']


@pytest.mark.parametrize('name', ('12x20x36', '1x9x40'))
def test_graph_replay_is_the_eager_loop_bit_for_bit(name):
    eager, he = _field(name, 6)
    graphed, hg = _field(name, 6, graph=True)
    assert torch.equal(eager, graphed) and torch.equal(he, hg)
    assert he[-1] < he[0]


def test_zero_iterations_return_the_field_and_mi_needs_the_composed_route():
    from deepatlas_amd.lib.refine import refine_field
    mv, fx, disp = _up(*rc.inputs('5x6x7'))
    out, hist = refine_field(mv, fx, disp, iters=0, lambda_reg=0.0, return_history=True)
    assert torch.equal(out, disp) and out.data_ptr() != disp.data_ptr() and hist.numel() == 0
    with pytest.raises(ValueError, match="supports sim = 'ncc'"):
        refine_field(mv, fx, disp, iters=1, sim='mi')
    with pytest.raises(ValueError, match='fused=False'):
        refine_field(mv, fx, disp, iters=1, lambda_jac=0.1)
    mv, fx, disp = _up(*rc.inputs('16x16x24o'))
    out, hist = refine_field(mv, fx, disp, iters=3, sim='mi', fused=False, lambda_jac=0.1, return_history=True)      # the other similarity, with the folding penalty
    assert torch.isfinite(out).all() and torch.isfinite(hist).all() and not torch.equal(out, disp)


# ---- recovery --------------------------------------------------------------------------------------------------------------------------
def test_recovers_a_known_field():
    from deepatlas_amd.lib.refine import refine_field, one_minus_ncc
    r = rc.recovery_twin()
    mv, fx, known = rc.recovery_inputs()
    mv, fx = _up(mv, fx)
    zero = torch.zeros_like(known).to(dev())
    out, hist = refine_field(mv, fx, zero, iters=rc.REC_ITERS, lr_vox=rc.REC_LR, lambda_reg=rc.REC_LAMBDA_REG, return_history=True)
    after = float(one_minus_ncc(mv, fx, out))
    epe = rc.endpoint_error(out, known)
    dh = rc.rel_max(hist.cpu(), r['ref']['hist'])
    print('recovery: 1 - NCC %.4f -> %.5f (float64 twin %.5f), endpoint error %.3f -> %.3f voxels (twin %.3f); history %.2e from the twin (bound %.2e)'
          % (float(hist[0]), after, r['sim_after'], r['epe_before'], epe, r['epe_after'], dh, r['bound_hist']))
    assert after <= 0.5 * float(hist[0]) and epe <= 0.5 * r['epe_before']
    assert dh <= r['bound_hist'], 'history is %.3e from the float64 twin (bound %.1e)' % (dh, r['bound_hist'])


# ---- the predictor ---------------------------------------------------------------------------------------------------------------------
class KnownField(torch.nn.Module):
    """Stand-in for a registration net: returns exactly the field it was given, and remembers the moving image it was shown."""

    def __init__(self, disp):
        super(KnownField, self).__init__()
        self.disp, self.seen = disp, None

    def forward(self, moving, fixed):
        self.seen = moving
        return self.disp, None, None


def test_predictor_refines_the_field_it_would_have_returned():
    from deepatlas_amd.lib.inference import RegistrationPredictor
    from deepatlas_amd.lib.refine import refine_field, one_minus_ncc
    mv, fx, disp = _up(*rc.inputs('16x16x24o'))
    kw = dict(iters=4, lr_vox=0.1, lambda_reg=0.5)
    got = RegistrationPredictor(KnownField(disp), refine=kw).field(mv[0, 0], fx[0, 0])
    assert torch.equal(got, refine_field(mv, fx, disp, **kw)) and not torch.equal(got, disp)
    plain = RegistrationPredictor(KnownField(disp)).field(mv[0, 0], fx[0, 0])
    assert torch.equal(plain, disp)
    p = RegistrationPredictor(KnownField(disp), refine=dict(iters=0, lambda_reg=0.0))
    assert torch.equal(p.field(mv[0, 0], fx[0, 0]), disp)                      # no iterations: the net's field bit for bit
    assert torch.equal(p.net_field(mv[0, 0], fx[0, 0]), disp) and torch.equal(p.refined(mv[0, 0], fx[0, 0], disp), disp)
    assert float(one_minus_ncc(mv, fx, got)) < float(one_minus_ncc(mv, fx, disp))
    assert torch.equal(RegistrationPredictor(KnownField(disp), refine=kw).field(mv[0, 0].double(), fx[0, 0].double()), got)      # a float64 prepared pair is cast
    with pytest.raises(ValueError, match="supports sim = 'ncc'"):
        RegistrationPredictor(KnownField(disp), refine=dict(iters=1, sim='mi', fused=True)).field(mv[0, 0], fx[0, 0])


def test_predictor_with_affine_init_refines_against_the_original_moving_image(monkeypatch):
    """The stand-in affine is a whole-voxel translation (exact in float32 on 5 x 9 x 17): the net sees the translated image, and the composed field is
    refined against the ORIGINAL one -- the result is refine_field(original moving, fixed, composed field) bit for bit."""
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics as metrics
    from deepatlas_amd.lib.inference import RegistrationPredictor
    from deepatlas_amd.lib.refine import refine_field
    import affine_cases as ac
    vol = ac.TRANSLATION_VOL
    mv, fx = _up(rc.sinusoid_image(vol, 1, 61), rc.sinusoid_image(vol, 1, 61, phase=0.4))
    theta = ac.translation_theta(1).to(dev())
    moved = ops.AffineWarpFn.apply(mv, theta)
    assert torch.equal(moved.cpu(), ac.shifted(mv.cpu(), ac.TRANSLATION_SHIFT))
    monkeypatch.setattr(metrics, 'affine_align', lambda im_m, im_t, mode, **kw: (theta, ops.AffineWarpFn.apply(im_m, theta)))
    net_field = rc.nudged(rc.smooth_field(vol, (0.3,), seed=62, taper=True), vol).to(dev())
    model = KnownField(net_field)
    kw = dict(iters=3, lr_vox=0.1, lambda_reg=0.5)
    got = RegistrationPredictor(model, affine_init='rigid', refine=kw).field(mv[0, 0], fx[0, 0])
    assert torch.equal(model.seen, moved)                                       # the net saw the pre-aligned image
    composed = ops.affine_disp(theta, net_field)
    assert torch.equal(got, refine_field(mv, fx, composed, **kw))
    assert not torch.equal(got, refine_field(moved, fx, composed, **kw))


# ---- the experiments -------------------------------------------------------------------------------------------------------------------
SHAPE = (16, 16, 32)


def _experiment(tmp_path, monkeypatch, extra):
    import train_reg
    from torch.utils.data import DataLoader
    from deepatlas_amd.lib.datasets import SyntheticRegDataset
    from deepatlas_amd.models.registration import RegistrationExperiment
    monkeypatch.chdir(tmp_path)
    ns = argparse.Namespace(device='0', debug=False, num_samples=3, num_epochs=1, lr=1e-3, test_only=False, data_root='./data', log_root='logs',
                            shape=list(SHAPE))
    cfg = train_reg.build_config(ns)
    cfg.update(extra)
    cfg['training_data_loader'] = DataLoader(SyntheticRegDataset(3, SHAPE, 32, seed=230), batch_size=1, shuffle=False)
    cfg['validation_data_loader'] = DataLoader(SyntheticRegDataset(2, SHAPE, 32, seed=1230), batch_size=1, shuffle=False)
    cfg.update(lr_mode='const', samples_per_epoch=2, print_batch_period=1)
    torch.manual_seed(11)
    exp = RegistrationExperiment(cfg)
    exp.train()
    return exp


def test_one_epoch_with_and_without_the_refine_key(tmp_path, monkeypatch, capsys):
    plain = _experiment(tmp_path, monkeypatch, {})
    out0 = capsys.readouterr().out
    refined = _experiment(tmp_path, monkeypatch, dict(refine=5))
    out1 = capsys.readouterr().out
    new = ['refined_dice_per_class', 'refined_dice_avg', 'refined_fold_frac', 'refine_sim_before', 'refine_sim_after']
    r0, r1 = plain.last_validation, refined.last_validation
    assert 'refine' not in plain.config and not any(k in r0 for k in new) and 'refine' not in out0
    assert sorted(r1) == sorted(list(r0) + new) and plain.exp_name == refined.exp_name
    for k in new[1:]:
        assert np.isfinite(r1[k]), (k, r1[k])
    assert r1['refine_sim_after'] <= r1['refine_sim_before']
    assert r1['dice_avg'] == r0['dice_avg'] and refined.best_score == plain.best_score          # model selection stays on the net's own field
    v0, v1 = ([l for l in o.splitlines() if l.startswith('Validation:')] for o in (out0, out1))
    assert len(v0) == len(v1) == 1
    tail = ', refined Dice %.4f (folding %.4f)' % (r1['refined_dice_avg'], r1['refined_fold_frac'])
    assert tail in v1[0] and v1[0].replace(tail, '').split(' (')[0:2] == v0[0].split(' (')[0:2]       # the line without the new part is the parent's
    print('one epoch at 16 x 16 x 32, 5 iterations: Dice %.4f -> refined %.4f, 1 - NCC %.4f -> %.4f' % (r1['dice_avg'], r1['refined_dice_avg'], r1['refine_sim_before'], r1['refine_sim_after']))


def test_validation_refines_a_batch_beyond_64_pairs_in_chunks():
    """65 pairs in one validation batch: refined as 64 + 1, and refine_sim_* are means over the PAIRS (each pair's own 1 - NCC)"""
    from deepatlas_amd.lib.refine import one_minus_ncc
    from deepatlas_amd.models.registration import eval_registration
    n, vol = 65, (8, 8, 8)
    mv, fx = rc.sinusoid_image(vol, n, 90), rc.sinusoid_image(vol, n, 90, phase=0.4)

    class Zero(torch.nn.Module):
        def forward(self, moving, fixed):
            return torch.zeros((moving.shape[0], 3) + tuple(moving.shape[2:]), device=moving.device), None, None
    seg = torch.zeros((n, 1) + vol, dtype=torch.long)
    res = eval_registration(Zero(), [(mv, fx, seg, seg, torch.zeros(n, dtype=torch.bool), ['p%d' % k for k in range(n)])], 4, dev(),
                            refine=dict(iters=2, lambda_reg=0.5))
    zero = torch.zeros((n, 3) + vol, device=dev())
    a, b = _up(mv, fx)
    want = torch.cat([one_minus_ncc(a[:64], b[:64], zero[:64], per_sample=True), one_minus_ncc(a[64:], b[64:], zero[64:], per_sample=True)]).double().mean()
    assert res['n_pairs'] == n and abs(res['refine_sim_before'] - float(want)) <= 1e-6
    assert res['refine_sim_after'] < res['refine_sim_before'] and np.isfinite(res['refined_fold_frac'])


# ---- predict_reg.py --------------------------------------------------------------------------------------------------------------------
# the files of tests/test_gpu_regapply.py's end-to-end test, built the same way: two scans of unequal spacing that prepare to 16 x 16 x 32 at 1 mm
SCANS = {'kneeLEFT0': ((12, 24, 17), (2.0, 0.75, 1.5), (-90.0, 120.0, -60.0)), 'kneeRIGHT1': ((9, 18, 68), (0.5, 1.0, 2.0), (75.0, -110.0, 40.0))}
N_CLASS = 4


def _write_pair_files(root):
    from deepatlas_amd.lib.nifti import write_nifti
    os.makedirs(str(root), exist_ok=True)
    for k, (name, (shape, spacing, origin)) in enumerate(sorted(SCANS.items())):
        z, y, x = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing='ij')
        lab = (1 + (x > 0.1 * k) + (y > -0.2)) * ((x ** 2 + y ** 2 + z ** 2) < 0.8)
        img = (lab * 200 + 50 * np.sin(3 * x + k) * np.cos(2 * y) + np.random.RandomState(k).uniform(0, 40, size=shape)).astype(np.int16)
        affine = np.diag(list(spacing) + [1.0])
        affine[:3, 3] = origin
        write_nifti(os.path.join(str(root), name + '_image.nii.gz'), img, spacing=spacing, affine=affine)
        write_nifti(os.path.join(str(root), name + '_masks.nii.gz'), lab.astype(np.uint8), spacing=spacing, affine=affine)
    listing = os.path.join(str(root), 'pairs.txt')
    with open(listing, 'w') as f:
        f.write('kneeLEFT0 kneeRIGHT1\nkneeRIGHT1, kneeLEFT0\n')
    return listing


def _write_checkpoint(folder):
    import json
    from deepatlas_amd.lib.network_factory import get_network
    os.makedirs(str(folder), exist_ok=True)
    torch.manual_seed(3)
    model = get_network('voxel_morph_cvpr')()
    model.weights_init()
    ckpt = os.path.join(str(folder), 'checkpoint.pth.tar')
    torch.save({'epoch': 0, 'model_state_dict': model.state_dict(), 'best_score': 0.0}, ckpt)
    cfg = {'data': 'OAI', 'model': 'voxel_morph_cvpr', 'model_settings': {}, 'n_classes': N_CLASS, 'crop_size': [1, 1, 1], 'lambda_reg': 1.0,
           'preprocess': [['resample', {'voxel_size': [1.0, 1.0, 1.0]}], ['percentile_rescale', {'lo': 0.5, 'hi': 99.5}], ['left_to_right', {}]]}
    with open(os.path.join(str(folder), 'train_config.json'), 'w') as f:
        json.dump(cfg, f)
    return ckpt


def test_predict_reg_refine_end_to_end(tmp_path):
    import re
    import regapply_cases as gc
    from deepatlas_amd.lib.nifti import read_nifti, read_nifti_field
    root = tmp_path / 'scans'
    listing = _write_pair_files(root)
    ckpt = _write_checkpoint(tmp_path / 'ckpt')
    out_dir = tmp_path / 'out'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'predict_reg.py'), '--ckpt', ckpt, '--output-dir', str(out_dir), '--data-dir', str(root), '--pair-list',
                          listing, '--label-dir', str(root), '--save-field', '--refine', '5'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=240)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.splitlines()
    found = [re.fullmatch(r'refine: 1-NCC (\d\.\d{4}) -> (\d\.\d{4}) \(5 iterations\)', l) for l in lines if l.startswith('refine:')]
    assert len(found) == 2 and all(found), lines
    for m_ in found:
        assert float(m_.group(2)) <= float(m_.group(1))
    for m, f in (('kneeLEFT0', 'kneeRIGHT1'), ('kneeRIGHT1', 'kneeLEFT0')):
        stem = os.path.join(str(out_dir), '%s_to_%s' % (m, f))
        fixed, moving = read_nifti(os.path.join(str(root), f + '_image.nii.gz')), read_nifti(os.path.join(str(root), m + '_image.nii.gz'))
        warped, seg, fld = read_nifti(stem + '_warped.nii.gz'), read_nifti(stem + '_seg.nii.gz'), read_nifti_field(stem + '_field.nii.gz')
        assert warped.array.shape == seg.array.shape == fixed.array.shape and fld.array.shape == (3,) + fixed.array.shape and np.isfinite(fld.array).all()
        # the warped file from the field file, as test_gpu_regapply.py re-derives it: y = A_m^-1 (d + A_f (x, 1)), cubic interpolation of the moving file
        x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in fixed.array.shape], indexing='ij')
        world = [fixed.affine[r, 0] * x[2] + fixed.affine[r, 1] * x[1] + fixed.affine[r, 2] * x[0] + fixed.affine[r, 3] + fld.array[r].astype(np.float64) for r in range(3)]
        inv = np.linalg.inv(moving.affine)
        ijk = [inv[r, 0] * world[0] + inv[r, 1] * world[1] + inv[r, 2] * world[2] + inv[r, 3] for r in range(3)]
        y = np.stack([ijk[2], ijk[1], ijk[0]])
        n = moving.array.shape
        src = moving.array[None]
        keep = ~gc.guard_mask(y, n, 3)
        inside = np.all([(y[a] >= -0.5) & (y[a] < n[a] - 0.5) for a in range(3)], axis=0)
        ys = np.where(inside[None], y, 0)
        ref = np.where(inside, gc.interpolate(gc.prefilter_ref64(src), ys, 3)[0], 0.0)
        low = np.where(inside, gc.interpolate(gc.prefilter_f32(src), ys.astype(np.float32), 3, np.float32)[0], 0.0)
        steep = max(float(np.abs(np.diff(moving.array.astype(np.float64), axis=a)).max()) for a in range(3))
        tol = gc.TOL_FACTOR * float(np.max(np.abs(low - ref)[keep])) + 1.5 * steep * 3 * (2.0 ** -24 * 256 / 0.5) + gc.FLOOR * float(np.abs(src).max())
        err = float(np.max(np.abs(warped.array - ref)[keep]))
        assert keep.mean() >= 1 - gc.GUARD_CAP and err <= tol, (err, tol)
        line = [l for l in lines if l.startswith('%s_to_%s: ' % (m, f))]
        assert len(line) == 1 and ', unrefined ' in line[0] and 'det J mean' in line[0]
