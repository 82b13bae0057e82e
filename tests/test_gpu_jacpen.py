"""GPU: the Jacobian folding penalty kernels (jacpen.hip) against the float64 reference of tests/jacpen_cases.py, their agreement with the
folding statistics of ops.jacobian_det, and the penalty inside the registration and joint steps.  Every bound comes from jacpen_cases.bounds():
4 x the float32 torch evaluation's own distance from float64, floors 5e-7 (loss, relative) and 1e-6 (gradient, max norm over the gradient's max)."""
import math

import pytest
import torch

import jacpen_cases as jc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def _run(name, eps, p, upstream=1.0, channels_last=False):
    """(loss, d (upstream x loss) / d disp) of a case on the device.  The case's field is NCDHW-contiguous (the op copies it into its own
    layout); channels_last hands in the layout the registration net produces (taken as a view)."""
    x = jc.field(name).to(dev())
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last_3d)
    x.requires_grad_(True)
    from deepatlas_amd.lib.loss import JacobianFoldingLoss
    loss = JacobianFoldingLoss(eps=eps, power=p)(x)
    (loss * upstream if upstream != 1.0 else loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad


@pytest.mark.parametrize('name,eps,p', jc.COMBOS, ids=jc.COMBO_IDS)
def test_penalty_matches_the_float64_reference(name, eps, p):
    loss, grad = _run(name, eps, p)
    l64, g64 = jc.reference(name, eps, p)
    lb, gb = jc.bounds(name, eps, p)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.dtype == torch.float32 and grad.shape == jc.field(name).shape
    dl, dg = abs(float(loss) - l64) / abs(l64), jc.rel_max(grad.cpu(), g64)
    print('%s eps %g p %d: loss %.9e (float64 %.9e) rel %.2e (bound %.1e); gradient %.2e (bound %.1e)' % (name, eps, p, float(loss), l64, dl, lb, dg, gb))
    assert dl <= lb and dg <= gb


@pytest.mark.parametrize('name', jc.IDS)
def test_upstream_gradient_and_the_channels_last_layout(name):
    """3.5 x L from a channels-last field: the same loss, 3.5 x the gradient (the factor is applied on the device)."""
    k = jc.IDS.index(name)
    eps, p = jc.EPS_VALUES[k % 2], jc.POWERS[(k // 2) % 2]
    loss, grad = _run(name, eps, p, upstream=3.5, channels_last=True)
    plain, _ = _run(name, eps, p)
    l64, g64 = jc.reference(name, eps, p)
    lb, gb = jc.bounds(name, eps, p)
    assert torch.equal(loss, plain)
    dl, dg = abs(float(loss) - l64) / abs(l64), jc.rel_max(grad.cpu(), 3.5 * g64)
    print('%s eps %g p %d: loss rel %.2e (bound %.1e); gradient %.2e (bound %.1e)' % (name, eps, p, dl, lb, dg, gb))
    assert dl <= lb and dg <= gb


@pytest.mark.parametrize('name', [n for n in jc.IDS if min(jc.CASES[n][0]) >= 2])
def test_penalty_agrees_with_the_folding_statistics(name):
    """eps = 0, p = 1: L N V = -sum min(det, 0) over the determinant map of ops.jacobian_det, and as many active voxels as it counts folds."""
    from deepatlas_amd import ops
    x = jc.field(name).to(dev())
    loss, stats = ops.jacobian_penalty_stats(x, 0.0, 1)
    jstats, det = ops.jacobian_det(x, return_map=True)
    torch.cuda.synchronize()
    nv = det.numel()
    want = float(-det.double().clamp(max=0).sum())
    lb, _ = jc.bounds(name, 0.0, 1)
    print('%s: L N V %.9e, penalty sum %.9e, -sum min(det, 0) %.9e; active %d, folds %d' % (name, float(loss) * nv, float(stats[0]), want, int(stats[1]), int(jstats[:, 4].sum())))
    assert want > 0.0
    assert abs(float(loss) * nv - want) / want <= lb and abs(float(stats[0]) - want) / want <= lb
    assert int(stats[1]) == int(jstats[:, 4].sum()) == int((det < 0).sum())
    assert torch.equal(loss, _run(name, 0.0, 1)[0])              # the autograd op and the statistics call are one kernel


def test_identity_field_has_zero_loss_and_an_exactly_zero_gradient():
    from deepatlas_amd.lib.loss import JacobianFoldingLoss
    for shape in ((2, 3, 5, 6, 7), (1, 3, 1, 4, 6), (1, 3, 2, 2, 2)):
        for eps in (0.0, 0.25, 1.0):                             # det = 1 exactly; active means det < eps, strictly
            for p in jc.POWERS:
                x = torch.zeros(shape, device=dev(), requires_grad=True)
                loss = JacobianFoldingLoss(eps=eps, power=p)(x)
                (loss * 3.5).backward()
                assert float(loss.detach()) == 0.0 and x.grad.shape == x.shape and not bool(x.grad.any()), (shape, eps, p)


@pytest.mark.parametrize('name', ['17x30x22', '33x47x61', '80x96x80'])
def test_two_runs_are_bit_identical(name):
    a, b = _run(name, 0.25, 2, upstream=3.5), _run(name, 0.25, 2, upstream=3.5)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')], ids=['nan', 'inf', '-inf'])
def test_a_non_finite_displacement_gives_a_non_finite_loss(value):
    """Nothing in the kernels is indexed by a data value: the loss is not finite, the backward pass runs, and the gradient is untouched
    three voxels away (a gradient entry reads the determinants of its six neighbours, those the displacements of theirs)."""
    from deepatlas_amd.lib.loss import JacobianFoldingLoss
    name = '17x30x22'
    _, clean = _run(name, 0.25, 1)
    for at in ((1, 2, 8, 15, 11), (0, 0, 0, 0, 0), (2, 1, 16, 29, 21)):      # inside, the two opposite corners; (n, c, d, h, w)
        x = jc.field(name).to(dev()).clone()
        x[at] = value
        x.requires_grad_(True)
        loss = JacobianFoldingLoss(eps=0.25, power=1)(x)
        loss.backward()
        torch.cuda.synchronize()
        assert not math.isfinite(float(loss)), (at, float(loss))
        n, _, d, h, w = at
        far = torch.ones(x.shape, dtype=torch.bool, device=dev())
        far[n, :, max(d - 2, 0):d + 3, max(h - 2, 0):h + 3, max(w - 2, 0):w + 3] = False
        assert torch.equal(x.grad[far], clean[far])


def test_descent_on_the_penalty_alone_removes_folds():
    """Plain gradient descent with the step size and count of jacpen_cases (chosen on the CPU, where the float64 twin's loss falls at every
    step and its folding count ends below a quarter): on the device the loss falls at every step and the folding count of ops.jacobian_det
    ends below half of the first one -- the factor two is the margin for float32 and for folds created at the threshold."""
    from deepatlas_amd import ops
    x = jc.field(jc.DESCENT_CASE).to(dev())
    losses, folds = [], []
    for _ in range(jc.DESCENT_STEPS + 1):
        x = x.detach().requires_grad_(True)
        loss = ops.JacobianPenaltyFn.apply(x, jc.DESCENT_EPS, jc.DESCENT_POWER)
        loss.backward()
        losses.append(float(loss))
        folds.append(int(ops.jacobian_det(x)[:, 4].sum()))
        x = x.detach() - jc.DESCENT_LR * x.grad
    print(['%.4e' % v for v in losses], folds)
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert folds[0] > 1000 and folds[-1] < folds[0] / 2


# ---- the steps -------------------------------------------------------------------------------------------------------------------------
SHAPE, C = (16, 16, 32), 8
JAC = {'eps': 1.0, 'power': 2}           # eps = 1: every voxel that shrinks is active, so the term is not zero on an untrained net's smooth field
ENTRIES = ('da_jacdet_penalty_fwd', 'da_jacdet_penalty_bwd')


def _nets():
    from oracle import nets
    from deepatlas_amd.lib.network_factory import get_network, unets
    spec = nets.UNET_TINY
    seg_sd = nets.closed_form_fill(nets.unet_param_shapes(1, C, spec['encoders'], spec['decoders']), seed=1)
    reg_sd = nets.closed_form_fill(nets.voxelmorph_param_shapes(), seed=4)
    seg = unets.UNet_generator(encoders=spec['encoders'], decoders=spec['decoders'], act='LeakyReLU')(in_channel=1, n_classes=C, bias=True, BN=True)
    seg.load_state_dict({k: v.clone() for k, v in seg_sd.items()}, strict=True)
    reg = get_network('voxel_morph_cvpr')()
    reg.load_state_dict({k: v.clone() for k, v in reg_sd.items()}, strict=True)
    return seg.to(dev()), reg.to(dev())


def _pair():
    from oracle import nets
    im_m = nets.closed_form_volume((1, 1) + SHAPE, seed=5)
    im_t = nets.closed_form_volume((1, 1) + SHAPE, seed=6)
    sm, st_ = nets.closed_form_labels((1,) + SHAPE, C, seed=7), nets.closed_form_labels((1,) + SHAPE, C, seed=8)
    return im_m.to(dev()), im_t.to(dev()), sm.to(dev()), st_.to(dev())


def _profiled(fn):
    """fn() under a CallProfiler: (result, the C entries it called)."""
    from deepatlas_amd import _native
    prev, _native.profiler = _native.profiler, _native.CallProfiler()
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {key[0] for key in _native.profiler.records}
    finally:
        _native.profiler = prev


def test_registration_step_with_the_penalty():
    from deepatlas_amd.models.joint import RegistrationStep
    from deepatlas_amd.optim import FlatAdam
    _, reg = _nets()
    im_m, im_t, _, _ = _pair()
    opt = FlatAdam(reg.parameters(), lr=1e-3)
    before = opt.flat_p.detach().clone()
    step = RegistrationStep(reg, opt, lam_reg=0.5, lam_jac=0.7, jac_settings=JAC)
    r, called = _profiled(lambda: step.gradients(im_m, im_t))
    assert set(ENTRIES) <= called
    assert 'jac' in r and float(r['jac']) > 0.0
    assert float(r['loss']) == float((r['sim'] + 0.5 * r['bend']) + 0.7 * r['jac'])
    out = step(im_m, im_t)                                       # the return tuple keeps its shape
    torch.cuda.synchronize()
    assert len(out) == 3 and len(out[1]) == 3 and len(out[2]) == 2 and torch.equal(step.last_jac, r['jac'])
    for t in (out[0], out[1][0], r['jac'], opt.flat_p):
        assert bool(torch.isfinite(t).all())
    assert not torch.equal(before, opt.flat_p)


def test_joint_step_with_the_penalty_in_every_branch():
    from deepatlas_amd.models.joint import DeepAtlasJointStep
    from deepatlas_amd.optim import FlatAdam
    seg, reg = _nets()
    im_m, im_t, sm, st_ = _pair()
    so, ro = FlatAdam(seg.parameters(), lr=1e-3), FlatAdam(reg.parameters(), lr=1e-3)
    step = DeepAtlasJointStep(seg, so, reg, ro, C, lam_sim=0.9, lam_reg=0.5, lam_anat=0.8, lam_sp=1.0, lam_jac=0.7, jac_settings=JAC)
    for seg_m, seg_t in ((sm, st_), (None, st_), (sm, None), (None, None)):
        r = step(im_m, im_t, seg_m, seg_t)
        torch.cuda.synchronize()
        assert 'jac' in r and float(r['jac']) > 0.0
        for k, v in r.items():
            assert bool(torch.isfinite(v).all()), k
        want = 0.9 * r['sim'] + 0.5 * r['bend']
        if seg_m is not None or seg_t is not None:
            want = want + 0.8 * r['anat_reg']
        assert float(r['loss_reg']) == float(want + 0.7 * r['jac']), (seg_m is None, seg_t is None)
    assert bool(torch.isfinite(so.flat_p).all()) and bool(torch.isfinite(ro.flat_p).all())


@pytest.mark.parametrize('which', ['reg', 'joint'])
def test_step_with_the_penalty_replays_as_a_hip_graph(which):
    """The penalty kernels use the workspace only (no allocation, no synchronisation): the step captured by graphs.GraphedStep trains like
    the eager one, bit for bit (deterministic mode for the warp's adjoint scatter)."""
    from deepatlas_amd import ops
    from deepatlas_amd.graphs import GraphedStep
    from deepatlas_amd.models.joint import DeepAtlasJointStep, RegistrationStep
    from deepatlas_amd.optim import FlatAdam
    prev = ops.set_deterministic(True)
    results = []
    try:
        for graph in (False, True):
            seg, reg = _nets()
            im_m, im_t, sm, st_ = _pair()
            so, ro = FlatAdam(seg.parameters(), lr=1e-3), FlatAdam(reg.parameters(), lr=1e-3)
            if which == 'reg':
                segments, between, opts = RegistrationStep(reg, ro, lam_jac=0.7, jac_settings=JAC).segments(im_m, im_t)
            else:
                segments, between, opts = DeepAtlasJointStep(seg, so, reg, ro, C, lam_jac=0.7, jac_settings=JAC).segments(im_m, im_t, sm, st_)
            g = GraphedStep(segments, opts, between=between, warmup=1 if graph else 10 ** 9)
            jacs = [float(g()['jac'].item()) for _ in range(4)]            # graphed: 1 eager, capture + replay, 2 replays
            assert (g.graphs is not None) == graph
            torch.cuda.synchronize()
            results.append((jacs, torch.cat([o.flat_p.detach().cpu() for o in opts])))
            g.close()
    finally:
        ops.set_deterministic(prev)
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert all(math.isfinite(v) and v > 0.0 for v in results[0][0]) and len(set(results[0][0])) == 4
    assert torch.equal(results[0][1], results[1][1])


@pytest.mark.parametrize('which', ['reg', 'joint'])
def test_zero_weight_is_the_step_without_the_argument(which):
    """lam_jac = 0: no module, none of the new entries called, and in deterministic mode the loss and the gradients are bit-identical to a
    step constructed without the argument."""
    from deepatlas_amd import ops
    from deepatlas_amd.models.joint import DeepAtlasJointStep, RegistrationStep
    from deepatlas_amd.optim import FlatAdam
    prev = ops.set_deterministic(True)
    got = []
    try:
        for kw in ({}, {'lam_jac': 0.0, 'jac_settings': JAC}):
            seg, reg = _nets()
            im_m, im_t, sm, st_ = _pair()
            so, ro = FlatAdam(seg.parameters(), lr=1e-3), FlatAdam(reg.parameters(), lr=1e-3)
            if which == 'reg':
                step = RegistrationStep(reg, ro, **kw)
                r, called = _profiled(lambda: step.gradients(im_m, im_t))
                loss = r['loss']
            else:
                step = DeepAtlasJointStep(seg, so, reg, ro, C, **kw)
                r, called = _profiled(lambda: step.reg_gradients(im_m, im_t, sm, st_))
                loss = r['loss_reg']
            assert step.jac is None and 'jac' not in r
            assert not called & set(ENTRIES) and 'da_bending_fwd' in called
            got.append((loss.clone(), next(reg.parameters()).grad.detach().clone(), ro.flat_g.detach().clone()))
    finally:
        ops.set_deterministic(prev)
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert bool(got[0][1].any())


# ---- the experiments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['reg', 'joint'])
def test_experiment_trains_with_the_penalty_and_logs_it(which, tmp_path, monkeypatch, capsys):
    """--lambda-jac through build_config into one epoch of the experiment: the name carries the weight, the training line the term."""
    import argparse
    from torch.utils.data import DataLoader
    import train_joint
    import train_reg
    from deepatlas_amd.lib.datasets import SyntheticRegDataset, SyntheticSegDataset
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    from deepatlas_amd.models.registration import RegistrationExperiment
    monkeypatch.chdir(tmp_path)
    shape = (16, 16, 32)
    ns = argparse.Namespace(device='0', debug=False, num_samples=3, num_epochs=1, lr=1e-3, test_only=False, data_root='./data', log_root='logs',
                            shape=list(shape), lambda_jac=0.5, jac_eps=1.0, jac_power=2)
    if which == 'reg':
        cfg = train_reg.build_config(ns)
        cfg['training_data_loader'] = DataLoader(SyntheticRegDataset(3, shape, 32, seed=230), batch_size=1, shuffle=False)
        cfg['validation_data_loader'] = DataLoader(SyntheticRegDataset(2, shape, 32, seed=1230), batch_size=1, shuffle=False)
        make = RegistrationExperiment
    else:
        ns.num_labeled = 3
        cfg = train_joint.build_config(ns)
        cfg['training_data_loader'] = DataLoader(SyntheticRegDataset(3, shape, 32, seed=230, labeled=[0, 1, 2]), batch_size=1, shuffle=False)
        cfg['validation_data_loader'] = DataLoader(SyntheticSegDataset(2, shape, 32, seed=1230), batch_size=1, shuffle=False)
        cfg['validation_pair_loader'] = DataLoader(SyntheticRegDataset(2, shape, 32, seed=1230), batch_size=1, shuffle=False)
        make = DeepAtlasExperiment
    cfg.update(lr_mode='const', samples_per_epoch=2, print_batch_period=1)
    exp = make(cfg)
    assert exp.exp_name.endswith('_jac0.5') and exp.lambda_jac == 0.5 and exp.jac_settings == {'eps': 1.0, 'power': 2}
    exp.train()
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith('Epoch[')]
    assert len(lines) == 2 and all(' jac: ' in l for l in lines), out
    assert all(float(l.split(' jac: ')[1].split()[0]) > 0.0 for l in lines)
    assert exp.step.jac is not None and (exp.step.jac.eps, exp.step.jac.power) == (1.0, 2)
    assert 0.0 <= exp.last_validation['nonpos_frac'] <= 1.0
