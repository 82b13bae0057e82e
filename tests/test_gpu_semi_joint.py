"""GPU: the joint step on pairs whose FIXED image has no manual segmentation (models/joint.py, seg_t=None), 16 x 16 x 32, C = 8 and 32.

The step is compared with a twin composed HERE from oracle.nets / oracle.losses (no code of deepatlas_amd): registration phase with the segmentation
net's eval-mode probabilities of the fixed image as Dice's target and the warped one-hot moving label as its source; segmentation phase as ONE
train-mode forward of cat([im_m, im_t]) with the supervised Dice on the moving half and Dice(softmax(Z_t), warped label) on the fixed half.  The twin
runs in fp32 (two steps: the loss terms) and in float64 (first step: the yardstick of the gradients).  Bounds are those of
test_gpu_nets.py::test_joint_step_vs_oracle: loss terms 1e-4 relative on the first step and 1e-3 on the second; a first-step gradient is no further
from the float64 twin than 5 x (deterministic mode; 10 x otherwise) the fp32 twin's own distance -- for that tensor or the median over the net, whichever
is larger -- and never held tighter than 2e-5; conv biases in front of a BatchNorm (zero analytic gradient) are held absolutely.
Also: fused against composed anatomy terms, the neither-labelled case (segmentation net, buffers and Adam state untouched; registration gradients those
of RegistrationStep), the labelled cases unchanged by an earlier seg_t=None call, and DeepAtlasExperiment / train_joint.py with the wider pair modes."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

from conftest import rel_l2
from test_gpu_nets import _joint_setup, dev

pytestmark = pytest.mark.gpu

SHAPE = (16, 16, 32)
LOSS_KEYS = ('sim', 'bend', 'anat_reg', 'sup', 'anat_seg', 'loss_reg', 'loss_seg')


# ---- the twin --------------------------------------------------------------------------------------------------------------------
def twin_step(seg_sd, seg_opt, reg_sd, reg_opt, im_m, im_t, seg_m, spec, C):
    """One step for seg_t=None on CPU tensors of one dtype (issue semantics; weights 1, 'Uniform', no_bg=False, eps=1e-6)."""
    from oracle import nets, losses, steps
    dt = im_m.dtype
    dice = lambda s, t, softmax: losses.dice_loss(s, t, C, weight_type='Uniform', no_bg=False, softmax=softmax, eps=1e-6)
    if seg_m is not None:
        with torch.no_grad():
            prob_t = F.softmax(nets.unet_forward(seg_sd, im_t, spec, training=False), dim=1)
        onehot_m = losses.mask_to_one_hot(seg_m.long().unsqueeze(1), C).to(dt)
    rn = reg_opt.names
    for n in rn:
        reg_sd[n].requires_grad_(True)
    disp, warped, deform = nets.voxelmorph_forward(reg_sd, im_m, im_t)
    l_sim, l_reg = losses.ncc_loss(warped, im_t), losses.bending_energy_loss(disp)
    zero = torch.zeros((), dtype=dt)
    if seg_m is not None:
        warped_lab = nets.warp_trilinear(onehot_m, deform)
        l_anat = dice(warped_lab, prob_t, False)
        loss_r = l_sim + l_reg + l_anat
    else:
        l_anat, loss_r = zero, l_sim + l_reg
    g = steps._grads(loss_r, reg_sd, rn)
    for n in rn:
        reg_sd[n].requires_grad_(False)
    reg_opt.step(reg_sd, g)
    out = dict(sim=l_sim.detach(), bend=l_reg.detach(), anat_reg=l_anat.detach(), loss_reg=loss_r.detach(), grads_reg=g)
    if seg_m is None:
        out.update(sup=zero, anat_seg=zero, loss_seg=zero, grads_seg=None)
        return out
    sn = seg_opt.names
    for n in sn:
        seg_sd[n].requires_grad_(True)
    logits = nets.unet_forward(seg_sd, torch.cat([im_m, im_t]), spec, training=True)
    n_m = im_m.shape[0]
    l_sp = dice(logits[:n_m], seg_m.long(), True)
    l_anat2 = dice(logits[n_m:], warped_lab.detach(), True)
    loss_s = l_sp + l_anat2
    g2 = steps._grads(loss_s, seg_sd, sn)
    for n in sn:
        seg_sd[n].requires_grad_(False)
    seg_opt.step(seg_sd, g2)
    out.update(sup=l_sp.detach(), anat_seg=l_anat2.detach(), loss_seg=loss_s.detach(), grads_seg=g2)
    return out


_TWINS = {}


def twins(C, labelled):
    """(fp32 twin: two steps, float64 twin: first step) on the closed-form inputs of test_gpu_nets._joint_setup; computed once per process, not modified"""
    key = (C, labelled)
    if key not in _TWINS:
        from oracle import nets, steps
        spec = nets.UNET_TINY
        res = {}
        for dt in (torch.float32, torch.float64):
            cast = lambda sd: {k: (v.clone().to(dt) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
            seg_sd = cast(nets.closed_form_fill(nets.unet_param_shapes(1, C, spec['encoders'], spec['decoders']), seed=1))
            reg_sd = cast(nets.closed_form_fill(nets.voxelmorph_param_shapes(), seed=4))
            im_m, im_t = nets.closed_form_volume((1, 1) + SHAPE, seed=5).to(dt), nets.closed_form_volume((1, 1) + SHAPE, seed=6).to(dt)
            sm = nets.closed_form_labels((1,) + SHAPE, C, seed=7) if labelled else None
            so, ro = steps.Adam(steps.trainable(seg_sd)), steps.Adam(steps.trainable(reg_sd))
            res[dt] = [twin_step(seg_sd, so, reg_sd, ro, im_m, im_t, sm, spec, C) for _ in range(2 if dt == torch.float32 else 1)]
        _TWINS[key] = (res[torch.float32], res[torch.float64][0])
    return _TWINS[key]


def _check_losses(out, ref, s):
    for k in LOSS_KEYS:
        r = float(ref[k])
        assert abs(out[k].item() - r) < (1e-4 if s == 0 else 1e-3) * max(1.0, abs(r)), (s, k, out[k].item(), r)


def _check_grads(net, phase, t32, t64, gbound):
    g32, g64 = t32['grads_' + phase], t64['grads_' + phase]
    skip = lambda n: phase == 'seg' and (n.endswith('conv.bias') or n.endswith('deconv.bias'))      # zero analytic gradient in front of a BatchNorm
    floors = {n: rel_l2(g32[n].numpy(), g64[n].numpy()) for n, _ in net.named_parameters() if not skip(n)}
    med = float(np.median(list(floors.values())))
    worst = 0.0
    for n, p in net.named_parameters():
        got = p.grad.detach().cpu().numpy()
        if skip(n):
            assert np.abs(got - g32[n].numpy()).max() < 1e-5, (phase, n)
            continue
        err = rel_l2(got, g64[n].numpy())
        worst = max(worst, err / max(floors[n], med))
        assert err < max(gbound * max(floors[n], med), 2e-5), (phase, n, err, floors[n], med, gbound)
    return worst


def _step_objects(C, fused=True):
    from deepatlas_amd.optim import FlatAdam
    from deepatlas_amd.models.joint import DeepAtlasJointStep
    spec, seg_sd, reg_sd, seg, reg, (im_m, im_t, sm, st_) = _joint_setup(C, SHAPE)
    step = DeepAtlasJointStep(seg, FlatAdam(seg.parameters(), lr=1e-3), reg, FlatAdam(reg.parameters(), lr=1e-3), C, fused=fused)
    d = dev()
    return step, seg, reg, (im_m.to(d), im_t.to(d), sm.to(d), st_.to(d))


def _run(step, args, deterministic):
    from deepatlas_amd import ops
    prev = ops.set_deterministic(deterministic)
    try:
        out = step(*args)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
    return out


@pytest.mark.parametrize('deterministic', [True, False], ids=['deterministic', 'default'])
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
@pytest.mark.parametrize('C', [8, 32])
def test_moving_labelled_fixed_unlabelled_vs_twin(C, fused, deterministic):
    """seg_m given, seg_t=None: the seven loss terms of two consecutive steps and every first-step gradient of both nets; with the fused anatomy kernels
    and with the op-by-op composition (fused=False), both held to the same float64 twin."""
    step, seg, reg, (im_m, im_t, sm, _) = _step_objects(C, fused)
    t32, t64 = twins(C, True)
    for s in range(2):
        out = _run(step, (im_m, im_t, sm, None), deterministic)
        assert set(out) == set(LOSS_KEYS)
        _check_losses(out, t32[s], s)
        if s == 0:
            assert out['sup'].item() > 0 and out['anat_reg'].item() > 0 and out['anat_seg'].item() > 0
            gbound = 5 if deterministic else 10
            w = [_check_grads(net, phase, t32[0], t64, gbound) for net, phase in ((reg, 'reg'), (seg, 'seg'))]
            print('C=%d fused=%s deterministic=%s: worst gradient distance / fp32 twin floor: reg %.2f, seg %.2f' % (C, fused, deterministic, w[0], w[1]))


@pytest.mark.parametrize('C', [8, 32])
def test_neither_labelled(C):
    """seg_m = seg_t = None: NCC + bending only, against the twin; the segmentation net's parameters, BatchNorm buffers and Adam state (step count included) stay
    bit-identical; the registration gradients are those of RegistrationStep on the same inputs."""
    from deepatlas_amd import ops
    from deepatlas_amd.optim import FlatAdam
    from deepatlas_amd.models.joint import RegistrationStep
    step, seg, reg, (im_m, im_t, sm, st_) = _step_objects(C)
    _run(step, (im_m, im_t, sm, st_), True)                       # one ordinary step first: the segmentation optimiser then HAS state to keep
    snap = lambda: ({k: v.detach().clone() for k, v in seg.state_dict().items()},
                    [{k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in step.seg_opt.state[p].items()} for p in step.seg_opt.param_groups[0]['params']],
                    step.seg_opt._steps)
    before = snap()
    reg_before = {k: v.detach().clone() for k, v in reg.state_dict().items()}
    out = _run(step, (im_m, im_t, None, None), True)
    after = snap()
    assert set(out) == set(LOSS_KEYS)
    assert all(out[k].item() == 0.0 for k in ('anat_reg', 'sup', 'anat_seg', 'loss_seg'))
    assert before[2] == after[2] >= 1
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k
    for a, b in zip(before[1], after[1]):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    got = {n: p.grad.detach().clone() for n, p in reg.named_parameters()}
    # RegistrationStep from the same weights on the same inputs
    _, _, _, _, reg2, _ = _joint_setup(C, SHAPE)
    reg2.load_state_dict(reg_before)
    ops.bump_weights_epoch()
    rstep = RegistrationStep(reg2, FlatAdam(reg2.parameters(), lr=1e-3))
    r = _run(rstep.gradients, (im_m, im_t), True)
    assert out['sim'].item() == r['sim'].item() and out['bend'].item() == r['bend'].item() and out['loss_reg'].item() == r['loss'].item()
    for n, p in reg2.named_parameters():
        assert torch.equal(got[n], p.grad), n
    # ... and against the twin, from fresh weights
    step, seg, reg, (im_m, im_t, _, _) = _step_objects(C)
    t32, t64 = twins(C, False)
    for s in range(2):
        out = _run(step, (im_m, im_t, None, None), True)
        _check_losses(out, t32[s], s)
        if s == 0:
            _check_grads(reg, 'reg', t32[0], t64, 5)


@pytest.mark.parametrize('C', [8, 32])
def test_labelled_cases_are_unchanged_by_an_earlier_unlabelled_call(C):
    """The two existing cases (seg_t given) from a step object that has served seg_t=None calls are bit-equal, in deterministic mode, to the same cases from a
    step object that never has: losses and every gradient of both nets."""
    from deepatlas_amd import ops
    results = []
    for visited in (False, True):
        step, seg, reg, (im_m, im_t, sm, st_) = _step_objects(C)
        init = ({k: v.detach().clone() for k, v in seg.state_dict().items()}, {k: v.detach().clone() for k, v in reg.state_dict().items()})
        res = []
        for seg_m in (sm, None):
            if visited:
                _run(step, (im_m, im_t, sm, None), True)
                _run(step, (im_m, im_t, None, None), True)
            with torch.no_grad():                                  # the same weights and BatchNorm buffers for every compared call
                for net, sd in ((seg, init[0]), (reg, init[1])):
                    for k, v in net.state_dict().items():
                        v.copy_(sd[k])
            ops.bump_weights_epoch()
            out = _run(step, (im_m, im_t, seg_m, st_), True)
            res.append(({k: out[k].item() for k in LOSS_KEYS}, {n: p.grad.detach().clone() for net in (reg, seg) for n, p in net.named_parameters()}))
        results.append(res)
    for (la, ga), (lb, gb) in zip(*results):
        assert la == lb, (la, lb)
        for n in ga:
            assert torch.equal(ga[n], gb[n]), n


def test_segments_refuses_an_unlabelled_fixed_image():
    step, _, _, (im_m, im_t, sm, _) = _step_objects(8)
    with pytest.raises(NotImplementedError):
        step.segments(im_m, im_t, sm, None)


# ---- experiment and command line -------------------------------------------------------------------------------------------------
def _experiment(tmp, pairs):
    import train_joint
    from deepatlas_amd.lib.datasets import SyntheticRegDataset, SyntheticSegDataset
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    shape = [16, 16, 32]
    ns = argparse.Namespace(device='0', debug=False, num_samples=4, num_epochs=1, lr=1e-3, test_only=False, data_root='./data', log_root=tmp, shape=shape,
                            num_labeled=1, pairs=pairs)
    cfg = train_joint.build_config(ns)
    labeled = DeepAtlasExperiment.labeled_subset(4, 1, cfg['random_seed'])
    data = SyntheticRegDataset(4, shape, 32, seed=230, labeled=labeled, pairs=pairs)
    cfg.update(lr_mode='const', samples_per_epoch=len(data), print_batch_period=2)
    cfg['training_data_loader'] = DataLoader(data, batch_size=1, shuffle=False)
    cfg['validation_data_loader'] = DataLoader(SyntheticSegDataset(2, shape, 32, seed=1230), batch_size=1, shuffle=False)
    cfg['validation_pair_loader'] = DataLoader(SyntheticRegDataset(2, shape, 32, seed=1230), batch_size=1, shuffle=False)
    return DeepAtlasExperiment(cfg), data


def test_experiment_with_any_labeled_pairs(tmp_path, monkeypatch):
    """pairs='any_labeled', 4 volumes of which 1 is labelled, deterministic mode: the three pairs with the labelled volume as the MOVING image reach the step with
    seg_t=None and a non-zero supervised term, and two runs from one seed end with bit-equal weights."""
    from deepatlas_amd import ops
    from deepatlas_amd.models import joint
    monkeypatch.chdir(tmp_path)
    calls = []
    inner_call = joint.DeepAtlasJointStep.__call__

    def spy(self, im_m, im_t, seg_m, seg_t):
        out = inner_call(self, im_m, im_t, seg_m, seg_t)
        calls.append((seg_m is None, seg_t is None, float(out['sup'])))
        return out
    monkeypatch.setattr(joint.DeepAtlasJointStep, '__call__', spy)
    prev = ops.set_deterministic(True)
    try:
        a, data = _experiment('a', 'any_labeled')
        assert len(data) == 6 and '_pairsany_labeled' in a.exp_name
        a.train()
        first = list(calls)
        b, _ = _experiment('b', 'any_labeled')
        b.train()
    finally:
        ops.set_deterministic(prev)
    assert len(first) == 6 and sorted(c[:2] for c in first) == [(False, True)] * 3 + [(True, False)] * 3
    assert all(sup > 0.0 for m_none, t_none, sup in first if t_none) and calls[6:] == first
    for ma, mb in ((a.seg_model, b.seg_model), (a.reg_model, b.reg_model)):
        sb = mb.state_dict()
        for k, v in ma.state_dict().items():
            assert torch.equal(v, sb[k]), k


def test_train_joint_command_line_with_all_pairs(tmp_path, monkeypatch):
    import train_joint
    from deepatlas_amd.models import joint
    monkeypatch.chdir(tmp_path)
    kinds = []
    inner_call = joint.DeepAtlasJointStep.__call__
    monkeypatch.setattr(joint.DeepAtlasJointStep, '__call__',
                        lambda self, im_m, im_t, seg_m, seg_t: kinds.append((seg_m is None, seg_t is None)) or inner_call(self, im_m, im_t, seg_m, seg_t))
    res = train_joint.main(['--num-samples', '3', '--num-epochs', '1', '--device', '0', '--shape', '16', '16', '32', '--log-root', 'joint', '--num-labeled', '1',
                            '--pairs', 'all'])
    assert set(res) >= {'seg_dice_avg', 'dice_avg', 'identity_dice_avg', 'nonpos_frac'}
    assert len(kinds) == 6 and sorted(kinds) == [(False, True)] * 2 + [(True, False)] * 2 + [(True, True)] * 2
