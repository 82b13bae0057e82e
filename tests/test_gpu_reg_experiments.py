"""GPU: RegistrationExperiment and DeepAtlasExperiment end to end at a small size -- they train, write the checkpoint files and keys they
promise, resume (next epoch, Adam state restored, the step after resume against the uninterrupted run), test() reloads the best file,
the validation numbers equal an independent recomputation from the same nets' outputs (torch-CPU fp64 oracle, tests/regeval_cases.py),
unlabelled moving volumes reach the joint step as seg_m=None, and the two command lines run.  Nothing here asserts that a score improves
with training: toy data, a few steps -- the tests check what is computed, not what is learned."""
import argparse
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import regeval_cases as rc

pytestmark = pytest.mark.gpu

REG_SHAPE = [16, 16, 32]
JOINT_SHAPE = [16, 24, 32]


def _ns(tmp, shape, **kw):
    # (log roots are relative names: the configs prefix them with './', and every test runs inside its tmp_path)
    base = dict(device='0', debug=False, num_samples=3, num_epochs=2, lr=1e-3, test_only=False, data_root='./data', log_root=tmp, shape=list(shape))
    base.update(kw)
    return argparse.Namespace(**base)


def _params(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _max_diff(a, b):
    return max(float((a[k].double() - b[k].double()).abs().max()) for k in a)


def _spy_first_epoch(exp, optimizers):
    """Record (current epoch, per-parameter Adam state) at the moment training starts (after initialize_model / resume)."""
    seen = {}
    inner = exp.train_one_epoch

    def wrapper():
        if not seen:
            seen['epoch'] = exp.current_epoch
            seen['adam'] = [[{k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()} for p in opt.param_groups[0]['params']]
                            for opt in optimizers(exp)]
            seen['steps'] = [opt._steps for opt in optimizers(exp)]
        return inner()
    exp.train_one_epoch = wrapper
    return seen


def _check_adam_restored(seen_adam, seen_steps, ckpt, n_steps):
    saved = ckpt['optimizer_state_dict']
    ids = saved['param_groups'][0]['params']
    assert len(ids) == len(seen_adam) > 0
    assert seen_steps == n_steps
    for i, st in zip(ids, seen_adam):
        ref = saved['state'][i]
        assert float(st['step']) == float(ref['step']) == float(n_steps)
        assert torch.equal(st['exp_avg'], ref['exp_avg'].cpu()) and torch.equal(st['exp_avg_sq'], ref['exp_avg_sq'].cpu())
    assert any(float(saved['state'][i]['exp_avg'].abs().max()) > 0 for i in ids)


def _recompute_registration(model, loader, n_class, device):
    """Independent recomputation of eval_registration's numbers: disp from model(...), scored with the torch-CPU fp64 oracle under the
    exclusion rule.  Returns the oracle's aggregated numbers and checks the device's per-pair Dice against the oracle's per-pair Dice."""
    from deepatlas_amd.lib import evalMetrics as metrics
    dice_o, dice_id, dice_dev, fold_lo, fold_hi, means, stds, bounds = [], [], [], [], [], [], [], []
    with torch.no_grad():
        model.eval()
        for im_m, im_t, seg_m, seg_t, has, _ in loader:
            disp = model(im_m.to(device), im_t.to(device))[0]
            det64, bound, _ = rc.jacobian_bound(disp.cpu())
            flat = det64.reshape(det64.shape[0], -1)
            fold_lo.append((flat <= -bound).mean(1)); fold_hi.append((flat <= bound).mean(1))
            means.append(flat.mean(1)); stds.append(flat.std(1)); bounds.append(bound)
            if not bool(has.all()):
                continue
            want, excluded = rc.nearest_oracle(seg_m, disp.cpu())
            k = int(excluded.sum())
            assert k <= max(rc.MAX_EXCLUDED * excluded.numel(), 1)
            c = rc.counts_np(want.numpy(), seg_t.numpy(), n_class).astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                d = (2.0 * c[..., 2] / (c[..., 0] + c[..., 1]))[:, 1:]
            dev = metrics.registration_dice(seg_m.to(device), seg_t.to(device), disp, n_class)
            # at most k voxels differ: |P & T| and |P| move by at most k each, so Dice = 2 I / (P + T) moves by at most 4 k / (P + T - k)
            denom = (c[..., 0] + c[..., 1])[:, 1:]
            tol = np.where(denom > k, 4.0 * k / np.maximum(denom - k, 1), np.inf)
            both = np.isfinite(d) & np.isfinite(dev)
            assert np.all(np.abs(d - dev)[both] <= tol[both])
            if k == 0:
                assert np.array_equal(d, dev, equal_nan=True)
            dice_o.append(d); dice_dev.append(dev)
            ci = rc.counts_np(seg_m.numpy(), seg_t.numpy(), n_class).astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                dice_id.append((2.0 * ci[..., 2] / (ci[..., 0] + ci[..., 1]))[:, 1:])
    return dict(dice_dev=np.concatenate(dice_dev), dice_id=np.concatenate(dice_id), fold_lo=np.concatenate(fold_lo).mean(), fold_hi=np.concatenate(fold_hi).mean(),
                det_mean=np.concatenate(means).mean(), det_std=np.concatenate(stds).mean(), bound=max(bounds))


def _check_validation_numbers(res, ref):
    from deepatlas_amd.models.registration import _nanmean
    per = _nanmean(ref['dice_dev'], axis=0)
    assert np.array_equal(res['dice_per_class'], per, equal_nan=True)                 # mean over the pairs that have the class
    assert res['dice_avg'] == float(np.nanmean(per))                                  # mean over the classes that occur
    per_id = _nanmean(ref['dice_id'], axis=0)
    assert np.array_equal(res['identity_dice_per_class'], per_id, equal_nan=True)     # disp = 0 is exact: equal to the host count, bit for bit
    assert res['identity_dice_avg'] == float(np.nanmean(per_id))
    assert ref['fold_lo'] - 1e-15 <= res['nonpos_frac'] <= ref['fold_hi'] + 1e-15
    assert abs(res['det_mean'] - ref['det_mean']) <= ref['bound'] and abs(res['det_std'] - ref['det_std']) <= 2 * ref['bound']
    assert 0.0 <= res['dice_avg'] <= 1.0 and res['n_dice_pairs'] == len(ref['dice_dev'])


def _reg_experiment(tmp, n_epochs, resume=''):
    import train_reg
    from deepatlas_amd.lib.datasets import SyntheticRegDataset
    from deepatlas_amd.models.registration import RegistrationExperiment
    cfg = train_reg.build_config(_ns(tmp, REG_SHAPE, num_epochs=n_epochs))
    cfg.update(lr_mode='const', samples_per_epoch=3, resume_dir=resume, print_batch_period=2)
    # a fixed batch order (the default loader shuffles with the global generator, whose state differs between a resumed and an uninterrupted run)
    cfg['training_data_loader'] = DataLoader(SyntheticRegDataset(3, REG_SHAPE, 32, seed=230), batch_size=1, shuffle=False)
    cfg['validation_data_loader'] = DataLoader(SyntheticRegDataset(2, REG_SHAPE, 32, seed=1230), batch_size=1, shuffle=False)
    return RegistrationExperiment(cfg)


def test_registration_experiment_trains_checkpoints_resumes_and_validates(tmp_path, monkeypatch):
    """Determinism at this size (16 x 16 x 32, deterministic mode): the test first compares two uninterrupted runs from the same seed and
    holds the step after resume to whatever they show -- bit-equality when they are bit-equal, their spread otherwise -- and prints
    which case held.  On an MI355X the bit-equal case held, here and in the joint test below: the two uninterrupted runs differ by 0, and
    so does the resumed run from the uninterrupted one."""
    from deepatlas_amd import ops
    monkeypatch.chdir(tmp_path)
    ops.set_deterministic(True)
    a = _reg_experiment('a', 2)
    a.train()
    pa = _params(a.model)
    ck_dir = a.ckpoint_dir
    assert {'checkpoint.pth.tar', 'model_best.pth.tar', 'train_config.json'} <= set(os.listdir(ck_dir))
    assert os.path.realpath(ck_dir).startswith(os.path.realpath(str(tmp_path)))
    for f in ('checkpoint.pth.tar', 'model_best.pth.tar'):
        ck = torch.load(os.path.join(ck_dir, f), map_location='cpu')
        assert set(ck) == {'epoch', 'model_state_dict', 'optimizer_state_dict', 'best_score'}, f
    assert torch.load(os.path.join(ck_dir, 'checkpoint.pth.tar'), map_location='cpu')['epoch'] == 2
    # the validation numbers of the last epoch = an independent recomputation from the same net's outputs
    _check_validation_numbers(a.last_validation, _recompute_registration(a.model, a.validation_data_loader, 32, a.device))
    assert a.last_validation['n_pairs'] == 2

    ops.set_deterministic(True)
    a2 = _reg_experiment('a2', 2)
    a2.train()
    spread = _max_diff(pa, _params(a2.model))

    ops.set_deterministic(True)
    b1 = _reg_experiment('b', 1)
    b1.train()
    ck_file = os.path.join(b1.ckpoint_dir, 'checkpoint.pth.tar')
    ck = torch.load(ck_file, map_location='cpu')
    assert ck['epoch'] == 1
    ops.set_deterministic(True)
    b2 = _reg_experiment('b', 2, resume=ck_file)
    seen = _spy_first_epoch(b2, lambda e: [e.optimizer])
    b2.train()
    assert seen['epoch'] == 2                                                     # continues at the next epoch
    _check_adam_restored(seen['adam'][0], seen['steps'][0], ck, n_steps=3)
    resumed = _max_diff(pa, _params(b2.model))
    print('registration: two uninterrupted runs differ by %.3e (%s), resumed run differs from the uninterrupted one by %.3e'
          % (spread, 'bit-equal' if spread == 0.0 else 'not bit-equal', resumed))
    assert resumed <= spread                                                      # spread == 0: bit-equal after resume
    assert torch.load(os.path.join(b2.ckpoint_dir, 'checkpoint.pth.tar'), map_location='cpu')['epoch'] == 2

    # test() reloads the best file
    best = torch.load(os.path.join(ck_dir, 'model_best.pth.tar'), map_location='cpu')
    res = a.test()
    for k, v in a.model.state_dict().items():
        assert torch.equal(v.cpu(), best['model_state_dict'][k]), k
    _check_validation_numbers(res, _recompute_registration(a.model, a.validation_data_loader, 32, a.device))
    assert best['best_score'] == a.best_score


def _joint_experiment(tmp, n_epochs, resume='', num_labeled=2):
    import train_joint
    from deepatlas_amd.lib.datasets import SyntheticRegDataset, SyntheticSegDataset
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    cfg = train_joint.build_config(_ns(tmp, JOINT_SHAPE, num_epochs=n_epochs, num_labeled=num_labeled))
    labeled = DeepAtlasExperiment.labeled_subset(3, num_labeled, cfg['random_seed'])
    data = SyntheticRegDataset(3, JOINT_SHAPE, 32, seed=230, labeled=labeled)
    cfg.update(lr_mode='const', samples_per_epoch=len(data), resume_dir=resume, print_batch_period=2)
    cfg['training_data_loader'] = DataLoader(data, batch_size=1, shuffle=False)
    cfg['validation_data_loader'] = DataLoader(SyntheticSegDataset(2, JOINT_SHAPE, 32, seed=1230), batch_size=1, shuffle=False)
    cfg['validation_pair_loader'] = DataLoader(SyntheticRegDataset(2, JOINT_SHAPE, 32, seed=1230), batch_size=1, shuffle=False)
    return DeepAtlasExperiment(cfg), data


def test_deepatlas_experiment_trains_checkpoints_resumes_and_validates(tmp_path, monkeypatch):
    """As the registration test, for the joint experiment (16 x 24 x 32, 3 volumes of which 2 are labelled): both nets and both
    optimisers are saved and restored, unlabelled moving volumes really reach the step as seg_m=None."""
    from deepatlas_amd import ops
    from deepatlas_amd.models import joint
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    monkeypatch.chdir(tmp_path)
    calls = []
    inner_call = joint.DeepAtlasJointStep.__call__

    def spy(self, im_m, im_t, seg_m, seg_t):
        out = inner_call(self, im_m, im_t, seg_m, seg_t)
        calls.append((seg_m is None, float(out['sup'])))
        return out
    monkeypatch.setattr(joint.DeepAtlasJointStep, '__call__', spy)

    ops.set_deterministic(True)
    a, data = _joint_experiment('a', 2)
    n_unlabelled = sum(1 for i in range(len(data)) if not data[i][4])
    assert len(data) == 4 and n_unlabelled == 2
    outs = []
    inner_step = a.train_step
    a.train_step = lambda batch: outs.append((bool(batch[4].all()), inner_step(batch))) or outs[-1][1]
    a.train()
    # seg_m=None steps really occur, and their loss dict has no supervised term
    assert len(calls) == 8 and sum(1 for none, _ in calls if none) == 2 * n_unlabelled
    assert all(sup == 0.0 for none, sup in calls if none) and all(sup > 0.0 for none, sup in calls if not none)
    assert len(outs) == 8
    for labelled, out in outs:
        assert ('sup' in out) == labelled
        assert {'loss_reg', 'loss_seg', 'sim', 'bend', 'anat_reg', 'anat_seg'} <= set(out)
    pa = {'seg': _params(a.seg_model), 'reg': _params(a.reg_model)}
    files = sorted(f for f in os.listdir(a.ckpoint_dir) if f.endswith('.pth.tar'))
    assert files == ['reg_checkpoint.pth.tar', 'reg_model_best.pth.tar', 'seg_checkpoint.pth.tar', 'seg_model_best.pth.tar']
    for net in ('seg', 'reg'):
        for f in ('checkpoint.pth.tar', 'model_best.pth.tar'):
            ck = torch.load(os.path.join(a.ckpoint_dir, net + '_' + f), map_location='cpu')
            assert set(ck) == {'epoch', 'model_state_dict', 'optimizer_state_dict', net + '_best_score'}, (net, f)
    # validation: segmentation Dice exactly as SegmentationExperiment.eval computes it, registration numbers against the oracle
    res = a.last_validation

    class View(object):
        model, config, device = a.seg_model, a.config, a.device
    per_class, avg, _ = SegmentationExperiment.eval(View(), a.validation_data_loader)
    assert torch.equal(res['seg_dice_per_class'], per_class) and res['seg_dice_avg'] == float(avg)
    _check_validation_numbers(res, _recompute_registration(a.reg_model, a.validation_pair_loader, 32, a.device))

    ops.set_deterministic(True)
    a2, _ = _joint_experiment('a2', 2)
    a2.train()
    spread = max(_max_diff(pa['seg'], _params(a2.seg_model)), _max_diff(pa['reg'], _params(a2.reg_model)))

    ops.set_deterministic(True)
    b1, _ = _joint_experiment('b', 1)
    b1.train()
    cks = {net: torch.load(os.path.join(b1.ckpoint_dir, net + '_checkpoint.pth.tar'), map_location='cpu') for net in ('seg', 'reg')}
    assert cks['seg']['epoch'] == cks['reg']['epoch'] == 1
    ops.set_deterministic(True)
    b2, _ = _joint_experiment('b', 2, resume=b1.ckpoint_dir)
    seen = _spy_first_epoch(b2, lambda e: [e.seg_optimizer, e.reg_optimizer])
    b2.train()
    assert seen['epoch'] == 2
    _check_adam_restored(seen['adam'][0], seen['steps'][0], cks['seg'], n_steps=4)
    _check_adam_restored(seen['adam'][1], seen['steps'][1], cks['reg'], n_steps=4)
    resumed = max(_max_diff(pa['seg'], _params(b2.seg_model)), _max_diff(pa['reg'], _params(b2.reg_model)))
    print('joint: two uninterrupted runs differ by %.3e (%s), resumed run differs from the uninterrupted one by %.3e'
          % (spread, 'bit-equal' if spread == 0.0 else 'not bit-equal', resumed))
    assert resumed <= spread

    # test() reloads the two best files
    best = {net: torch.load(os.path.join(a.ckpoint_dir, net + '_model_best.pth.tar'), map_location='cpu') for net in ('seg', 'reg')}
    res = a.test()
    for net, model in (('seg', a.seg_model), ('reg', a.reg_model)):
        for k, v in model.state_dict().items():
            assert torch.equal(v.cpu(), best[net]['model_state_dict'][k]), (net, k)
    _check_validation_numbers(res, _recompute_registration(a.reg_model, a.validation_pair_loader, 32, a.device))


def test_joint_warm_start_from_pretrained_checkpoints(tmp_path, monkeypatch):
    """The DeepAtlas recipe: each net pre-trained alone; the joint experiment starts from those weights (epoch counter at 1)."""
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    monkeypatch.chdir(tmp_path)
    reg = _reg_experiment('reg', 1)
    reg.train()
    ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                            data_root='./data', log_root='seg', shape=JOINT_SHAPE)
    seg = SegmentationExperiment(train_seg.build_config(ns))
    seg.train()
    exp, _ = _joint_experiment('joint', 1, num_labeled=3)
    exp.config['seg_resume_dir'] = os.path.join(seg.ckpoint_dir, 'checkpoint.pth.tar')
    exp.config['reg_resume_dir'] = os.path.join(reg.ckpoint_dir, 'checkpoint.pth.tar')
    exp.setup_train()
    assert exp.initialize_models() == 0
    for model, ref in ((exp.seg_model, seg.model), (exp.reg_model, reg.model)):
        want = ref.state_dict()
        for k, v in model.state_dict().items():
            assert torch.equal(v, want[k]), k
    assert exp.seg_optimizer._steps == 0 and exp.reg_optimizer._steps == 0


def test_train_reg_and_train_joint_command_lines(tmp_path, monkeypatch):
    import train_joint
    import train_reg
    monkeypatch.chdir(tmp_path)
    common = ['--num-samples', '3', '--num-epochs', '1', '--device', '0']
    res = train_reg.main(common + ['--shape'] + [str(s) for s in REG_SHAPE] + ['--log-root', 'reg', '--lambda-reg', '0.5'])
    assert set(res) >= {'dice_per_class', 'dice_avg', 'identity_dice_avg', 'nonpos_frac', 'det_mean', 'det_std'}
    res = train_joint.main(common + ['--shape'] + [str(s) for s in JOINT_SHAPE] + ['--log-root', 'joint', '--num-labeled', '2',
                                                                                 '--lambda-anat', '0.5'])
    assert set(res) >= {'seg_dice_avg', 'seg_dice_per_class', 'dice_avg', 'identity_dice_avg', 'nonpos_frac'}
    found = [f for _, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith('.pth.tar')]
    assert sorted(found) == ['checkpoint.pth.tar', 'model_best.pth.tar', 'reg_checkpoint.pth.tar', 'reg_model_best.pth.tar',
                             'seg_checkpoint.pth.tar', 'seg_model_best.pth.tar']
