"""CPU: the plumbing of the instance refinement that needs no device -- the step per channel, the settings a config or a command line leads to, the
flags of predict_reg.py and train_reg.py, the printed lines, and that a run without the flags and keys has the config, the name and the lines it always
had."""
import argparse

import pytest

import train_joint
import train_reg
import predict_reg
from deepatlas_amd import ops
from deepatlas_amd.lib import refine as R
from deepatlas_amd.models.registration import RegistrationExperiment, check_refine, refine_text, refuse_refine


def _ns(**kw):
    base = dict(device='0', debug=False, num_samples=4, num_epochs=3, lr=1e-3, test_only=False, data_root='./data', log_root='./logs', shape=[16, 16, 32])
    base.update(kw)
    return argparse.Namespace(**base)


def test_lr3_is_the_same_distance_on_every_axis():
    assert ops.refine_lr3(0.1, (80, 96, 80)) == (0.1 * 2 / 79, 0.1 * 2 / 95, 0.1 * 2 / 79)          # (x, y, z) = (W, H, D)
    assert ops.refine_lr3(0.5, (3, 5, 9)) == (0.5 * 2 / 8, 0.5 * 2 / 4, 0.5 * 2 / 2)
    assert ops.refine_lr3(0.1, (1, 9, 40)) == (0.1 * 2 / 39, 0.1 * 2 / 8, 0.0)                      # nothing moves along an extent of 1
    for size in ((80, 96, 80), (3, 5, 9)):                                                         # a step is lr_vox voxels: lr3 x (extent - 1) / 2
        lr3 = ops.refine_lr3(0.25, size)
        assert all(abs(lr3[c] * (e - 1) / 2 - 0.25) < 1e-15 for c, e in enumerate((size[2], size[1], size[0])))


def test_settings_from_config():
    cfg = {'lambda_reg': 2.5, 'sim_loss': 'ncc', 'sim_settings': {}}
    assert R.settings_from_config(cfg, None) is None
    assert R.settings_from_config(cfg, 30) == {'iters': 30, 'lambda_reg': 2.5, 'sim': 'ncc', 'fused': True}
    assert R.settings_from_config(cfg, {'iters': 7, 'lambda_reg': 0.0, 'lr_vox': 0.2}) == {'iters': 7, 'lambda_reg': 0.0, 'lr_vox': 0.2, 'sim': 'ncc', 'fused': True}
    mi = {'lambda_reg': 1.0, 'sim_loss': 'mi', 'sim_settings': {'num_bins': 16}}
    assert R.settings_from_config(mi, 5) == {'iters': 5, 'lambda_reg': 1.0, 'sim': 'mi', 'sim_settings': {'num_bins': 16}, 'fused': False}
    assert R.settings_from_config(mi, {'iters': 5, 'sim': 'ncc'})['fused'] is True and 'sim_settings' not in R.settings_from_config(mi, {'iters': 5, 'sim': 'ncc'})
    assert R.settings_from_config({}, 3) == {'iters': 3, 'lambda_reg': 1.0, 'sim': 'ncc', 'fused': True}                  # a config written before the keys
    assert R.settings_from_config(cfg, {'iters': 3, 'lambda_jac': 0.5})['fused'] is False
    for bad in (True, 2.5, 'ten', {'iters': -1}, {'iters': 3, 'steps': 2}, {'iters': 3, 'lr_vox': float('nan')}, {'iters': 3, 'sim': 'ssd'},
                {'iters': 3, 'sim': 'mi', 'fused': True}, {'iters': 3, 'lambda_jac': 0.1, 'fused': True}):
        with pytest.raises(ValueError):
            R.settings_from_config(cfg, bad)
    with pytest.raises(ValueError, match="supports sim = 'ncc'"):
        R.check_settings(sim='lncc', fused=True)


def test_train_reg_flag_and_config_key():
    parser = train_reg.add_refine_arguments(train_reg.add_tre_arguments(train_reg.add_affine_arguments(train_reg.add_inverse_consistency_arguments(
        train_reg.add_common_arguments(argparse.ArgumentParser())))))
    c0 = train_reg.build_config(parser.parse_args([]))
    assert 'refine' not in c0 and 'refine_eval' not in c0 and check_refine(c0) is None
    assert c0 == train_reg.build_config(train_reg.add_tre_arguments(train_reg.add_affine_arguments(train_reg.add_inverse_consistency_arguments(
        train_reg.add_common_arguments(argparse.ArgumentParser())))).parse_args([]))                          # the config a run without the flag always had
    c1 = train_reg.build_config(parser.parse_args(['--refine-eval', '20', '--lambda-reg', '0.5']))
    assert c1['refine'] == 20 and 'refine_eval' not in c1
    assert check_refine(c1) == {'iters': 20, 'lambda_reg': 0.5, 'sim': 'ncc', 'fused': True}
    assert RegistrationExperiment.experiment_name(c1) == RegistrationExperiment.experiment_name(dict(c1, refine=None))     # no part in the name
    assert {k: v for k, v in c1.items() if k != 'refine'} == train_reg.build_config(parser.parse_args(['--lambda-reg', '0.5']))
    with pytest.raises(ValueError):
        check_refine(dict(c0, refine={'iters': 3, 'sim': 'mi', 'fused': True}))
    assert refine_text({'dice_avg': 0.5}) == ''
    assert refine_text({'refined_dice_avg': 0.61234, 'refined_fold_frac': 0.00123}) == ', refined Dice 0.6123 (folding 0.0012)'


def test_joint_experiment_refuses_the_key():
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    cfg = train_joint.build_config(_ns(num_labeled=4, pairs='fixed_labeled'))
    refuse_refine(cfg, 'joint')                                                   # absent: nothing
    refuse_refine(dict(cfg, refine=None), 'joint')
    cfg['refine'] = 5
    with pytest.raises(ValueError, match=r"config\['refine'\] is not supported by the joint experiment"):
        DeepAtlasExperiment(cfg)


def test_predict_reg_flags():
    p = predict_reg.build_parser()
    base = ['--ckpt', 'c', '--output-dir', 'o', '--moving', 'a', '--fixed', 'b']
    cfg = {'lambda_reg': 2.0, 'sim_loss': 'lncc', 'sim_settings': {'filter_size': 5}}
    assert predict_reg.refine_settings(p.parse_args(base), cfg) is None
    got = predict_reg.refine_settings(p.parse_args(base + ['--refine', '40']), cfg)
    assert got == {'iters': 40, 'lambda_reg': 2.0, 'sim': 'lncc', 'sim_settings': {'filter_size': 5}, 'fused': False}         # the checkpoint's regulariser and similarity
    got = predict_reg.refine_settings(p.parse_args(base + ['--refine', '40', '--refine-lr', '0.05', '--refine-lambda-reg', '0.1', '--refine-sim', 'ncc']), cfg)
    assert got == {'iters': 40, 'lr_vox': 0.05, 'lambda_reg': 0.1, 'sim': 'ncc', 'fused': True}
    for flags in (['--refine-lr', '0.05'], ['--refine-lambda-reg', '1'], ['--refine-sim', 'mi']):
        with pytest.raises(ValueError, match='go with --refine'):
            predict_reg.refine_settings(p.parse_args(base + flags), cfg)
    with pytest.raises(ValueError):
        predict_reg.refine_settings(p.parse_args(base + ['--refine', '-2']), cfg)
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--refine', '5', '--refine-sim', 'ssd'])


def test_printed_lines():
    assert predict_reg.format_refine(0.31234, 0.12, 50) == 'refine: 1-NCC 0.3123 -> 0.1200 (50 iterations)'
    jac = {'mean': 1.0, 'std': 0.25, 'folds': 3}
    assert predict_reg.format_pair('a_to_b', jac) == 'a_to_b: det J mean 1.0000 std 0.2500 folds 3'                      # without the flag: the lines it always printed
    assert predict_reg.format_pair('a_to_b', jac, 0.5, 0.25) == 'a_to_b: Dice Avg: 0.500000 (identity 0.250000), det J mean 1.0000 std 0.2500 folds 3'
    assert predict_reg.format_pair('a_to_b', jac, 0.5, 0.25, 0.4) == 'a_to_b: Dice Avg: 0.500000 (identity 0.250000, unrefined 0.400000), det J mean 1.0000 std 0.2500 folds 3'
