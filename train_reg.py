"""Train the registration net (VoxelMorph) alone: the registration counterpart of train_seg.py, which the reference lists as TODO
(README.md:15-19).  Same flag style as train_seg.py; the step is similarity + lambda_reg * bending energy (models/joint.py RegistrationStep;
--sim-loss ncc | lncc | mi, NCC by default), the data are ordered pairs of synthetic volumes (--moving-remap: the moving image in another
"modality") or, with --data NAME, of the NIfTI volumes of a list file (the flags of train_seg.py; --misalign and --report-tre stay
synthetic-only), validation reports the hard-label registration Dice (against the identity deformation's) and the Jacobian statistics of the
predicted deformation.  --lambda-jac > 0 adds the Jacobian folding penalty (--jac-eps, --jac-power) to the step: it trains against the
folding fraction that validation prints.  --lambda-ic > 0 adds the inverse-consistency penalty: the step predicts both directions of every pair
in one doubled-batch forward and penalises the composition of the two fields; validation then (or with --report-ic alone) also prints the
inverse-consistency error in voxels.  --affine-init rigid | affine pre-aligns every pair's moving image to the fixed one (lib/affine.py
affine_register: a coarse-to-fine Adam on 6 or 12 parameters through the fused affine warp kernels) before the net sees it, in training and in
validation, where the affine and the predicted field are composed into one field; --misalign ROT_DEG TRANS_VOX gives the synthetic pairs the
global misalignment that stage is for."""
import argparse
import os

from deepatlas_amd.models.nifti_data import add_data_arguments, apply_data_arguments
from deepatlas_amd.models.registration import RegistrationExperiment


def build_config(args):
    n_classes = 32
    config = dict(
        debug_mode=args.debug,
        resume_dir='',
        random_seed=230,
        data='synthetic',
        n_epochs=args.num_epochs,
        samples_per_epoch=args.num_samples * max(args.num_samples - 1, 1),    # every ordered pair once
        batch_size=1,
        valid_batch_size=1,
        print_batch_period=50,
        valid_epoch_period=1,
        save_ckpts_epoch_period=1,
        model='voxel_morph_cvpr',
        model_settings={},
        n_classes=n_classes,
        lambda_reg=1.0,
        learning_rate=1e-3,
        lr_mode='multiStep',
        milestones=[0.5, 1],
        gamma=0.2,
    )
    config.update(args.__dict__)
    config['learning_rate'] = args.lr
    config['synthetic_shape'] = tuple(args.shape)
    config['data_dir'] = os.path.join(args.data_root, "synthetic")
    config['valid_data_dir'] = config['data_dir']
    config['log_dir'] = './{}/{}'.format(args.log_root, config['data'])
    config['device'] = 'cuda:{}'.format(args.device) if args.device.isdigit() else args.device
    if not config.get('matrix_precision'):                # absent = the package default, 'fp32_split'
        config.pop('matrix_precision', None)
    if not config.get('atlas_fusion'):                    # absent = no registration-based segmentation at validation
        config.pop('atlas_fusion', None)
    apply_similarity_arguments(config)
    apply_jacobian_arguments(config)
    apply_inverse_consistency_arguments(config)
    apply_affine_arguments(config)
    apply_tre_arguments(config)
    apply_refine_arguments(config)
    return apply_data_arguments(config)


def apply_refine_arguments(config):
    """--refine-eval ITERS -> config['refine'] = ITERS; an absent flag leaves no key, so a run without it has the config it always had."""
    iters = config.pop('refine_eval', None)
    if iters is not None:
        config['refine'] = int(iters)
    return config


def apply_tre_arguments(config):
    """--report-tre AMP_VOX -> config['report_tre'] = {'amp_vox': AMP_VOX}; an absent flag leaves no key, so a run without it has the config it
    always had."""
    amp = config.pop('report_tre', None)
    if amp is not None:
        config['report_tre'] = {'amp_vox': float(amp)}
    return config


def apply_affine_arguments(config):
    """--affine-init / --affine-iters / --misalign -> config['affine_init'], config['affine_settings']['iters'], config['misalign']; an absent
    flag leaves no key, so a run without them has the config it always had."""
    mode = config.pop('affine_init', None)
    iters = config.pop('affine_iters', None)
    mis = config.pop('misalign', None)
    if mode:
        config['affine_init'] = mode
    if iters is not None:
        config['affine_settings'] = dict(config.get('affine_settings') or {}, iters=tuple(int(k) for k in iters))
    if mis is not None:
        config['misalign'] = tuple(float(v) for v in mis)
    return config


def apply_inverse_consistency_arguments(config):
    """--lambda-ic / --report-ic -> config['lambda_ic'] and config['report_ic']; an absent flag leaves no key (no penalty; the report follows the
    penalty), so a run without them has the config it always had."""
    lam = float(config.pop('lambda_ic', None) or 0.0)
    if lam != 0.0:
        config['lambda_ic'] = lam
    if config.pop('report_ic', None):
        config['report_ic'] = True
    return config


def apply_jacobian_arguments(config):
    """--lambda-jac / --jac-eps / --jac-power -> config['lambda_jac'] (0 when the flag is absent: no penalty) and config['jac_settings']."""
    config['lambda_jac'] = float(config.get('lambda_jac') or 0.0)
    settings = dict(config.get('jac_settings') or {})
    for flag, key in (('jac_eps', 'eps'), ('jac_power', 'power')):
        value = config.pop(flag, None)
        if value is not None:
            settings[key] = value
    config['jac_settings'] = settings
    return config


def apply_similarity_arguments(config):
    """--sim-loss / --mi-bins / --moving-remap -> config['sim_loss'] (always present, 'ncc' when the flag is absent), config['sim_settings'],
    config['moving_remap'] (absent = both images of a pair in the same modality)."""
    config['sim_loss'] = config.get('sim_loss') or 'ncc'
    bins = config.pop('mi_bins', None)
    settings = dict(config.get('sim_settings') or {})
    if config['sim_loss'] == 'mi' and bins is not None:
        settings['num_bins'] = int(bins)
    config['sim_settings'] = settings
    if not config.get('moving_remap'):
        config.pop('moving_remap', None)
    return config


def add_common_arguments(parser):
    parser.add_argument('--device', '-g', default='0', type=str, help='index of used GPU')
    parser.add_argument('--debug', '-d', action='store_true', help='if debug mode')
    parser.add_argument('--num-samples', '-ns', default=21, type=int, help='number of volumes for training (pairs: n (n - 1))')
    parser.add_argument('--num-epochs', '-ne', default=100, type=int, help='number of epochs for training')
    parser.add_argument('--lr', default=1e-3, type=float, help='learning rate')
    parser.add_argument('--test_only', '-t', action='store_true', help='only test model')
    parser.add_argument('--data-root', '-root', default='./data', type=str, help='root of the data folder')
    parser.add_argument('--log-root', '-log', default='./logs', type=str, help='root of the log folders')
    parser.add_argument('--shape', nargs=3, type=int, default=[64, 64, 64], help='synthetic volume size D H W (multiples of 16)')
    parser.add_argument('--matrix-precision', default=None, choices=['fp32', 'fp32_split', 'bf16'],
                        help="arithmetic of the 3x3x3 convolutions, as in train_seg.py ('fp32_split' when absent)")
    parser.add_argument('--lambda-reg', default=1.0, type=float, help='weight of the bending-energy regulariser')
    parser.add_argument('--atlas-fusion', default=None, choices=['majority', 'local'],
                        help="also validate the registration net as a segmenter: every validation volume is segmented from the labelled "
                             "training volumes (at most 5) by multi-atlas label fusion, majority vote or locally weighted voting")
    parser.add_argument('--sim-loss', default='ncc', choices=['ncc', 'lncc', 'mi'],
                        help="image similarity of the registration step: global NCC (default), local NCC over 9^3 windows, or mutual information "
                             "(for pairs whose intensities are not linearly related)")
    parser.add_argument('--mi-bins', default=None, type=int, help='intensity bins of --sim-loss mi (2..32, default 32)')
    parser.add_argument('--moving-remap', default=None, choices=['invert', 'fold'],
                        help="synthetic multi-modal pairs: the moving image is shown as 1 - x ('invert') or |2 x - 1| ('fold'); labels are untouched")
    parser.add_argument('--lambda-jac', default=0.0, type=float,
                        help='weight of the Jacobian folding penalty mean(max(0, eps - det J)^power) of the predicted deformation (0: off)')
    parser.add_argument('--jac-eps', default=None, type=float, help='margin of --lambda-jac: voxels with det J < eps are penalised (0..1, default 0)')
    parser.add_argument('--jac-power', default=None, type=int, choices=[1, 2], help='exponent of --lambda-jac (default 1)')
    return add_data_arguments(parser)


def add_inverse_consistency_arguments(parser):
    """The flags of the registration experiment alone (the joint step has no inverse-consistency term: train a net here and pass it on as --reg-ckpt)."""
    parser.add_argument('--lambda-ic', default=0.0, type=float,
                        help='weight of the inverse-consistency penalty: mean |u_ab(x) + u_ba(x + u_ab(x))|^2 in voxels^2, both directions (0: off)')
    parser.add_argument('--report-ic', action='store_true',
                        help='validation also runs the reverse direction and prints the inverse-consistency error in voxels (implied by --lambda-ic > 0)')
    return parser


def add_affine_arguments(parser):
    """The affine pre-alignment stage and the synthetic misalignment it is for (registration experiment only; not with --lambda-ic)."""
    parser.add_argument('--affine-init', default=None, choices=['rigid', 'affine'],
                        help="pre-align every pair's moving image to the fixed image before the net sees it: 6-parameter rigid or 12-parameter "
                             "affine, coarse to fine (pooling 4, 2, 1) by Adam on the image similarity; validation composes the affine with the "
                             "predicted field and also prints the Dice of the affine alone")
    parser.add_argument('--affine-iters', default=None, type=int, nargs=3, metavar=('I4', 'I2', 'I1'),
                        help='Adam iterations of --affine-init on the three pyramid levels (default 60 40 20)')
    parser.add_argument('--misalign', default=None, type=float, nargs=2, metavar=('ROT_DEG', 'TRANS_VOX'),
                        help="give every pair's moving image and segmentation a rigid misalignment, in training and validation alike: per axis a "
                             "rotation ~ N(0, ROT_DEG / 2) degrees and a translation ~ N(0, TRANS_VOX / 2) voxels, seeded by the pair's name (the "
                             "same in every epoch).  The resample fills the image with 0.1 outside the volume (labels: 0)")
    return parser


def add_tre_arguments(parser):
    """The known-deformation probe of the registration experiment's validation (not with --affine-init)."""
    parser.add_argument('--report-tre', default=None, type=float, metavar='AMP_VOX',
                        help="validation also deforms every fixed image by a known smooth field of at most AMP_VOX voxels, registers it back and "
                             "prints the landmark error in voxels against the exact inverse of that field (one more net forward per pair)")
    return parser


def add_refine_arguments(parser):
    """Instance refinement at validation (registration experiment only)."""
    parser.add_argument('--refine-eval', default=None, type=int, metavar='ITERS',
                        help="validation also refines every pair's field on that pair by ITERS Adam iterations on the similarity under the training "
                             "regulariser (lib/refine.py) and prints the refined Dice and folding fraction; model selection stays on the net's own field")
    return parser


def main(argv=None):
    args = add_refine_arguments(add_tre_arguments(add_affine_arguments(add_inverse_consistency_arguments(add_common_arguments(argparse.ArgumentParser()))))).parse_args(argv)
    exp = RegistrationExperiment(build_config(args))
    if not args.test_only:
        exp.train()
    return exp.test()


if __name__ == '__main__':
    main()
