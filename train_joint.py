"""DeepAtlas joint training of the registration and the segmentation net from few labelled volumes (the reference's stated goal,
listed as TODO in its README.md:15-19).  Flags of train_reg.py plus the four loss weights of models/joint.py DeepAtlasJointStep,
--num-labeled (how many of the training volumes have a manual segmentation), --pairs (which ordered pairs are trained on: those with a
labelled fixed volume, those with a label on either side, or all) and --seg-ckpt / --reg-ckpt (checkpoint files of
train_seg.py / train_reg.py to start from: the DeepAtlas recipe pre-trains each net alone)."""
import argparse
import os

from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
from deepatlas_amd.models.nifti_data import apply_data_arguments
from train_reg import add_common_arguments, apply_jacobian_arguments, apply_similarity_arguments


def build_config(args):
    n_classes = 32
    config = dict(
        debug_mode=args.debug,
        resume_dir='',
        seg_resume_dir='',
        reg_resume_dir='',
        random_seed=230,
        data='synthetic',
        n_epochs=args.num_epochs,
        samples_per_epoch=args.num_samples * max(args.num_samples - 1, 1),
        batch_size=1,
        valid_batch_size=1,
        print_batch_period=50,
        valid_epoch_period=1,
        save_ckpts_epoch_period=1,
        model='UNet_light',
        model_settings={'in_channel': 1, 'n_classes': n_classes, 'bias': True, 'BN': True},
        reg_model='voxel_morph_cvpr',
        reg_model_settings={},
        n_classes=n_classes,
        lambda_sim=1.0,
        lambda_reg=1.0,
        lambda_anat=1.0,
        lambda_sp=1.0,
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
    n_volumes = max(args.num_samples, 2)
    num_labeled = getattr(args, 'num_labeled', None)
    config['num_labeled'] = n_volumes if num_labeled is None else max(0, min(num_labeled, n_volumes))      # clamped to the number of volumes
    config['pairs'] = getattr(args, 'pairs', 'fixed_labeled')
    config['seg_resume_dir'] = config.pop('seg_ckpt', None) or ''
    config['reg_resume_dir'] = config.pop('reg_ckpt', None) or ''
    if not config.get('matrix_precision'):
        config.pop('matrix_precision', None)
    if not config.get('atlas_fusion'):
        config.pop('atlas_fusion', None)
    apply_similarity_arguments(config)
    apply_jacobian_arguments(config)
    return apply_data_arguments(config)


def main(argv=None):
    parser = add_common_arguments(argparse.ArgumentParser())
    parser.add_argument('--lambda-sim', default=1.0, type=float, help='weight of the image similarity (--sim-loss; NCC by default)')
    parser.add_argument('--lambda-anat', default=1.0, type=float, help='weight of the anatomy similarity (Dice of the warped segmentation)')
    parser.add_argument('--lambda-sp', default=1.0, type=float, help='weight of the supervised segmentation loss')
    parser.add_argument('--num-labeled', default=None, type=int, help='number of training volumes with a manual segmentation (default: all)')
    parser.add_argument('--pairs', default='fixed_labeled', choices=['fixed_labeled', 'any_labeled', 'all'],
                        help="pairs trained on: fixed volume labelled (default) | a label on either side (an unlabelled fixed image is trained against the "
                             "warped label of the moving one) | every pair (pairs without any label train the registration net alone)")
    parser.add_argument('--seg-ckpt', default=None, type=str, help='checkpoint file of train_seg.py to start the segmentation net from')
    parser.add_argument('--reg-ckpt', default=None, type=str, help='checkpoint file of train_reg.py to start the registration net from')
    args = parser.parse_args(argv)
    exp = DeepAtlasExperiment(build_config(args))
    if not args.test_only:
        exp.train()
    return exp.test()


if __name__ == '__main__':
    main()
