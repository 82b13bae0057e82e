"""Train a 3D U-Net: the build's counterpart of the reference's train_seg.py (same flags, same config dict,
train_seg.py:10-93) with its three shipped bugs fixed: the em-dash in '--num-epochs', the
positional './data' / './logs' defaults, and the undefined args.leaf.  Device selection is explicit.  The data
source is the synthetic volume generator, or with --data NAME the reference's NIfTI list-file datasets read without SimpleITK (--data-dir,
--train-list, --valid-list, --test-list) and prepared on the device (--voxel-size, --rescale-percentiles, --normalize, --ignore-labels,
--crop-size).  --patch-size D H W trains on patches cropped on the device and evaluates tile by tile (--patch-mode, --patch-threshold,
--patches-per-volume, --tile-overlap, --tile-batch); --tile-blend / --tile-mirror blend the evaluation tiles' probabilities
(lib/inference.py)."""
import argparse
import os

from deepatlas_amd.models.nifti_data import add_data_arguments, apply_data_arguments
from deepatlas_amd.models.segmentation import SegmentationExperiment


def build_config(args):
    n_classes = 32
    config = dict(
        debug_mode=args.debug,
        resume_dir='',
        random_seed=230,
        data='synthetic',
        n_epochs=args.num_epochs,
        samples_per_epoch=args.num_samples * 2,   # due to flipping data augmentation
        batch_size=1,
        valid_batch_size=1,
        print_batch_period=50,
        valid_epoch_period=1,
        save_ckpts_epoch_period=1,
        model='UNet_light',
        model_settings={'in_channel': 1, 'n_classes': n_classes, 'bias': True, 'BN': True},
        n_classes=n_classes,
        class_name={k: str(k) for k in range(1, n_classes)},
        crop_size=[0, 10, 7, 14, 8, 7],
        loss='dice',
        loss_settings={'n_class': n_classes, 'weight_type': 'Uniform', 'no_bg': False, 'softmax': True, 'eps': 1e-6},
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
    # opt-in device augmentation (lib/transforms.py:161-259), every other argument at the reference's default
    augment = []
    aug_rigid = config.pop('aug_rigid', None)
    aug_bspline = config.pop('aug_bspline', None)
    if aug_rigid:
        augment.append(['rigid', {'rotation_angles': list(aug_rigid[:3]), 'translation': list(aug_rigid[3:])}])
    if aug_bspline is not None:
        augment.append(['bspline', {'deform_scale': aug_bspline}])
    # ... and the intensity half (lib/transforms.py:293-320 and RandomIntensityTransform), after the spatial transforms
    aug_blur = config.pop('aug_blur', None)
    aug_bilateral = config.pop('aug_bilateral', None)
    aug_intensity = config.pop('aug_intensity', False)
    aug_bias = config.pop('aug_bias', None)
    aug_noise = config.pop('aug_noise', None)
    if aug_blur is not None:
        augment.append(['blur', {'variance': aug_blur, 'maximumKernelWidth': 32, 'maximumError': 0.01}])
    if aug_bilateral:
        augment.append(['bilateral', {'domainSigma': aug_bilateral[0], 'rangeSigma': aug_bilateral[1]}])
    if aug_intensity or aug_bias is not None or aug_noise is not None:
        kwargs = {}
        if aug_bias is not None:
            kwargs['bias_scale'] = aug_bias
        if aug_noise is not None:
            kwargs['noise_std'] = [0.0, aug_noise]
        augment.append(['intensity', kwargs])
    if augment:
        config['augment'] = augment
    # opt-in clean-up of the validation / test prediction (lib/evalMetrics.py parse_postprocess); absent = the reference's raw argmax alone
    mode = config.pop('postprocess', None)
    connectivity = config.pop('cc_connectivity', None)
    min_size = config.pop('cc_min_size', None)
    if mode:
        post = {'mode': {'largest-cc': 'largest_cc', 'min-size': 'min_size'}[mode], 'connectivity': connectivity or 6}
        if post['mode'] == 'min_size':
            post['min_size'] = min_size if min_size is not None else 64
        config['postprocess'] = post
    # opt-in surface-distance metrics of the validation / test prediction (lib/evalMetrics.py parse_surface_metrics); absent = Dice alone
    surface = config.pop('surface_metrics', False)
    spacing = config.pop('surface_spacing', None)
    percentile = config.pop('surface_percentile', None)
    if surface or spacing is not None or percentile is not None:
        config['surface_metrics'] = {'spacing': list(spacing) if spacing is not None else [1.0, 1.0, 1.0],
                                     'percentile': percentile if percentile is not None else 95.0}
    # opt-in boundary loss beside the region loss (lib/loss.py BoundaryLoss); absent = the step as it was, and no key in the config
    if config.get('lambda_boundary') is None:
        config.pop('lambda_boundary', None)
    # opt-in patch training and tiled evaluation (models/segmentation.py parse_patch); absent = whole volumes, and no key in the config
    patch_size = config.pop('patch_size', None)
    patch_mode = config.pop('patch_mode', None)
    patch_threshold = config.pop('patch_threshold', None)
    per_volume = config.pop('patches_per_volume', None)
    tile_overlap = config.pop('tile_overlap', None)
    tile_batch = config.pop('tile_batch', None)
    if patch_size is not None:
        config['patch'] = {'size': list(patch_size), 'mode': patch_mode or 'balanced', 'threshold': 0.01 if patch_threshold is None else patch_threshold,
                           'classes': None, 'per_volume': per_volume or 1, 'overlap': list(tile_overlap) if tile_overlap is not None else [8, 8, 8],
                           'tile_batch': tile_batch or 4, 'include_last': False}
    elif any(v is not None for v in (patch_mode, patch_threshold, per_volume, tile_overlap, tile_batch)):
        raise ValueError('--patch-mode, --patch-threshold, --patches-per-volume, --tile-overlap and --tile-batch need --patch-size')
    # opt-in blending of the evaluation tiles (lib/inference.py parse_tile_blend); absent = the core copy, and no key in the config
    tile_blend = config.pop('tile_blend', None)
    tile_mirror = config.pop('tile_mirror', None)
    if tile_blend is not None or tile_mirror is not None:
        if patch_size is None:
            raise ValueError('--tile-blend and --tile-mirror need --patch-size')
        config['tile_blend'] = {'window': tile_blend or 'gaussian', 'sigma_scale': 0.125, 'mirror': list(tile_mirror or '')}
    if not config.get('matrix_precision'):                # (--matrix-precision; not a key of the reference's config: absent = the package default, 'fp32_split')
        config.pop('matrix_precision', None)
    return apply_data_arguments(config)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--device', '-g', default='0', type=str, help='index of used GPU')
    parser.add_argument('--debug', '-d', action='store_true', help='if debug mode')
    parser.add_argument('--preload', '-load', action='store_true', help='if preload data into memory to speed up IO')
    parser.add_argument('--num-samples', '-ns', default=21, type=int, help='number of samples for training')
    parser.add_argument('--num-epochs', '-ne', default=100, type=int, help='number of epochs for training')
    parser.add_argument('--lr', default=1e-3, type=float, help='learning rate')
    parser.add_argument('--test_only', '-t', action='store_true', help='only test model')
    parser.add_argument('--data-root', '-root', default='./data', type=str, help='root of the data folder')
    parser.add_argument('--log-root', '-log', default='./logs', type=str, help='root of the log folders')
    parser.add_argument('--shape', nargs=3, type=int, default=[64, 64, 64], help='synthetic volume size D H W (multiples of 8)')
    parser.add_argument('--matrix-precision', default=None, choices=['fp32', 'fp32_split', 'bf16'],
                        help="arithmetic of the 3x3x3 convolutions: 'fp32_split' (default; what bench.py measures) every fp32 operand scaled per staged "
                             "tile and split into two fp16 terms, three products per multiply on the fp16 matrix pipe: 22-bit products (per-product bound "
                             "7e-7, NARROWER than an fp32 multiply; sums of >= ~100 terms are as close to double as fp32's; elements > 2^15..2^18 below "
                             "their tile's maximum keep only an absolute 2^-40 of it -- csrc/split_f16.h); 'fp32' the fp32 matrix instructions = the "
                             "reference's arithmetic (~1.7x slower steps); 'bf16' operands rounded to bf16")
    parser.add_argument('--aug-rigid', nargs=6, type=float, default=None, metavar=('RX', 'RY', 'RZ', 'TX', 'TY', 'TZ'),
                        help='augment training batches with RandomRigidTransform: rotation_angles (degrees) and translation (voxels), (x, y, z)')
    parser.add_argument('--aug-bspline', type=float, default=None, metavar='DEFORM_SCALE',
                        help='augment training batches with RandomBSplineTransform(deform_scale=DEFORM_SCALE), after the rigid one')
    parser.add_argument('--aug-blur', type=float, default=None, metavar='VARIANCE',
                        help='augment training batches with GaussianBlur(variance=VARIANCE, maximumKernelWidth=32, maximumError=0.01), after the spatial transforms')
    parser.add_argument('--aug-bilateral', nargs=2, type=float, default=None, metavar=('DOMAIN_SIGMA', 'RANGE_SIGMA'),
                        help='augment training batches with BilateralFilter(domainSigma=DOMAIN_SIGMA, rangeSigma=RANGE_SIGMA), after the blur')
    parser.add_argument('--aug-intensity', action='store_true',
                        help='augment training batches with RandomIntensityTransform at its defaults (gamma, gain, noise, clamp), last')
    parser.add_argument('--aug-bias', type=float, default=None, metavar='SCALE',
                        help='bias_scale of --aug-intensity: a smooth multiplicative bias field exp(b), b ~ normal(0, SCALE / 2) on the control grid; implies --aug-intensity')
    parser.add_argument('--aug-noise', type=float, default=None, metavar='STD_MAX',
                        help='upper end of the noise_std range of --aug-intensity (default 0.05); implies --aug-intensity')
    parser.add_argument('--postprocess', default=None, choices=['largest-cc', 'min-size'],
                        help="additionally score the validation / test prediction after a connected-component clean-up on the device: "
                             "'largest-cc' keeps the largest component of every class, 'min-size' drops components below --cc-min-size voxels")
    parser.add_argument('--cc-connectivity', type=int, default=None, choices=[6, 18, 26], help='connectivity of --postprocess (default 6)')
    parser.add_argument('--cc-min-size', type=int, default=None, metavar='VOXELS', help="smallest component --postprocess min-size keeps (default 64)")
    parser.add_argument('--surface-metrics', action='store_true',
                        help='additionally report the Hausdorff percentile (HD95) and the average symmetric surface distance (ASSD) of the '
                             'validation / test prediction, computed on the device (and of the cleaned map with --postprocess)')
    parser.add_argument('--surface-spacing', nargs=3, type=float, default=None, metavar=('SD', 'SH', 'SW'),
                        help='voxel spacing of --surface-metrics (default 1 1 1); implies --surface-metrics')
    parser.add_argument('--surface-percentile', type=float, default=None, metavar='P',
                        help='percentile of the pooled surface distances reported as HD95 (default 95); implies --surface-metrics')
    parser.add_argument('--lambda-boundary', type=float, default=None, metavar='W',
                        help="add W x the boundary loss (Kervadec et al.: softmax probability times the signed distance to the ground truth, the "
                             "distance maps rebuilt on the device from every batch's labels) to the step's loss; 0 or absent: off")
    parser.add_argument('--patch-size', nargs=3, type=int, default=None, metavar=('D', 'H', 'W'),
                        help='train on patches of this size cropped on the device (volumes of different shapes then train together) and evaluate '
                             'every volume tile by tile; multiples of 8 for the U-Nets')
    parser.add_argument('--patch-mode', default=None, choices=['balanced', 'random'],
                        help="'balanced' (default): BalancedRandomCrop's cycle over the classes; 'random': uniform starts")
    parser.add_argument('--patch-threshold', type=float, default=None, metavar='SHARE',
                        help='share of the class a balanced patch must exceed (default 0.01)')
    parser.add_argument('--patches-per-volume', type=int, default=None, metavar='P', help='patches cropped from one loaded volume (default 1); divides the batch size')
    parser.add_argument('--tile-overlap', nargs=3, type=int, default=None, metavar=('D', 'H', 'W'),
                        help='overlap of the evaluation tiles on every side (default 8 8 8); 2 x overlap < patch size')
    parser.add_argument('--tile-batch', type=int, default=None, metavar='T', help='evaluation tiles per forward pass (default 4)')
    parser.add_argument('--tile-blend', default=None, choices=['gaussian', 'constant'],
                        help="blend the evaluation tiles' probabilities under this window instead of copying tile cores (needs --patch-size)")
    parser.add_argument('--tile-mirror', default=None, metavar='AXES',
                        help="also run the evaluation tiles mirrored along these axes, e.g. 'zyx', and average (implies --tile-blend gaussian)")
    add_data_arguments(parser, with_preload=False)              # (--preload is the reference's own flag, above)
    args = parser.parse_args(argv)
    exp = SegmentationExperiment(build_config(args))
    if not args.test_only:
        exp.train()
    exp.test()


if __name__ == '__main__':
    main()
