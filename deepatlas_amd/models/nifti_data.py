"""Loaders of the experiments for config['data'] != 'synthetic': the reference's list-file datasets (models/segmentation.py:54-79, 241-251) over
lib/datasets.py's NIfTI classes.  Config keys are the reference's: data, data_dir, valid_data_dir, training_list_file, validation_list_file,
testing_list_file, preload, crop_size, num_samples.  config['preprocess'] (optional, the project's own) prepends transforms of
lib/transforms.py ahead of SitkToTensor: [['resample', {...}], ['percentile_rescale', {...}], ['normalize', {}], ['left_to_right', {}],
['label_filter', {...}]], the form of config['augment'].
"""
from ..lib import datasets as med_data
from ..lib import transforms as med_transforms


def is_nifti(cfg):
    return cfg.get('data', 'synthetic') != 'synthetic'


def refuse_synthetic_only(cfg, keys):
    """Options that are defined on the synthetic volumes alone raise with NIfTI data."""
    for k in keys:
        if is_nifti(cfg) and cfg.get(k) is not None:
            raise ValueError("config[%r] is synthetic-only: it does not go with config['data'] = %r (NIfTI volumes)" % (k, cfg['data']))


def pre_transform(cfg):
    """Compose([*preprocess, SitkToTensor(), CropTensor(crop_size) if crop_size]), as models/segmentation.py:57-64."""
    steps = med_transforms.make_preprocess(cfg.get('preprocess')) + [med_transforms.SitkToTensor()]
    if cfg.get('crop_size'):
        steps.append(med_transforms.CropTensor(cfg['crop_size']))
    return med_transforms.Compose(steps)


def seg_dataset(cfg, list_key, dir_key, n_samples=None):
    """The volume dataset of one list file of the config; None when the config has no such list."""
    if not cfg.get(list_key):
        return None
    data_dir = cfg.get(dir_key) or cfg['data_dir']
    return med_data.get_seg_dataset(cfg['data'])(cfg[list_key], data_dir, with_seg=True, preload=bool(cfg.get('preload')),
                                                 pre_transform=pre_transform(cfg), n_samples=n_samples)


def shape_multiple(model_name):
    """Every extent of a volume must be a multiple of this for the net to accept it: 8 for the U-Nets (three 2x poolings whose skip connections
    are concatenated with the up-sampled path), 1 for VoxelMorph (it up-samples to the skip's own size)."""
    return 8 if str(model_name).startswith('UNet') else 1


def check_patch(patch, models):
    """The patch geometry every net of `models` accepts: extents that are multiples of shape_multiple(model), 2 * overlap < size per axis."""
    size, overlap = [int(v) for v in patch['size']], [int(v) for v in patch.get('overlap') or (0, 0, 0)]
    text = 'x'.join(str(v) for v in size)
    for m in models:
        k = shape_multiple(m)
        if any(v % k for v in size) or min(size) < 1:
            raise ValueError('%s takes patches whose extents are multiples of %d: patch %s' % (m, k, text))
    if any(o < 0 or 2 * o >= v for o, v in zip(overlap, size)):
        raise ValueError('the tile overlap %s must satisfy 0 <= 2 * overlap < size on every axis of patch %s' % ('x'.join(str(o) for o in overlap), text))
    return tuple(size)


def check_shapes(datasets, models, patch=None):
    """Raise ValueError, listing names and shapes, unless every prepared volume of `datasets` has one common shape that every net of `models`
    accepts.  Runs at setup (a dataset that is not preloaded reads every volume once here) so that a bad volume does not surface later
    inside collation or a kernel.
    With `patch` (the experiment's config['patch']: 'size' and 'overlap', (z, y, x)) the volumes may differ in shape: the nets see patches.
    Then every extent of every volume must be >= the patch's, the patch's extents multiples of shape_multiple(model) and 2 * overlap < size;
    returns the patch size."""
    found = []
    for ds in datasets:
        if ds is None:
            continue
        for i in range(len(ds)):
            image, _, name = ds[i]
            found.append((name, tuple(int(s) for s in image.shape[-3:])))
    if not found:
        raise ValueError('the list files name no volume')
    shapes = sorted(set(s for _, s in found))
    listing = ', '.join('%s %s' % (n, 'x'.join(str(v) for v in s)) for n, s in found)
    if patch is not None:
        size = check_patch(patch, models)
        small = [(n, s) for n, s in found if any(v < w for v, w in zip(s, size))]
        if small:
            raise ValueError('volumes smaller than the patch %s on some axis: %s' % ('x'.join(str(v) for v in size),
                                                                                      ', '.join('%s %s' % (n, 'x'.join(str(v) for v in s)) for n, s in small)))
        return size
    if len(shapes) > 1:
        raise ValueError('the prepared volumes do not share one shape (resample / crop them to a common grid): ' + listing)
    for m in models:
        k = shape_multiple(m)
        if any(v % k for v in shapes[0]) or min(shapes[0]) < 1:
            raise ValueError('%s takes volumes whose extents are multiples of %d: %s' % (m, k, listing))
    return shapes[0]


# ---- command line (train_seg.py, train_reg.py, train_joint.py) ----------------------------------------------------------------------------
_ARGUMENT_KEYS = ('nifti_data', 'nifti_data_dir', 'nifti_valid_data_dir', 'train_list', 'valid_list', 'test_list', 'voxel_size',
                  'rescale_percentiles', 'normalize', 'ignore_labels', 'nifti_crop_size', 'nifti_preload')


def add_data_arguments(parser, with_preload=True):
    parser.add_argument('--data', dest='nifti_data', default=None, choices=sorted(med_data.NIFTI_SEG_DATASETS),
                        help='train on NIfTI volumes of this dataset family (list files of scan names + a directory) instead of synthetic ones')
    parser.add_argument('--data-dir', dest='nifti_data_dir', default=None, type=str, help='directory of the volumes named by --train-list')
    parser.add_argument('--valid-data-dir', dest='nifti_valid_data_dir', default=None, type=str,
                        help='directory of the volumes named by --valid-list / --test-list (default: --data-dir)')
    parser.add_argument('--train-list', dest='train_list', default=None, nargs='+', help='list file(s) of the training scans, one name per line')
    parser.add_argument('--valid-list', dest='valid_list', default=None, nargs='+', help='list file(s) of the validation scans')
    parser.add_argument('--test-list', dest='test_list', default=None, nargs='+', help='list file(s) of the test scans')
    parser.add_argument('--voxel-size', dest='voxel_size', default=None, nargs=3, type=float, metavar=('X', 'Y', 'Z'),
                        help='resample every volume to this voxel size on the device (nearest neighbour, as the reference executes)')
    parser.add_argument('--rescale-percentiles', dest='rescale_percentiles', default=None, nargs=2, type=float, metavar=('LO', 'HI'),
                        help='rescale the image so that its LO / HI percentiles map to 0 / 1 (clamped)')
    parser.add_argument('--normalize', dest='normalize', action='store_true', help='normalise the image to zero mean and unit variance')
    parser.add_argument('--ignore-labels', dest='ignore_labels', default=None, nargs='+', type=int, help='labels of the segmentation set to 0')
    parser.add_argument('--crop-size', dest='nifti_crop_size', default=None, nargs='+', type=int,
                        help='CropTensor: 3 (both sides) or 6 (low z y x, high z y x) voxel counts cut off every prepared volume')
    if with_preload:
        parser.add_argument('--preload', '-load', dest='nifti_preload', action='store_true', help='prepare every volume once and keep it on the device')
    return parser


def apply_data_arguments(config):
    """The flags of add_data_arguments -> the reference's config keys.  Without --data nothing is left in the config: a run has the config it
    always had.  Tolerates configs built from namespaces that lack the flags."""
    a = {k: config.pop(k, None) for k in _ARGUMENT_KEYS}
    if not a['nifti_data']:
        return config
    if not a['nifti_data_dir'] or not a['train_list'] or not a['valid_list']:
        raise ValueError('--data needs --data-dir, --train-list and --valid-list')
    config['data'] = a['nifti_data']
    config['data_dir'] = a['nifti_data_dir']
    config['valid_data_dir'] = a['nifti_valid_data_dir'] or a['nifti_data_dir']
    config['training_list_file'] = list(a['train_list'])
    config['validation_list_file'] = list(a['valid_list'])
    if a['test_list']:
        config['testing_list_file'] = list(a['test_list'])
    config['crop_size'] = list(a['nifti_crop_size']) if a['nifti_crop_size'] else None
    if a['nifti_preload']:
        config['preload'] = True
    config['preload'] = bool(config.get('preload'))
    steps = []
    if a['voxel_size']:
        steps.append(['resample', {'voxel_size': [float(v) for v in a['voxel_size']]}])
    if a['rescale_percentiles']:
        steps.append(['percentile_rescale', {'lo': float(a['rescale_percentiles'][0]), 'hi': float(a['rescale_percentiles'][1])}])
    if a['normalize']:
        steps.append(['normalize', {}])
    if a['ignore_labels']:
        steps.append(['label_filter', {'ignore_labels': [int(l) for l in a['ignore_labels']]}])
    if steps:
        config['preprocess'] = steps
    if 'log_dir' in config and 'synthetic' in str(config['log_dir']):
        head, tail = config['log_dir'].rsplit('synthetic', 1)
        config['log_dir'] = head + config['data'] + tail
    return config
