"""Register pairs of NIfTI scans with a trained registration net and write the moving scan, its labels and the field on the fixed scan's own grid.

    python predict_reg.py --ckpt CKPT --output-dir DIR (--moving FILE... --fixed FILE... | --data-dir DIR --pair-list FILE)
        [--config JSON] [--interp linear|bspline] [--moving-labels FILE...] [--fixed-labels FILE...] [--label-dir DIR] [--save-field]
        [--refine ITERS [--refine-lr VOX] [--refine-lambda-reg W] [--refine-sim ncc|lncc|mi]]

The config is the train_config.json the experiment wrote beside its checkpoints (--config names another; find_config and load_model are
predict_seg.py's).  Per pair: lib/nifti.py reads both files; config['preprocess'] (and config['crop_size']) prepares both as training did
(lib/inference.py prepare); the two prepared shapes must agree and suit the net (nifti_data.check_shapes' ValueError otherwise); the net
predicts one field on the prepared grid, with config['affine_init'] after the affine pre-alignment and composed with it
(lib/inference.py RegistrationPredictor).  Then the moving FILE's raw intensities are carried onto the fixed FILE's grid with one
interpolation (ops.warp_to_grid: every output voxel's position goes through fixed frame -> field -> moving frame; cubic B-spline by default,
--interp linear for trilinear) and written as <moving>_to_<fixed>_warped.nii.gz, float32, with the fixed file's geometry.  --moving-labels
adds ..._seg.nii.gz (nearest neighbour, the labels' dtype, config['preprocess']'s label_filter applied as predict_seg.py does),
--save-field ..._field.nii.gz (the displacement in millimetres between the two files' world frames, lib/nifti.py write_nifti_field).
Per pair the Jacobian statistics of the prepared-grid field are printed; with both label sets also the Dice of the warped labels on the
fixed file's grid beside the Dice a zero field gives through the same op; at the end their means.
--refine ITERS refines every pair's field on that pair (lib/refine.py refine_field: ITERS Adam iterations of --refine-lr voxels on the similarity
under the bending energy; the weight and the similarity default to the checkpoint's train_config.json) and prints
`refine: 1-NCC a.bcde -> f.ghij (K iterations)`; everything written and the det J line then belong to the refined field, and with both label
sets the Dice of the unrefined field is printed beside the refined one.
Out of scope: reorientation by the affine and oblique grids, the inverse direction, tiled registration, joint checkpoints beyond loading
their reg_ file, clamping the cubic overshoot."""
import argparse
import json
import os

import numpy as np
import torch

INTERP_ORDER = {'linear': 1, 'bspline': 3}


def build_parser():
    parser = argparse.ArgumentParser(description='Register pairs of NIfTI scans with a trained net.')
    parser.add_argument('--ckpt', required=True, type=str, help='checkpoint file (model_best.pth.tar / checkpoint.pth.tar)')
    parser.add_argument('--output-dir', required=True, type=str, help='directory the results are written to')
    parser.add_argument('--moving', nargs='+', default=None, metavar='FILE', help='moving scans (.nii / .nii.gz)')
    parser.add_argument('--fixed', nargs='+', default=None, metavar='FILE', help='fixed scans, one per --moving')
    parser.add_argument('--data-dir', default=None, type=str, help='with --pair-list: directory of the scans, named as the training dataset names them')
    parser.add_argument('--pair-list', dest='pair_list', default=None, type=str, help='list file, one pair per line: moving name, fixed name')
    parser.add_argument('--config', default=None, type=str, help='config JSON (default: train_config.json beside the checkpoint)')
    parser.add_argument('--device', '-g', default='0', type=str, help='index of used GPU')
    parser.add_argument('--interp', default='bspline', choices=sorted(INTERP_ORDER), help='interpolation of the moving intensities (default bspline)')
    parser.add_argument('--moving-labels', nargs='+', default=None, metavar='FILE', help='label files of the moving scans, one per --moving')
    parser.add_argument('--fixed-labels', nargs='+', default=None, metavar='FILE', help='label files of the fixed scans, one per --fixed, to score against')
    parser.add_argument('--label-dir', default=None, type=str, help='with --pair-list: directory of both scans\' label files, named as the training dataset names them')
    parser.add_argument('--save-field', action='store_true', help='also write <pair>_field.nii.gz: the displacement in millimetres')
    parser.add_argument('--refine', default=None, type=int, metavar='ITERS', help="refine every pair's field on that pair by ITERS Adam iterations (default: off)")
    parser.add_argument('--refine-lr', default=None, type=float, metavar='VOX', help='step of --refine in voxels (default 0.1)')
    parser.add_argument('--refine-lambda-reg', default=None, type=float, metavar='W', help="bending-energy weight of --refine (default: the checkpoint's lambda_reg)")
    parser.add_argument('--refine-sim', default=None, choices=['ncc', 'lncc', 'mi'], help="similarity of --refine (default: the checkpoint's sim_loss)")
    return parser


def refine_settings(args, cfg):
    """None without --refine, else the refine_field keywords: the flags over the checkpoint's training config (lib/refine.py settings_from_config).
    The other --refine-* flags need --refine."""
    from deepatlas_amd.lib.refine import settings_from_config
    given = {k: v for k, v in (('lr_vox', args.refine_lr), ('lambda_reg', args.refine_lambda_reg), ('sim', args.refine_sim)) if v is not None}
    if args.refine is None:
        if given:
            raise ValueError('--refine-lr / --refine-lambda-reg / --refine-sim go with --refine ITERS')
        return None
    return settings_from_config(cfg, dict(given, iters=args.refine))


def read_pair_list(path):
    """[(moving name, fixed name)] of a list file: two names per line, separated by white space or a comma; blank lines are skipped."""
    pairs = []
    with open(path) as f:
        for k, line in enumerate(f):
            names = line.replace(',', ' ').split()
            if not names:
                continue
            if len(names) != 2:
                raise ValueError('%s line %d: a pair takes two scan names, got %r' % (path, k + 1, line.strip()))
            pairs.append((names[0], names[1]))
    if not pairs:
        raise ValueError('%s names no pair' % path)
    return pairs


def resolve_pairs(args, cfg):
    """[(pair name, moving name, moving path, fixed name, fixed path, moving label path or None, fixed label path or None)] of the command line."""
    from deepatlas_amd.lib import datasets as med_data
    from predict_seg import scan_name
    family = med_data.NIFTI_SEG_DATASETS.get(cfg.get('data'), med_data.SegDataSetOAIZIB)
    files, listed = args.moving is not None or args.fixed is not None, args.pair_list is not None
    if files == listed:
        raise ValueError('give --moving FILE... --fixed FILE..., or --data-dir DIR --pair-list FILE')
    if files:
        if args.moving is None or args.fixed is None or len(args.moving) != len(args.fixed):
            raise ValueError('--moving and --fixed take one file each per pair')
        if args.label_dir is not None:
            raise ValueError('--label-dir goes with --pair-list; with --moving / --fixed use --moving-labels / --fixed-labels')
        for flag, given, scans in (('--moving-labels', args.moving_labels, args.moving), ('--fixed-labels', args.fixed_labels, args.fixed)):
            if given is not None and len(given) != len(scans):
                raise ValueError('%s takes one file per pair' % flag)
        n = len(args.moving)
        rows = zip([scan_name(p) for p in args.moving], args.moving, [scan_name(p) for p in args.fixed], args.fixed,
                   args.moving_labels or [None] * n, args.fixed_labels or [None] * n)
    else:
        if not args.data_dir:
            raise ValueError('--pair-list needs --data-dir')
        if args.moving_labels is not None or args.fixed_labels is not None:
            raise ValueError('--moving-labels / --fixed-labels go with --moving / --fixed; with --pair-list use --label-dir')
        image = lambda n: os.path.join(args.data_dir, family.IMAGE_PATTERN[0], family.IMAGE_PATTERN[1] % n)
        label = lambda n: os.path.join(args.label_dir, family.SEGMENTATION_PATTERN[0], family.SEGMENTATION_PATTERN[1] % n) if args.label_dir else None
        rows = [(m, image(m), f, image(f), label(m), label(f)) for m, f in read_pair_list(args.pair_list)]
    return [('%s_to_%s' % (m, f), m, mp, f, fp, ml, fl) for m, mp, f, fp, ml, fl in rows]


def native_tensor(array, device, labels=False):
    """A file's array on the device in a dtype the warp takes: as it is when it can be, else float32 (intensities) / int32 (labels)."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    ok = (torch.uint8, torch.int16, torch.int32) if labels else (torch.float32, torch.float64, torch.int16, torch.uint8, torch.int32)
    if t.dtype not in ok:
        t = t.to(torch.int32 if labels else torch.float32)
    return t.to(device)


def read_labels(path, name, label_filters):
    """The label file as predict_seg.py scores it: config['preprocess']'s label_filter steps applied to the raw array."""
    from deepatlas_amd.lib.nifti import read_nifti
    vol = read_nifti(path)
    sample = {'segmentation': vol.array, 'image': None, 'name': name}
    for t in label_filters:
        sample = t(sample)
    seg = sample['segmentation']
    seg = seg.cpu().numpy() if torch.is_tensor(seg) else np.asarray(seg)
    return vol, np.ascontiguousarray(seg.astype(vol.array.dtype, copy=False))


def native_dice(warped, truth, n_class):
    """Mean Dice over the foreground classes that occur, of two label maps on one grid (device tensors)."""
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics as metrics
    as_counted = lambda t: t if t.dtype in (torch.uint8, torch.int32, torch.int64) else t.to(torch.int32)
    counts = ops.label_overlap_counts(as_counted(warped).unsqueeze(0), as_counted(truth).unsqueeze(0), n_class)
    d = metrics.dice_from_counts(counts)[0, 1:]
    return float(np.nanmean(d)) if np.any(~np.isnan(d)) else float('nan')


def format_pair(name, jac, dice=None, identity=None, unrefined=None):
    line = 'det J mean %.4f std %.4f folds %d' % (jac['mean'], jac['std'], jac['folds'])
    if dice is not None:
        line = 'Dice Avg: %.6f (identity %.6f%s), ' % (dice, identity, '' if unrefined is None else ', unrefined %.6f' % unrefined) + line
    return '%s: %s' % (name, line)


def format_refine(before, after, iters):
    return 'refine: 1-NCC %.4f -> %.4f (%d iterations)' % (before, after, iters)


def main(argv=None):
    args = build_parser().parse_args(argv)
    from deepatlas_amd.lib import evalMetrics as metrics
    from deepatlas_amd.lib import transforms as T
    from deepatlas_amd.lib.inference import RegistrationPredictor, prepare
    from deepatlas_amd.lib.nifti import write_nifti, write_nifti_field
    from deepatlas_amd.lib.refine import one_minus_ncc
    from deepatlas_amd.models import nifti_data
    from deepatlas_amd.models.registration import check_affine_init
    from predict_seg import find_config, load_model
    with open(find_config(args.ckpt, args.config)) as f:
        cfg = json.load(f)
    pairs = resolve_pairs(args, cfg)
    refine = refine_settings(args, cfg)               # (checked before anything is loaded)
    affine_init, affine_settings = check_affine_init(cfg)
    device = torch.device('cuda:{}'.format(args.device) if args.device.isdigit() else args.device)
    torch.cuda.set_device(device)
    predictor = RegistrationPredictor(load_model(cfg, args.ckpt, device), affine_init, affine_settings, refine=refine)
    n_class = int(cfg.get('n_classes') or 0)
    label_filters = [t for t in T.make_preprocess(cfg.get('preprocess')) if isinstance(t, T.SegmentationLabelFilter)]
    order = INTERP_ORDER[args.interp]
    os.makedirs(args.output_dir, exist_ok=True)
    rows = []
    for name, m_name, m_path, f_name, f_path, m_lab, f_lab in pairs:
        vol_m, im_m, rec_m = prepare(m_path, m_name, cfg)
        vol_f, im_f, rec_f = prepare(f_path, f_name, cfg)
        nifti_data.check_shapes([[(im_m, None, m_name), (im_f, None, f_name)]], [cfg['model']])
        im_m, im_f = im_m.to(device), im_f.to(device)
        disp = net_disp = predictor.net_field(im_m, im_f)
        if refine is not None:
            disp = predictor.refined(im_m, im_f, net_disp)
            sim = [float(one_minus_ncc(*(t.reshape((1, 1) + tuple(t.shape[-3:])).float() for t in (im_m, im_f)), d)) for d in (net_disp, disp)]
            print(format_refine(sim[0], sim[1], refine['iters']))
        out = predictor.apply(native_tensor(vol_m.array, device), disp, vol_f, rec_f, vol_m, rec_m, order=order, world=args.save_field)
        warped, world = out if args.save_field else (out, None)
        stem = os.path.join(args.output_dir, name)
        write_nifti(stem + '_warped.nii.gz', warped.cpu().numpy(), like=vol_f)
        if world is not None:
            write_nifti_field(stem + '_field.nii.gz', world.cpu().numpy(), like=vol_f)
        js = metrics.jacobian_stats(disp)
        jac = {'mean': float(js['mean'][0]), 'std': float(js['std'][0]), 'folds': int(js['n_nonpos'][0])}
        dice = identity = unrefined = None
        if m_lab is not None:
            lab_vol, lab = read_labels(m_lab, m_name, label_filters)
            if tuple(lab.shape) != tuple(vol_m.array.shape):
                raise ValueError('%s holds %s voxels, the scan %s' % (m_lab, tuple(lab.shape), tuple(vol_m.array.shape)))
            lab_dev = native_tensor(lab, device, labels=True)
            moved = predictor.apply(lab_dev, disp, vol_f, rec_f, vol_m, rec_m, order=0)
            write_nifti(stem + '_seg.nii.gz', moved.cpu().numpy().astype(lab.dtype, copy=False), like=vol_f)
            if f_lab is not None:
                if n_class < 2:
                    raise ValueError("scoring needs config['n_classes']")
                _, truth = read_labels(f_lab, f_name, label_filters)
                if tuple(truth.shape) != tuple(vol_f.array.shape):
                    raise ValueError('%s holds %s voxels, the scan %s' % (f_lab, tuple(truth.shape), tuple(vol_f.array.shape)))
                truth_dev = native_tensor(truth, device, labels=True)
                still = predictor.apply(lab_dev, torch.zeros_like(disp), vol_f, rec_f, vol_m, rec_m, order=0)
                dice, identity = native_dice(moved, truth_dev, n_class), native_dice(still, truth_dev, n_class)
                if refine is not None:
                    unrefined = native_dice(predictor.apply(lab_dev, net_disp, vol_f, rec_f, vol_m, rec_m, order=0), truth_dev, n_class)
        rows.append((jac, dice, identity, unrefined))
        print(format_pair(name, jac, dice, identity, unrefined))
    mean_jac = {'mean': float(np.mean([r[0]['mean'] for r in rows])), 'std': float(np.mean([r[0]['std'] for r in rows])),
                'folds': int(round(float(np.mean([r[0]['folds'] for r in rows]))))}
    scored = [r for r in rows if r[1] is not None]
    print(format_pair('mean over %d pairs' % len(rows), mean_jac,
                      float(np.nanmean([r[1] for r in scored])) if scored else None, float(np.nanmean([r[2] for r in scored])) if scored else None,
                      float(np.nanmean([r[3] for r in scored])) if scored and refine is not None else None))


if __name__ == '__main__':
    main()
