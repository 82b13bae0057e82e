"""RegistrationExperiment: the experiment the reference lists as TODO (README.md:15-19), on the skeleton of SegmentationExperiment.

Model = the registration net (lib/network_factory/voxel_morph.py), step = models/joint.py RegistrationStep (NCC + lambda_reg * bending
energy, unchanged), data = ordered (moving, fixed) pairs (lib/datasets.py:331-451).  Validation scores what a registration is for: the
hard-label registration Dice -- the moving segmentation warped with the predicted deformation (nearest neighbour) against the fixed
segmentation -- next to the same Dice for the identity deformation on the same pairs, and the regularity of the deformation (det J:
mean, standard deviation, folding fraction), all from exact device kernels (lib/evalMetrics.py registration_dice / jacobian_stats).
Checkpoints carry the keys of SegmentationExperiment's ({'epoch', 'model_state_dict', 'optimizer_state_dict', 'best_score'}).
config['atlas_fusion'] ('majority' | 'local', default None: off) adds registration-based segmentation to validation and test(): every
validation volume is segmented from the training volumes (at most atlas_fusion_max = 5) by multi-atlas label fusion (lib/evalMetrics.py
atlas_segmentation) and scored against its own segmentation: atlas_dice_per_class / atlas_dice_avg.
config['sim_loss'] ('ncc' default | 'lncc' | 'mi') and config['sim_settings'] (constructor arguments of that loss) choose the image
similarity of the step; config['moving_remap'] (None | 'invert' | 'fold') gives the synthetic pairs a moving image of another "modality".
config['lambda_jac'] (default 0: off) weights the Jacobian folding penalty of the step (lib/loss.py JacobianFoldingLoss: the trained form of the
folding fraction validation prints); config['jac_settings'] are its constructor arguments (eps, power).
config['lambda_ic'] (default 0: off) weights the inverse-consistency penalty of the step (lib/loss.py InverseConsistencyLoss; the step then predicts
both directions in one doubled-batch forward); config['report_ic'] (default None: on exactly when lambda_ic > 0) makes validation also run the
reverse direction and report the composition residual in voxels (ic_mean_vox, ic_max_vox, ic_outside_frac).
config['affine_init'] (None default: off | 'rigid' | 'affine') runs an affine pre-alignment (lib/affine.py affine_register, settings in
config['affine_settings']) on every pair: training sees (aligned moving, fixed); validation aligns, runs the net on the aligned pair, composes
the affine with the predicted field (ops.affine_disp) and scores that ONE field, so labels are interpolated once, and also reports the Dice of
the affine alone (affine_dice_avg).  config['misalign'] = (rotation in degrees, translation in voxels) (default None) gives every pair's moving
image and segmentation a rigid misalignment, the same one in every epoch (seeded by the pair's name), in training and validation alike.
config['report_tre'] (None default: off | a dict with 'amp_vox' and optionally 'points') makes validation also run the known-deformation
probe (lib/evalMetrics.py known_deformation_tre) on the fixed image of every pair, one more net forward: the landmark error in voxels against
the exact inverse of a known smooth field (tre_mean_vox, tre_max_vox, tre_initial_mean_vox).  It takes no part in the experiment's name.
config['refine'] (None default: off | an iteration count | a dict of lib/refine.py refine_field keywords) makes validation also refine every pair's
field on that pair (refined_dice_avg, refined_fold_frac, refine_sim_before, refine_sim_after); the regulariser weight and the similarity default to
the training ones.  It takes no part in the experiment's name, and model selection and best_score stay on the net's own field.
config['data'] other than 'synthetic' (models/nifti_data.py) trains on the ordered pairs of the NIfTI volumes of a list file; misalign and report_tre
are synthetic-only and raise with such data.
"""
import datetime
import os
import time
import warnings
import zlib

import numpy as np
import torch
from torch.utils.data import DataLoader

from .base import BaseExperiment
from . import nifti_data
from .joint import RegistrationStep, SIM_LOSSES, make_jac_penalty, make_ic_penalty
from .segmentation import SegmentationExperiment, refuse_patch
from ..lib.inference import refuse_tile_blend
from ..lib import datasets as med_data
from ..lib import refine as refine_lib
from ..lib import evalMetrics as metrics
from ..lib import affine as affine_lib
from ..lib.transforms import rigid_index_affine
from ..lib.loss import JacobianFoldingLoss
from ..lib.network_factory import get_network
from ..lib.param_dict import save_dict_to_json
from ..optim import FlatAdam
from .. import ops
from .. import parallel

try:
    from tensorboardX import SummaryWriter
except Exception:                                             # tensorboardX is optional here
    SummaryWriter = None


def _nanmean(a, axis=None):
    """numpy.nanmean without its warning for an all-NaN slice (a class that occurs in no pair stays NaN)."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=RuntimeWarning)
        return np.nanmean(a, axis=axis)


def misalign_pairs(im_m, seg_m, names, misalign):
    """Rigid misalignment of the moving images (N x 1 x D x H x W, on the device) and segmentations (N x D x H x W or None) of a batch:
    per pair, rotation angles (x, y, z) ~ N(0, rot_deg / 2) degrees and a translation ~ N(0, trans_vox / 2) voxels per axis, as
    lib/transforms.py draw_rigid draws them, from a generator seeded by zlib.crc32 of the pair's name: a pair is misaligned the same way in
    every epoch.  About the volume's centre, through rigid_index_affine + ops.spatial_resample: trilinear image with 0.1 outside the
    volume, nearest labels with 0 outside.  Returns (images, segmentations)."""
    rot, trans = misalign
    D, H, W = (int(v) for v in im_m.shape[-3:])
    centre = ((W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0)
    if len(names) != im_m.shape[0]:
        raise ValueError('misalign needs one name per pair, got %d names for %d pairs' % (len(names), im_m.shape[0]))
    mats = []
    for name in names:
        rs = np.random.RandomState(zlib.crc32(str(name).encode()) & 0xffffffff)
        angles = rs.normal(0, rot / 2, 3) * np.pi / 180 if rot > 0 else np.zeros(3)
        shift = rs.normal(0, trans / 2, 3) if trans > 0 else np.zeros(3)
        mats.append(rigid_index_affine(angles, shift, (1.0, 1.0, 1.0), centre))
    if seg_m is not None and seg_m.dtype not in (torch.uint8, torch.int32, torch.int64):
        seg_m = seg_m.long()
    return ops.spatial_resample(im_m.float(), seg_m, np.stack(mats), interpolator='linear')


def eval_registration(model, dataloader, n_classes, device, report_ic=False, affine_init=None, affine_settings=None, misalign=None, tre_probe=None,
                      refine=None):
    """Registration metrics of `model` over a loader of (moving image, fixed image, moving seg, fixed seg, has_moving_seg, name) batches.
    Pairs without a moving segmentation have no registration Dice and are skipped for it; every pair counts for the Jacobian statistics.
    Returns a dict: dice_per_class [C-1] (mean over the pairs that have the class: nanmean), dice_avg (mean over the classes that occur),
    identity_dice_per_class / identity_dice_avg (the same for disp = 0 on the same pairs: what registration bought), nonpos_frac (mean
    folding fraction), det_mean / det_std (means over the pairs of the per-pair mean / standard deviation of det J), n_pairs, n_dice_pairs.
    report_ic: the net is also run in the reverse direction, model(im_t, im_m), and the dict gains ic_mean_vox / ic_max_vox / ic_outside_frac:
    the means over the pairs of the per-pair mean and maximum of the composition residual |u_mt(x) + u_tm(x + u_mt(x))| in voxels and of the
    share of voxels whose sample point leaves the volume (metrics.inverse_consistency).
    misalign: every pair's moving image and segmentation are first misaligned (misalign_pairs).  affine_init ('rigid' | 'affine'): every pair
    is pre-aligned (metrics.affine_align with affine_settings), the net runs on (aligned moving, fixed) and its field is composed with the
    affine (ops.affine_disp): Dice and det J are those of that one field on the ORIGINAL moving labels; the dict gains
    affine_dice_per_class / affine_dice_avg, the Dice under the affine's field alone (the inverse-consistency report is then that of the net on the aligned pair).
    tre_probe (a dict amp_vox, points): the known-deformation probe (metrics.known_deformation_tre) runs on the fixed image of every batch, one
    more net forward, and the dict gains tre_mean_vox / tre_initial_mean_vox (means over the pairs of the per-pair mean landmark error against
    the exact inverse of the known field, and of what no registration would leave) and tre_max_vox (the largest landmark error of any pair).
    refine (a dict of lib/refine.py refine_field keywords): every pair's field -- with affine_init the composed one -- is additionally refined on that
    pair against the original moving image, and the dict gains refined_dice_per_class / refined_dice_avg, refined_fold_frac and refine_sim_before /
    refine_sim_after (the means over the pairs of each pair's 1 - NCC under the net's field and under the refined one; batches beyond 64 pairs are refined in chunks); every other entry is the net's own."""
    dice_aff = []
    dice_ref, fold_ref, sim_ref = [], [], {'before': [], 'after': []}
    tre = {'tre_mean_vox': [], 'tre_max_vox': [], 'tre_initial_mean_vox': []}
    dice, dice_id, jac = [], [], {'nonpos_frac': [], 'mean': [], 'std': []}
    ic = {'mean_vox': [], 'max_vox': [], 'outside_frac': []}
    with torch.no_grad():
        model.eval()
        for im_m, im_t, seg_m, seg_t, has, _name in dataloader:
            im_m, im_t = im_m.to(device), im_t.to(device)
            if misalign is not None:
                im_m, seg_m = misalign_pairs(im_m, seg_m.to(device), _name, misalign)
            disp_aff, im_m0 = None, im_m
            if affine_init is None:
                disp = net_disp = model(im_m, im_t)[0]
            else:
                theta, im_a = metrics.affine_align(im_m, im_t, mode=affine_init, **dict(affine_settings or {}))
                net_disp = model(im_a, im_t)[0]
                disp = ops.affine_disp(theta, net_disp)
                disp_aff = ops.affine_disp(theta, size=im_m.shape[2:])
                im_m = im_a
            js = metrics.jacobian_stats(disp)
            for k in jac:
                jac[k].append(js[k])
            if refine is not None:
                parts = []
                for k in range(0, im_t.shape[0], ops.REFINE_MAX_BATCH):          # the kernels take 64 samples per call; a sample's statistics are its own
                    m_k, t_k, d_k = (t[k:k + ops.REFINE_MAX_BATCH] for t in (im_m0.float(), im_t.float(), disp))
                    parts.append(refine_lib.refine_field(m_k, t_k, d_k, **refine))
                    sim_ref['before'].append(refine_lib.one_minus_ncc(m_k, t_k, d_k, per_sample=True).cpu().numpy())
                    sim_ref['after'].append(refine_lib.one_minus_ncc(m_k, t_k, parts[-1], per_sample=True).cpu().numpy())
                disp_r = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
                fold_ref.append(metrics.jacobian_stats(disp_r)['nonpos_frac'])
            if report_ic:
                ics = metrics.inverse_consistency(net_disp, model(im_t, im_m)[0])
                for k in ic:
                    ic[k].append(ics[k])
            if tre_probe is not None:
                probe = metrics.known_deformation_tre(model, im_t, _name, amp_vox=tre_probe['amp_vox'], n_points=tre_probe['points'])
                for k in tre:
                    tre[k].append(probe[k])
            keep = torch.as_tensor(has).reshape(-1).bool()
            if bool(keep.any()):
                sm, st_, dk = seg_m[keep].to(device), seg_t[keep].to(device), disp[keep.to(device)]
                dice.append(metrics.registration_dice(sm, st_, dk, n_classes))
                dice_id.append(metrics.registration_dice(sm, st_, torch.zeros_like(dk), n_classes))
                if disp_aff is not None:
                    dice_aff.append(metrics.registration_dice(sm, st_, disp_aff[keep.to(device)], n_classes))
                if refine is not None:
                    dice_ref.append(metrics.registration_dice(sm, st_, disp_r[keep.to(device)], n_classes))
    out = {}
    for key, rows in ((('dice', dice), ('identity_dice', dice_id)) + ((('affine_dice', dice_aff),) if affine_init is not None else ())
                      + ((('refined_dice', dice_ref),) if refine is not None else ())):
        per = _nanmean(np.concatenate(rows, 0), axis=0) if rows else np.full(n_classes - 1, np.nan)
        out[key + '_per_class'] = per
        out[key + '_avg'] = float(_nanmean(per)) if np.isfinite(per).any() else float('nan')
    for k, name in (('nonpos_frac', 'nonpos_frac'), ('mean', 'det_mean'), ('std', 'det_std')):
        out[name] = float(np.mean(np.concatenate(jac[k]))) if jac[k] else float('nan')
    if report_ic:
        for k in ic:
            out['ic_' + k] = float(np.mean(np.concatenate(ic[k]))) if ic[k] else float('nan')
    if tre_probe is not None:
        for k in tre:
            rows = np.concatenate(tre[k]) if tre[k] else np.full(1, np.nan)
            out[k] = float(np.max(rows) if k == 'tre_max_vox' else np.mean(rows))
    if refine is not None:
        out['refined_fold_frac'] = float(np.mean(np.concatenate(fold_ref))) if fold_ref else float('nan')
        for k in sim_ref:
            out['refine_sim_' + k] = float(np.mean(np.concatenate(sim_ref[k]))) if sim_ref[k] else float('nan')
    out['n_pairs'] = int(sum(len(a) for a in jac['mean']))
    out['n_dice_pairs'] = int(sum(len(a) for a in dice))
    return out


def dataset_volumes(loader, indices=None, first=None):
    """The (image 1 x D x H x W, segmentation D x H x W) volumes behind a loader: of a pairwise dataset the volumes its pairs are drawn
    from (its .seg), of a volume dataset its samples; `indices` selects and orders them, `first` keeps that many (only those are built)."""
    base = getattr(loader.dataset, 'seg', loader.dataset)
    indices = list(range(len(base)) if indices is None else indices)
    return [tuple(base[i][:2]) for i in (indices if first is None else indices[:first])]


def eval_atlas_fusion(model, atlases, volumes, n_classes, device, mode='majority', radius=2, sigma=0.1, chunk=4):
    """Registration-based segmentation as a score of the registration net: every volume of `volumes` is segmented from the labelled
    `atlases` (lists of (image, segmentation)) with lib/evalMetrics.py atlas_segmentation and scored against its own segmentation.
    Returns {'atlas_dice_per_class' [C-1] (nanmean over the volumes), 'atlas_dice_avg' (mean over the classes that occur)}."""
    if not atlases:
        raise ValueError('atlas fusion needs at least one labelled training volume')
    ims = torch.stack([a[0] for a in atlases]).to(device)
    labs = torch.stack([a[1] for a in atlases]).to(device)
    rows = []
    for im, seg in volumes:
        fused, _ = metrics.atlas_segmentation(model, ims, labs, im.to(device), mode=mode, radius=radius, sigma=sigma, chunk=chunk)
        counts = ops.label_overlap_counts(fused, seg.to(device).reshape(fused.shape), n_classes)
        rows.append(metrics.dice_from_counts(counts)[:, 1:])
    per = _nanmean(np.concatenate(rows, 0), axis=0) if rows else np.full(n_classes - 1, np.nan)
    return {'atlas_dice_per_class': per, 'atlas_dice_avg': float(_nanmean(per)) if np.isfinite(per).any() else float('nan')}


def check_atlas_fusion(cfg):
    """config['atlas_fusion']: None (off, the default), 'majority' or 'local'; config['atlas_fusion_max']: the most atlases used (default 5)."""
    mode = cfg.get('atlas_fusion')
    if mode is not None and mode not in metrics.ATLAS_FUSION_MODES:
        raise ValueError("config['atlas_fusion'] must be None or one of %s, got %r" % (', '.join(metrics.ATLAS_FUSION_MODES), mode))
    cap = int(cfg.get('atlas_fusion_max', 5))
    if mode is not None and not 1 <= cap <= ops.FUSION_MAX_ATLASES:
        raise ValueError("config['atlas_fusion_max'] must be 1..%d, got %r" % (ops.FUSION_MAX_ATLASES, cap))
    return mode, cap


def check_sim_loss(cfg):
    """config['sim_loss']: 'ncc' (the default, also when absent), 'lncc' or 'mi'; config['sim_settings']: that loss's constructor arguments."""
    name = cfg.get('sim_loss') or 'ncc'
    if name not in SIM_LOSSES:
        raise ValueError("config['sim_loss'] must be one of %s, got %r" % (', '.join(sorted(SIM_LOSSES)), name))
    return name, dict(cfg.get('sim_settings') or {})


def check_jac_penalty(cfg):
    """config['lambda_jac']: weight of the Jacobian folding penalty, finite and >= 0 (0, also when absent: off); config['jac_settings']: the
    constructor arguments of JacobianFoldingLoss (eps in [0, 1], power 1 or 2).  Both are checked here, also when the penalty is off."""
    settings = dict(cfg.get('jac_settings') or {})
    unknown = sorted(set(settings) - {'eps', 'power'})
    if unknown:
        raise ValueError("config['jac_settings'] takes 'eps' and 'power', got %s" % ', '.join(repr(k) for k in unknown))
    JacobianFoldingLoss(**settings)                           # raises for a bad eps / power
    return make_jac_penalty(cfg.get('lambda_jac'))[0], settings


def jac_name_suffix(cfg):
    """'_jac<lambda>' for an experiment name when the penalty is on, '' otherwise (names of runs without it stay as they were)."""
    lam = cfg.get('lambda_jac') or 0.0
    return '_jac%s' % lam if lam > 0 else ''


def check_ic_penalty(cfg):
    """config['lambda_ic']: weight of the inverse-consistency penalty, finite and >= 0 (0, also when absent: off); config['report_ic']: whether
    validation reports the inverse-consistency error: None (the default, also when absent) = exactly when lambda_ic > 0.  Returns (weight, report)."""
    lam = make_ic_penalty(cfg.get('lambda_ic'))[0]
    report = cfg.get('report_ic')
    return lam, (lam > 0.0 if report is None else bool(report))


def ic_name_suffix(cfg):
    """'_ic<lambda>' for an experiment name when the penalty is on, '' otherwise (names of runs without it stay as they were)."""
    lam = cfg.get('lambda_ic') or 0.0
    return '_ic%s' % lam if lam > 0 else ''


AFFINE_SETTINGS_KEYS = ('sim', 'sim_settings', 'levels', 'iters', 'lr')


def check_affine_init(cfg):
    """config['affine_init']: None (off, the default, also when absent), 'rigid' or 'affine'; config['affine_settings']: arguments of
    lib/affine.py affine_register among sim, sim_settings, levels, iters, lr (checked here, also when the stage is off).  The stage does not go
    with the inverse-consistency penalty (the symmetric step would need both directions pre-aligned): lambda_ic > 0 raises.
    Returns (mode or None, settings)."""
    mode = cfg.get('affine_init')
    if mode is not None and mode not in affine_lib.AFFINE_MODES:
        raise ValueError("config['affine_init'] must be None or one of %s, got %r" % (', '.join(affine_lib.AFFINE_MODES), mode))
    settings = dict(cfg.get('affine_settings') or {})
    unknown = sorted(set(settings) - set(AFFINE_SETTINGS_KEYS))
    if unknown:
        raise ValueError("config['affine_settings'] takes %s, got %s" % (', '.join(AFFINE_SETTINGS_KEYS), ', '.join(repr(k) for k in unknown)))
    if 'levels' in settings or 'iters' in settings:
        affine_lib.check_schedule(settings.get('levels', affine_lib.DEFAULT_LEVELS), settings.get('iters', affine_lib.DEFAULT_ITERS))
    if 'sim' in settings and settings['sim'] not in affine_lib.SIM_LOSSES:
        raise ValueError("config['affine_settings']['sim'] must be one of %s, got %r" % (', '.join(sorted(affine_lib.SIM_LOSSES)), settings['sim']))
    if 'lr' in settings and not 0.0 < float(settings['lr']) < float('inf'):
        raise ValueError("config['affine_settings']['lr'] must be a finite learning rate > 0, got %r" % (settings['lr'],))
    if mode is not None and float(cfg.get('lambda_ic') or 0.0) > 0.0:
        raise ValueError("config['affine_init'] does not go with config['lambda_ic'] > 0: the symmetric step predicts both directions of a pair, "
                         "and the pre-alignment aligns only the moving image; train with one of the two")
    return mode, settings


def check_misalign(cfg):
    """config['misalign']: None (off, the default, also when absent) or (rotation in degrees, translation in voxels), both finite and >= 0."""
    mis = cfg.get('misalign')
    if mis is None:
        return None
    try:
        rot, trans = (float(v) for v in mis)
    except (TypeError, ValueError):
        raise ValueError("config['misalign'] must be None or (rotation in degrees, translation in voxels), got %r" % (mis,))
    if not (0.0 <= rot < float('inf') and 0.0 <= trans < float('inf')):
        raise ValueError("config['misalign'] takes two finite values >= 0, got %r" % (mis,))
    return rot, trans


TRE_PROBE_POINTS = 1000


def check_report_tre(cfg):
    """config['report_tre']: None (off, the default, also when absent) or a dict with 'amp_vox' (the largest displacement of the known field in
    voxels, finite and > 0) and optionally 'points' (landmarks per pair, default 1000).  The probe deforms the fixed image itself, so it does
    not go with config['affine_init'] (the net would see a pair that was never pre-aligned): that raises.  Returns None or the complete dict."""
    probe = cfg.get('report_tre')
    if probe is None:
        return None
    if not isinstance(probe, dict) or 'amp_vox' not in probe or set(probe) - {'amp_vox', 'points'}:
        raise ValueError("config['report_tre'] must be None or a dict with 'amp_vox' and optionally 'points', got %r" % (probe,))
    amp, points = float(probe['amp_vox']), probe.get('points', TRE_PROBE_POINTS)
    if not 0.0 < amp < float('inf'):
        raise ValueError("config['report_tre']['amp_vox'] must be a finite number of voxels > 0, got %r" % (probe['amp_vox'],))
    if int(points) != points or int(points) < 1:
        raise ValueError("config['report_tre']['points'] must be a whole number >= 1, got %r" % (points,))
    if cfg.get('affine_init'):
        raise ValueError("config['report_tre'] does not go with config['affine_init']: the probe's pairs are not pre-aligned")
    return {'amp_vox': amp, 'points': int(points)}


def check_refine(cfg):
    """config['refine']: None (off, the default, also when absent), an iteration count or a dict of lib/refine.py refine_field keywords: validation
    then also refines every pair's field (eval_registration).  What the value leaves open comes from the training config (the regulariser weight,
    the similarity).  It takes no part in the experiment's name, in model selection or in best_score.  Returns None or the complete dict."""
    return refine_lib.settings_from_config(cfg, cfg.get('refine'))


def refuse_refine(cfg, experiment):
    """The experiments that do not refine at validation say so instead of ignoring the key."""
    if cfg.get('refine') is not None:
        raise ValueError("config['refine'] is not supported by the %s experiment: refine a trained net's fields with the registration experiment or predict_reg.py"
                         % experiment)


def refine_text(res):
    if 'refined_dice_avg' not in res:
        return ''
    return ', refined Dice {:.4f} (folding {:.4f})'.format(res['refined_dice_avg'], res['refined_fold_frac'])


def tre_text(res):
    """What a validation or test line adds when the known-deformation probe is on ('' otherwise)."""
    if 'tre_mean_vox' not in res:
        return ''
    return ', TRE {:.2f} (initial {:.2f}) vox'.format(res['tre_mean_vox'], res['tre_initial_mean_vox'])


def affine_name_suffix(cfg):
    """'_misalign<rot>_<trans>' and '_affine<mode>' for an experiment name when they are on, '' otherwise (names of runs without them stay as
    they were)."""
    mis = cfg.get('misalign')
    text = '_misalign%s_%s' % tuple(mis) if mis is not None else ''
    return text + ('_affine%s' % cfg['affine_init'] if cfg.get('affine_init') else '')


def affine_text(res):
    """What a validation or test line adds beside the identity Dice when the affine stage is on ('' otherwise)."""
    return ', affine {:.4f}'.format(res['affine_dice_avg']) if 'affine_dice_avg' in res else ''


def ic_text(res):
    """What a validation or test line adds when the inverse-consistency report is on ('' otherwise)."""
    if 'ic_mean_vox' not in res:
        return ''
    return '  inverse consistency {:.4f} vox mean, {:.3f} max, {:.3%} outside'.format(res['ic_mean_vox'], res['ic_max_vox'], res['ic_outside_frac'])


def atlas_fusion_text(res):
    """What a validation line adds when atlas fusion is on ('' otherwise)."""
    if 'atlas_dice_avg' not in res:
        return ''
    return '  atlas-fusion Dice Avg: {:.4f} per class {}'.format(
        res['atlas_dice_avg'], np.array2string(np.asarray(res['atlas_dice_per_class']), precision=3, max_line_width=100000))


class RegistrationExperiment(BaseExperiment):
    def __init__(self, config):
        super(RegistrationExperiment, self).__init__(config)
        self.device = torch.device(self.config.get('device', 'cuda'))
        cfg = self.config
        refuse_patch(cfg, 'registration')
        refuse_tile_blend(cfg, 'registration')
        if cfg['debug_mode']:
            print("Debug mode")
            cfg['print_batch_period'] = cfg['valid_epoch_period'] = 2
        self.atlas_fusion, self.atlas_fusion_max = check_atlas_fusion(cfg)
        self.sim_loss, self.sim_settings = check_sim_loss(cfg)
        self.lambda_jac, self.jac_settings = check_jac_penalty(cfg)
        self.lambda_ic, self.report_ic = check_ic_penalty(cfg)
        self.affine_init, self.affine_settings = check_affine_init(cfg)
        self.misalign = check_misalign(cfg)
        self.report_tre = check_report_tre(cfg)
        self.refine = check_refine(cfg)
        nifti_data.refuse_synthetic_only(cfg, ('misalign', 'report_tre'))
        self.exp_name = self.experiment_name(cfg)
        run_dir = "debug_reg" if cfg['debug_mode'] else self.exp_name
        self.ckpoint_dir = os.path.join(cfg['log_dir'], run_dir, str(cfg['random_seed']))
        self.writer = None
        self.global_step = 0
        self.best_score = 0
        self.current_epoch = 1
        self.training_data_loader = self.config.get('training_data_loader')
        self.validation_data_loader = self.config.get('validation_data_loader')
        print("Init experiment {} seed {}".format(self.exp_name, self.config['random_seed']))

    @staticmethod
    def experiment_name(cfg):
        """Reg_<model>_<data dir name>_<n>samples_batch_<b>_<e>epochs_<sim_loss>_bending_<lambda_reg>_lr_<lr>[_scheduler_<mode>][_moving<remap>][_jac<lambda_jac>][_ic<lambda_ic>][_misalign<rot>_<trans>][_affine<mode>]"""
        parts = ['Reg_', cfg['model'], '_', os.path.basename(cfg['data_dir']), '_%ssamples' % cfg['num_samples'], '_batch_%s' % cfg['batch_size'],
                 '_%sepochs' % cfg['n_epochs'], '_%s_bending_%s' % (cfg.get('sim_loss') or 'ncc', cfg['lambda_reg']), '_lr_%s' % cfg['learning_rate']]
        if cfg['lr_mode'] != 'const':
            parts.append('_scheduler_%s' % cfg['lr_mode'])
        if cfg.get('moving_remap'):
            parts.append('_moving%s' % cfg['moving_remap'])
        parts.append(jac_name_suffix(cfg))
        parts.append(ic_name_suffix(cfg))
        parts.append(affine_name_suffix(cfg))
        return ''.join(str(v) for v in parts)

    # ---- setup ---------------------------------------------------------------------------------
    def setup_log(self):
        if parallel.rank() != 0:
            return
        if not os.path.isdir(self.ckpoint_dir):
            os.makedirs(self.ckpoint_dir)
        save_dict_to_json(self.config, os.path.join(self.ckpoint_dir, "train_config.json"))
        if SummaryWriter is not None:
            self.writer = SummaryWriter(self.ckpoint_dir)

    def setup_train_data(self):
        if self.training_data_loader is not None:
            return
        if nifti_data.is_nifti(self.config):
            return self.setup_nifti_data()
        dataset = med_data.get_reg_dataset(self.config['data'])
        shape = self.config['synthetic_shape']
        remap = {'moving_remap': self.config['moving_remap']} if self.config.get('moving_remap') else {}
        training_data = dataset(max(self.config['num_samples'], 2), shape, self.config['n_classes'], seed=self.config['random_seed'], **remap)
        sampler = parallel.distributed_sampler(training_data, shuffle=True, seed=self.config['random_seed'])
        self.training_data_loader = DataLoader(training_data, batch_size=self.config['batch_size'], shuffle=sampler is None,
                                               sampler=sampler, num_workers=0)
        validation_data = dataset(max(self.config.get('num_valid_samples', 2), 2), shape, self.config['n_classes'],
                                  seed=self.config['random_seed'] + 1000, **remap)
        self.validation_data_loader = DataLoader(validation_data, batch_size=1, shuffle=False, num_workers=0)

    def setup_nifti_data(self):
        """Pairs over the reference's list-file volume datasets (models/nifti_data.py): the training list's first num_samples scans, the
        validation list whole; all volumes must share one shape."""
        cfg = self.config
        remap = {'moving_remap': cfg['moving_remap']} if cfg.get('moving_remap') else {}
        training_vols = nifti_data.seg_dataset(cfg, 'training_list_file', 'data_dir', n_samples=max(cfg['num_samples'], 2))
        validation_vols = nifti_data.seg_dataset(cfg, 'validation_list_file', 'valid_data_dir')
        if training_vols is None or validation_vols is None:
            raise ValueError("config['data'] = %r needs config['training_list_file'] and config['validation_list_file']" % (cfg['data'],))
        nifti_data.check_shapes([training_vols, validation_vols], [cfg['model']])
        training_data = med_data.NiftiRegDataset(training_vols, **remap)
        sampler = parallel.distributed_sampler(training_data, shuffle=True, seed=cfg['random_seed'])
        self.training_data_loader = DataLoader(training_data, batch_size=cfg['batch_size'], shuffle=sampler is None, sampler=sampler, num_workers=0)
        self.validation_data_loader = DataLoader(med_data.NiftiRegDataset(validation_vols, **remap), batch_size=1, shuffle=False, num_workers=0)

    def setup_model(self):
        self.model = get_network(self.config['model'])(**self.config.get('model_settings', {}))
        self.model.to(self.device)

    def setup_optimizer(self):
        self.optimizer = FlatAdam(self.model.parameters(), lr=self.config['learning_rate'])
        ops.enable_async_wgrad(bool(self.config.get('async_wgrad', True)))
        ops.set_matrix_precision(self.config.get('matrix_precision') or ops.DEFAULT_MATRIX_PRECISION)
        self.scheduler = SegmentationExperiment.make_scheduler(self.optimizer, self.config)
        self.step = RegistrationStep(self.model, self.optimizer, lam_reg=self.config['lambda_reg'], sim_loss=self.sim_loss, sim_settings=self.sim_settings,
                                     lam_jac=self.lambda_jac, jac_settings=self.jac_settings, lam_ic=self.lambda_ic)

    # ---- training ------------------------------------------------------------------------------
    def train(self):
        self.setup_train()
        print("Training {}".format(self.exp_name))
        finished_epoch, self.best_score = self.initialize_model(self.model, self.optimizer, self.config['resume_dir'])
        parallel.broadcast_parameters(self.optimizer, model=self.model)
        parallel.pin_host_resources()
        self.current_epoch = finished_epoch + 1
        for epoch in range(self.current_epoch, self.config['n_epochs'] + 1):
            self.train_one_epoch()
            self.validate()
            self.current_epoch += 1
        if self.writer is not None:
            self.writer.close()
        print('Finished Training: {}'.format(self.exp_name))

    def train_step(self, im_m, im_t, names=None):
        """One RegistrationStep on a batch of pairs: (loss, (disp, warped, deform), (similarity, bending)).  With config['misalign'] the moving
        images are misaligned first (`names`: the pairs' names, which seed it); with config['affine_init'] they are then pre-aligned to the
        fixed images without autograd, and the step sees (aligned moving, fixed)."""
        im_m, im_t = im_m.to(self.device, non_blocking=True), im_t.to(self.device, non_blocking=True)
        if self.misalign is not None:
            if names is None:
                raise ValueError("config['misalign'] needs the pairs' names to seed the misalignment")
            im_m = misalign_pairs(im_m, None, names, self.misalign)[0]
        if self.affine_init is not None:
            with torch.no_grad():
                im_m = metrics.affine_align(im_m, im_t, mode=self.affine_init, **self.affine_settings)[1]
        return self.step(im_m, im_t)

    def train_one_epoch(self):
        running_loss = 0.0
        running_jac = None                         # the folding penalty of the period, summed on the device (penalty on only)
        running_ic = None                          # likewise the inverse-consistency penalty (report on and penalty on only)
        log_ic = self.report_ic and self.step.ic is not None
        iters_per_epoch = max(self.config['samples_per_epoch'] // (self.config['batch_size'] * parallel.world_size()), 1)
        train_data_iter = None
        period = self.config['print_batch_period']
        for i in range(iters_per_epoch):
            try:
                batch = next(train_data_iter)
            except (StopIteration, TypeError):
                train_data_iter = iter(self.training_data_loader)
                batch = next(train_data_iter)
            self.global_step = (self.current_epoch - 1) * iters_per_epoch + (i + 1) * self.config['batch_size']
            loss, _, _ = self.train_step(batch[0], batch[1], batch[5])
            running_loss += loss.item()
            if self.step.jac is not None:
                running_jac = self.step.last_jac if running_jac is None else running_jac + self.step.last_jac
            if log_ic:
                running_ic = self.step.last_ic if running_ic is None else running_ic + self.step.last_ic
            if i % period == period - 1:
                if parallel.rank() == 0:
                    jac_text = '' if running_jac is None else ' jac: {:.3e}'.format(running_jac.item() / (period if i > 0 else 1))
                    if running_ic is not None:
                        jac_text += ' ic: {:.3e}'.format(running_ic.item() / (period if i > 0 else 1))
                    print('Epoch[{}/{}] it {} loss: {:.3f}{} lr:{} {}'.format(
                        self.current_epoch, self.config['n_epochs'], i + 1, running_loss / period if i > 0 else running_loss, jac_text,
                        self.optimizer.param_groups[0]['lr'], datetime.datetime.now().strftime("%D %H:%M:%S")))
                    if self.writer is not None:
                        self.writer.add_scalar('loss/training', running_loss / period, global_step=self.global_step)
                        self.writer.add_scalar('learning_rate', self.optimizer.param_groups[0]['lr'], global_step=self.global_step)
                        if running_jac is not None:
                            self.writer.add_scalar('loss/training_jac', running_jac.item() / period, global_step=self.global_step)
                        if running_ic is not None:
                            self.writer.add_scalar('loss/training_ic', running_ic.item() / period, global_step=self.global_step)
                running_loss = 0.0
                running_jac = None
                running_ic = None

    def eval(self, dataloader):
        res = eval_registration(self.model, dataloader, self.config['n_classes'], self.device, report_ic=self.report_ic,
                                affine_init=self.affine_init, affine_settings=self.affine_settings, misalign=self.misalign, tre_probe=self.report_tre,
                                refine=self.refine)
        if self.atlas_fusion:
            # the volumes behind the loader's pairs, each segmented from the training volumes (all labelled here), at most atlas_fusion_max
            if self.training_data_loader is None:
                self.setup_train_data()
            atlases = dataset_volumes(self.training_data_loader, first=self.atlas_fusion_max)
            res.update(eval_atlas_fusion(self.model, atlases, dataset_volumes(dataloader), self.config['n_classes'], self.device,
                                         mode=self.atlas_fusion))
        return res

    def validate(self):
        if self.current_epoch % self.config['valid_epoch_period'] != 0:
            return
        start_time = time.time()
        res = self.last_validation = self.eval(self.validation_data_loader)
        score = res['dice_avg']
        if self.scheduler is not None:
            if self.config['lr_mode'] == 'plateau':
                self.scheduler.step(score)
            else:
                self.scheduler.step()
        # (the first validation of a run always leaves a best file, also when its score is 0 or NaN: test() reloads it)
        is_best = not os.path.isfile(os.path.join(self.ckpoint_dir, 'model_best.pth.tar'))
        if score > self.best_score:
            is_best = True
            self.best_score = score
        if parallel.rank() != 0:
            return
        if self.writer is not None:
            tag = 'validation_{}/'.format(self.config['data'])
            for k in ('dice_avg', 'identity_dice_avg', 'nonpos_frac', 'det_mean', 'det_std'):
                self.writer.add_scalar(tag + k, res[k], global_step=self.global_step)
            for k in ('ic_mean_vox', 'ic_max_vox', 'ic_outside_frac', 'affine_dice_avg', 'tre_mean_vox', 'tre_max_vox', 'tre_initial_mean_vox',
                      'refined_dice_avg', 'refined_fold_frac', 'refine_sim_before', 'refine_sim_after'):
                if k in res:
                    self.writer.add_scalar(tag + k, res[k], global_step=self.global_step)
        print("Validation: registration Dice Avg: {:.4f} (identity {:.4f}{}){}  det J {:.4f} +- {:.4f}, folding {:.3%}{}{}{} ({:.3f} sec) {}".format(
            score, res['identity_dice_avg'], affine_text(res), atlas_fusion_text(res), res['det_mean'], res['det_std'], res['nonpos_frac'], refine_text(res), ic_text(res), tre_text(res), time.time() - start_time,
            datetime.datetime.now().strftime("%D %H:%M:%S")))
        if self.current_epoch % self.config['save_ckpts_epoch_period'] == 0:
            self.save_checkpoint({'epoch': self.current_epoch,
                                  'model_state_dict': self.model.state_dict(),
                                  'optimizer_state_dict': self.optimizer.state_dict(),
                                  'best_score': self.best_score},
                                 is_best, self.ckpoint_dir)

    def test(self, best=True, if_log=True):
        """Reload the best (or the last) checkpoint and report the registration metrics on the test loader."""
        self.setup_model()
        if self.validation_data_loader is None:
            self.setup_train_data()
        ckpoint_file = os.path.join(self.ckpoint_dir, 'model_best.pth.tar' if best else 'checkpoint.pth.tar')
        last_epoch, best_score = self.initialize_model(self.model, optimizer=None, ckpoint_path=ckpoint_file)
        loader = self.config.get('testing_data_loader') or self.validation_data_loader
        res = self.eval(loader)
        print('Testing Model: {} ({} epochs)  registration Dice_avg: {} (identity {}{})  folding fraction: {}{}{}{}'.format(
            ckpoint_file, last_epoch, res['dice_avg'], res['identity_dice_avg'], affine_text(res), res['nonpos_frac'], atlas_fusion_text(res), ic_text(res), tre_text(res)))
        return res
