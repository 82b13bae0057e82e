"""SegmentationExperiment: mirror of models/segmentation.py with the step loop on the HIP path.

Same config keys (train_seg.py:33-61), same setup order, same step semantics (models/segmentation.py:141-157:
train(); zero_grad(); out = model(x); loss = crit(out, y.long()); backward(); Adam.step(); loss.item()), eval =
argmax -> per-class Dice for classes 1..C-1 averaged over volumes then classes (:179-201), validate ->
scheduler.step + checkpoint (:203-239).  Differences, all host-side: the device is explicit
(config['device'], default 'cuda'), data comes from config['data'] == 'synthetic', from the reference's NIfTI list-file datasets
(config['data'] 'OAI', 'OASIS', 'LPBA40', 'CUMC12', 'IBSR18', 'MGH10' or 'MindBoggle' with the reference's keys data_dir, valid_data_dir,
training_list_file, validation_list_file, testing_list_file, preload, crop_size, num_samples, plus the optional config['preprocess'];
models/nifti_data.py) or from injected loaders,
TensorBoard logging is optional, eval Dice is computed on the device (lib/evalMetrics.py), and with
torch.distributed initialised the gradients are averaged with one flat-bucket all-reduce (parallel.py).
config['lambda_boundary'] (default 0: off) weights Kervadec's boundary loss as a second term of the step (lib/loss.py BoundaryLoss: signed
distance maps built on the device from the batch's index labels, after any augmentation); config['boundary_settings'] optionally holds its
`classes` and `spacing`.  Without the key, or with 0, nothing changes.
config['patch'] (default None: off; parse_patch states its form) turns on patch training and tiled evaluation: a training batch is
batch_size patches cropped on the device (lib/transforms.py BalancedRandomCrop / RandomCrop's uniform draw) from batch_size / per_volume
volumes, cropped before config['augment'] acts; validation and test tile every volume with Partition, run the net over the tiles and assemble
the argmax.  Volumes of different shapes then train together.  Without the key nothing changes.
config['tile_blend'] (default None: off; lib/inference.py parse_tile_blend states its form; it needs config['patch']) replaces the tiled
evaluation's core copy by blended sliding-window inference (lib/inference.py SlidingWindowPredictor): the overlapping tiles' probabilities
are averaged under a window, optionally over mirrored copies.  It takes no part in the experiment's name; without the key nothing changes.
"""
import datetime
import os
import time

import numpy as np
import torch
import torch.optim.lr_scheduler as lr_scheduler
from torch.utils.data import DataLoader

from .base import BaseExperiment
from . import nifti_data
from ..lib import datasets as med_data
from ..lib import evalMetrics as metrics
from ..lib import inference
from ..lib import transforms as med_transforms
from ..lib.loss import get_loss_function, BoundaryLoss
from ..lib.network_factory import get_network
from ..lib.param_dict import save_dict_to_json
from ..optim import FlatAdam
from .. import ops
from .. import parallel
from .. import trace

try:
    from tensorboardX import SummaryWriter
except Exception:                                             # tensorboardX is optional here
    SummaryWriter = None


def check_boundary_term(cfg):
    """config['lambda_boundary']: weight of the boundary loss, finite and >= 0 (0, also when absent: off); config['boundary_settings']: the
    optional constructor arguments `classes` and `spacing` of BoundaryLoss.  Both are checked here, also when the term is off."""
    lam = cfg.get('lambda_boundary')
    lam = 0.0 if lam is None else lam
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= float(lam) < float('inf'):
        raise ValueError("config['lambda_boundary'] must be a finite number >= 0, got %r" % (cfg.get('lambda_boundary'),))
    settings = dict(cfg.get('boundary_settings') or {})
    unknown = sorted(set(settings) - {'classes', 'spacing'})
    if unknown:
        raise ValueError("config['boundary_settings'] takes 'classes' and 'spacing', got %s" % ', '.join(repr(k) for k in unknown))
    if 'n_classes' in cfg:
        BoundaryLoss(cfg['n_classes'], **settings)             # raises for a bad class list / spacing
    return float(lam), settings


def boundary_name_suffix(cfg):
    """'_boundary<lambda>' for an experiment name when the term is on, '' otherwise (names of runs without it stay as they were)."""
    lam = cfg.get('lambda_boundary') or 0.0
    return '_boundary%s' % lam if lam > 0 else ''


PATCH_DEFAULTS = {'size': None, 'mode': 'balanced', 'threshold': 0.01, 'classes': None, 'per_volume': 1, 'overlap': [8, 8, 8], 'tile_batch': 4,
                  'include_last': False}


def parse_patch(spec):
    """config['patch'] -> None (off) or the full dict {'size': [d, h, w], 'mode': 'balanced' | 'random', 'threshold': a float or a list (the
    crops' thresholds), 'classes': None or a list of labels, 'per_volume': patches cropped from one volume, 'overlap': [d, h, w] of the
    evaluation tiles, 'tile_batch': tiles per forward pass, 'include_last': the crop domain}.  Sizes are (z, y, x), like synthetic_shape; only
    'size' is required.  The geometry against the nets and the volumes is checked at setup (nifti_data.check_shapes)."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError("config['patch'] must be None or a dict, got %r" % (spec,))
    unknown = sorted(set(spec) - set(PATCH_DEFAULTS))
    if unknown:
        raise ValueError("config['patch'] takes %s, got %s" % (sorted(PATCH_DEFAULTS), ', '.join(repr(k) for k in unknown)))
    out = dict(PATCH_DEFAULTS)
    out.update({k: v for k, v in spec.items() if v is not None or k == 'classes'})
    for key in ('size', 'overlap'):
        v = out[key]
        if v is None or len(v) != 3 or any(int(a) != a for a in v):
            raise ValueError("config['patch'][%r] takes three integers (z, y, x), got %r" % (key, v))
        out[key] = [int(a) for a in v]
    if min(out['size']) < 1 or min(out['overlap']) < 0:
        raise ValueError("config['patch']: size must be positive and overlap >= 0, got %r and %r" % (out['size'], out['overlap']))
    if out['mode'] not in ('balanced', 'random'):
        raise ValueError("config['patch']['mode'] %r: 'balanced' or 'random'" % (out['mode'],))
    for key in ('per_volume', 'tile_batch'):
        if isinstance(out[key], bool) or int(out[key]) != out[key] or int(out[key]) < 1:
            raise ValueError("config['patch'][%r] must be an integer >= 1, got %r" % (key, out[key]))
        out[key] = int(out[key])
    out['threshold'] = [float(t) for t in out['threshold']] if np.ndim(out['threshold']) else float(out['threshold'])
    out['classes'] = None if out['classes'] is None else list(out['classes'])
    out['include_last'] = bool(out['include_last'])
    return out


def refuse_patch(cfg, what):
    """Patch training is the segmentation experiment's alone: the `what` experiment raises when given config['patch']."""
    if cfg.get('patch') is not None:
        raise ValueError("config['patch'] (patch training and tiled evaluation) is not implemented for the %s experiment" % what)


def patch_name_suffix(cfg):
    """'_patch<d>x<h>x<w>' for an experiment name in patch mode, '' otherwise (names of runs without it stay as they were)."""
    patch = cfg.get('patch')
    return '_patch%s' % 'x'.join(str(int(v)) for v in patch['size']) if patch is not None else ''


class SegmentationExperiment(BaseExperiment):
    def __init__(self, config):
        super(SegmentationExperiment, self).__init__(config)
        self.device = torch.device(self.config.get('device', 'cuda'))
        cfg = self.config
        if cfg['debug_mode']:                                    # debug runs print and validate every second batch / epoch
            print("Debug mode")
            cfg['print_batch_period'] = cfg['valid_epoch_period'] = 2
        self.lambda_boundary, self.boundary_settings = check_boundary_term(cfg)
        self.boundary_criterion = None
        self.last_boundary = None                                # the step's boundary term (a device scalar) when the term is on
        self.patch = parse_patch(cfg.get('patch'))
        self.crop = self.partition = None
        if self.patch is not None:
            self.setup_patch()
        self.tile_blend = inference.parse_tile_blend(cfg.get('tile_blend'), self.patch)
        self.predictor = None                                    # the SlidingWindowPredictor of config['tile_blend'], built on first use
        self.exp_name = self.experiment_name(cfg)
        # <log_dir>/<experiment name | "debug_seg">/<seed>: the directory layout the reference's checkpoints and resume_dir use
        # (models/segmentation.py:40-42), so runs of either code base can resume each other's checkpoints
        run_dir = "debug_seg" if cfg['debug_mode'] else self.exp_name
        self.ckpoint_dir = os.path.join(cfg['log_dir'], run_dir, str(cfg['random_seed']))
        self.writer = None
        self.global_step = 0
        self.training_data_loader = self.config.get('training_data_loader')
        self.validation_data_loader = self.config.get('validation_data_loader')
        # optional training-batch augmentation, config['augment'] = [['rigid', {...}], ['bspline', {...}]] (lib/transforms.py:161-259)
        self.augment = med_transforms.make_augmentation(self.config.get('augment'))
        print("Init experiment {} seed {}".format(self.exp_name, self.config['random_seed']))

    @staticmethod
    def experiment_name(cfg):
        """The run's name, field by field as the reference composes it (models/segmentation.py:27-38) -- it is part of the checkpoint path:
        Seg_<model>[_bias][_BN]_<data dir name>_<n>samples_batch_<b>_<e>epochs_<loss>_<weighting>_lr_<lr>[_scheduler_<mode>][_boundary<lambda_boundary>]
        [_patch<d>x<h>x<w>]."""
        ms = cfg['model_settings']
        parts = ['Seg_', cfg['model']]
        if ms['bias']:
            parts.append('_bias')
        if ms['BN']:
            parts.append('_BN')
        parts += ['_', os.path.basename(cfg['data_dir']),
                  '_%ssamples' % cfg['num_samples'], '_batch_%s' % cfg['batch_size'], '_%sepochs' % cfg['n_epochs'],
                  '_%s_%s' % (cfg['loss'], cfg['loss_settings']['weight_type']), '_lr_%s' % cfg['learning_rate']]
        if cfg['lr_mode'] != 'const':
            parts.append('_scheduler_%s' % cfg['lr_mode'])
        parts.append(boundary_name_suffix(cfg))
        parts.append(patch_name_suffix(cfg))
        return ''.join(str(v) for v in parts)

    # ---- setup ---------------------------------------------------------------------------------
    def setup_patch(self):
        """The crop transform of the training batches and the tiling of the evaluation volumes, from config['patch'] ((z, y, x) sizes are
        flipped to the (x, y, z) the two classes take)."""
        cfg, patch = self.config, self.patch
        if cfg['batch_size'] % patch['per_volume'] != 0:
            raise ValueError("config['batch_size'] = %d patches is no multiple of config['patch']['per_volume'] = %d"
                             % (cfg['batch_size'], patch['per_volume']))
        if cfg['model_settings'].get('in_channel', 1) != 1:
            raise ValueError("config['patch']: the tiled evaluation takes single-channel images")
        nifti_data.check_patch(patch, [cfg['model']])
        size_xyz = tuple(int(v) for v in reversed(patch['size']))
        if patch['mode'] == 'random':
            self.crop = med_transforms.BalancedRandomCrop(size_xyz, threshold=0.0, classes=[None], patches=patch['per_volume'],
                                                          include_last=patch['include_last'])
        else:
            thr = patch['threshold']
            if patch['classes'] is None:
                thr = tuple(thr) if isinstance(thr, list) else float(thr)
            self.crop = med_transforms.BalancedRandomCrop(size_xyz, threshold=thr, classes=patch['classes'], patches=patch['per_volume'],
                                                          include_last=patch['include_last'])
        self.partition = med_transforms.Partition(size_xyz, tuple(int(v) for v in reversed(patch['overlap'])))

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
        dataset = med_data.get_seg_dataset(self.config['data'])
        shape = self.config['synthetic_shape']
        if self.patch is not None and any(int(v) < w for v, w in zip(shape, self.patch['size'])):
            raise ValueError('the synthetic volumes %s are smaller than the patch %s on some axis'
                             % ('x'.join(str(int(v)) for v in shape), 'x'.join(str(w) for w in self.patch['size'])))
        training_data = dataset(self.config["num_samples"] * 2, shape, self.config['n_classes'], seed=self.config['random_seed'])
        sampler = parallel.distributed_sampler(training_data, shuffle=True, seed=self.config['random_seed'])
        self.training_data_loader = DataLoader(training_data, batch_size=self.config['batch_size'] if self.patch is None else 1,
                                               shuffle=sampler is None, sampler=sampler, num_workers=0)
        validation_data = dataset(self.config.get('num_valid_samples', 2), shape, self.config['n_classes'],
                                  seed=self.config['random_seed'] + 1000)
        self.validation_data_loader = DataLoader(validation_data, batch_size=1, shuffle=False, num_workers=0)

    def setup_nifti_data(self):
        """models/segmentation.py:54-79, 241-251: the training list's first num_samples * 2 scans, the validation and test lists whole; every
        prepared volume must have the one shape the net accepts (nifti_data.check_shapes raises otherwise).  With config['patch'] the volumes may
        differ in shape (each must hold a patch) and the training loader yields one volume at a time."""
        cfg = self.config
        training_data = nifti_data.seg_dataset(cfg, 'training_list_file', 'data_dir', n_samples=cfg['num_samples'] * 2)
        validation_data = nifti_data.seg_dataset(cfg, 'validation_list_file', 'valid_data_dir')
        testing_data = nifti_data.seg_dataset(cfg, 'testing_list_file', 'valid_data_dir')
        if training_data is None or validation_data is None:
            raise ValueError("config['data'] = %r needs config['training_list_file'] and config['validation_list_file']" % (cfg['data'],))
        nifti_data.check_shapes([training_data, validation_data, testing_data], [cfg['model']], patch=self.patch)
        sampler = parallel.distributed_sampler(training_data, shuffle=True, seed=cfg['random_seed'])
        self.training_data_loader = DataLoader(training_data, batch_size=cfg['batch_size'] if self.patch is None else 1, shuffle=sampler is None,
                                               sampler=sampler, num_workers=0)
        self.validation_data_loader = DataLoader(validation_data, batch_size=1, shuffle=False, num_workers=0)
        if testing_data is not None:
            self.testing_data_loader = DataLoader(testing_data, batch_size=1, shuffle=False, num_workers=0)

    def setup_model(self):
        model_type = get_network(self.config['model'])
        self.model = model_type(**self.config['model_settings'])
        self.model.to(self.device)
        # softmax-Dice training (train_seg.py:55): the output convolution is evaluated inside the fused head + softmax + Dice kernels
        # (ops.HeadDiceFn) and the logits tensor is only built on demand (train_step's `output`.materialize(), eval mode)
        # (with the boundary term on, the logits feed two losses: they are materialised once and the head is not fused)
        if (self.config.get('fuse_head_dice', True) and self.config.get('loss') == 'dice' and not self.lambda_boundary > 0
                and self.config.get('loss_settings', {}).get('softmax') and hasattr(type(self.model), 'lazy_head')):
            self.model.lazy_head = True

    def setup_loss(self):
        self.criterion = get_loss_function(self.config['loss'])(**self.config['loss_settings']).to(self.device)
        if self.lambda_boundary > 0:
            self.boundary_criterion = BoundaryLoss(self.config['n_classes'], **self.boundary_settings).to(self.device)

    def setup_optimizer(self):
        """models/segmentation.py:90-111: Adam + plateau / multiStep / const."""
        self.optimizer = FlatAdam(self.model.parameters(), lr=self.config['learning_rate'])
        # conv weight gradients on a second stream, accumulated into the optimiser's flat bucket (joined in zero_grad / step)
        ops.enable_async_wgrad(bool(self.config.get('async_wgrad', True)))
        # matrix mode of the 3x3x3 convolutions: 'fp32_split' (default, and what bench.py measures: two-term fp16 split per staged tile, 22-bit
        # products on the fp16 matrix pipe -- per product narrower than fp32, bounds in csrc/split_f16.h), 'fp32' (the fp32 matrix instructions:
        # the reference's arithmetic; pass matrix_precision='fp32' for that) or 'bf16' (operands rounded, BASELINE config 5)
        ops.set_matrix_precision(self.config.get('matrix_precision') or ops.DEFAULT_MATRIX_PRECISION)
        self.scheduler = self.make_scheduler(self.optimizer, self.config)

    @staticmethod
    def make_scheduler(optimizer, cfg):
        """Learning-rate schedule of the reference (models/segmentation.py:93-111).  'plateau': x 0.2 when the validation score (maximised)
        has not improved by 0.003 (absolute) for 100 epochs' worth of validations, never below 1e-5.  'multiStep': x gamma at the given
        fractions of n_epochs (the config's `milestones` are replaced by the epoch numbers, as the reference does).  Anything else: constant."""
        mode = cfg['lr_mode']
        if mode == 'plateau':
            validations = 100 // cfg['valid_epoch_period']
            return lr_scheduler.ReduceLROnPlateau(optimizer, mode='max', factor=0.2, patience=validations, threshold=0.003, threshold_mode='abs', min_lr=1e-5)
        if mode == 'multiStep':
            cfg['milestones'] = [int(frac * cfg['n_epochs']) for frac in cfg['milestones']]
            return lr_scheduler.MultiStepLR(optimizer, cfg['milestones'], gamma=cfg['gamma'])
        return None

    # ---- training ------------------------------------------------------------------------------
    def train(self):
        self.setup_train()
        print("Training {}".format(self.exp_name))
        finished_epoch, self.best_score = self.initialize_model(self.model, self.optimizer, self.config['resume_dir'])
        parallel.broadcast_parameters(self.optimizer, model=self.model)
        parallel.pin_host_resources()                 # per-rank core slice + gc.freeze(): the host launch loop is the DP scaling risk
        self.current_epoch = finished_epoch + 1
        for epoch in range(self.current_epoch, self.config['n_epochs'] + 1):
            self.train_one_epoch()
            self.validate()
            self.current_epoch += 1
        if self.writer is not None:
            self.writer.close()
        print('Finished Training: {}'.format(self.exp_name))

    def train_step(self, images, truths):
        """One optimisation step (models/segmentation.py:141-157)."""
        self.model.train()
        with trace.range('seg/zero_grad'):
            self.optimizer.zero_grad()
        with trace.range('seg/forward'):
            output = self.model(images.to(self.device, non_blocking=True))
        with trace.range('seg/loss'):
            truths = truths.to(self.device, non_blocking=True)
            loss = self.criterion(output, truths)
            if self.boundary_criterion is not None:
                boundary = self.boundary_criterion(output, truths)
                self.last_boundary = boundary.detach()
                loss = loss + self.lambda_boundary * boundary
        with trace.range('seg/backward'):
            loss.backward()
        with trace.range('seg/allreduce'):
            parallel.allreduce_gradients(self.optimizer)
        with trace.range('seg/adam'):
            self.optimizer.step()
        return loss, output

    def augment_batch(self, images, truths):
        """config['augment']'s transforms, in order, on the device, to one training batch (N x 1 x D x H x W, N x D x H x W).  Validation
        and test batches are never augmented."""
        sample = {'image': images.to(self.device, non_blocking=True), 'segmentation': truths.to(self.device, non_blocking=True)}
        for t in self.augment:
            sample = t(sample)
        return sample['image'], sample['segmentation']

    def patch_batch(self, train_data_iter):
        """config['batch_size'] patches: per_volume crops from each of batch_size / per_volume volumes, drawn from the loader one after another
        (a loader may hand over several volumes of one shape at once).  Returns (images, truths, the loader's iterator)."""
        need = self.config['batch_size'] // self.patch['per_volume']
        imgs, segs, have = [], [], 0
        while have < need:
            try:
                images, truths, name = next(train_data_iter)
            except (StopIteration, TypeError):
                train_data_iter = iter(self.training_data_loader)
                images, truths, name = next(train_data_iter)
            images, truths = images[:need - have], truths[:need - have]
            out = self.crop({'image': images.to(self.device, non_blocking=True), 'segmentation': truths.to(self.device, non_blocking=True)})
            imgs.append(out['image'])
            segs.append(out['segmentation'])
            have += int(images.shape[0])
        return (imgs[0], segs[0], train_data_iter) if len(imgs) == 1 else (torch.cat(imgs, 0), torch.cat(segs, 0), train_data_iter)

    def train_one_epoch(self):
        running_loss = running_boundary = 0.0
        iters_per_epoch = max(self.config['samples_per_epoch'] // (self.config['batch_size'] * parallel.world_size()), 1)
        train_data_iter = None
        for i in range(iters_per_epoch):
            if self.patch is not None:
                images, truths, train_data_iter = self.patch_batch(train_data_iter)
            else:
                try:
                    images, truths, name = next(train_data_iter)
                except (StopIteration, TypeError):
                    train_data_iter = iter(self.training_data_loader)
                    images, truths, name = next(train_data_iter)
            self.global_step = (self.current_epoch - 1) * iters_per_epoch + (i + 1) * self.config['batch_size']
            if self.augment:
                images, truths = self.augment_batch(images, truths)
            loss, output = self.train_step(images, truths)
            running_loss += loss.item()
            if self.boundary_criterion is not None:
                running_boundary += self.last_boundary.item()
            if i % self.config['print_batch_period'] == self.config['print_batch_period'] - 1:
                if parallel.rank() == 0:
                    print('Epoch[{}/{}] it {} loss: {:.3f}{} lr:{} {}'.format(
                        self.current_epoch, self.config['n_epochs'], i + 1,
                        running_loss / self.config['print_batch_period'] if i > 0 else running_loss,
                        '' if self.boundary_criterion is None else ' boundary: {:.4f}'.format(
                            running_boundary / self.config['print_batch_period'] if i > 0 else running_boundary),
                        self.optimizer.param_groups[0]['lr'], datetime.datetime.now().strftime("%D %H:%M:%S")))
                    if self.writer is not None:
                        self.writer.add_scalar('loss/training', running_loss / self.config['print_batch_period'], global_step=self.global_step)
                        self.writer.add_scalar('learning_rate', self.optimizer.param_groups[0]['lr'], global_step=self.global_step)
                running_loss = running_boundary = 0.0

    def predict_tiled(self, images):
        """Label maps N x D x H x W (uint8) of a batch N x 1 x D x H x W in patch mode: per volume Partition's reflect-padded overlap tiles of
        the patch size, the net over chunks of tile_batch tiles, the first-max argmax of every tile, and assemble's core copy.
        With config['tile_blend'] the tiles' probabilities are blended instead (lib/inference.py SlidingWindowPredictor)."""
        if getattr(self, 'tile_blend', None) is not None:
            if self.predictor is None or self.predictor.model is not self.model:
                self.predictor = inference.SlidingWindowPredictor(self.model, self.config['n_classes'], self.patch['size'], self.patch['overlap'],
                                                                  tile_batch=self.patch['tile_batch'], **self.tile_blend)
            return self.predictor.predict_batch(images)
        out = []
        tb = self.patch['tile_batch']
        for n in range(images.shape[0]):
            vol = images[n, 0]
            tiles = self.partition({'image': vol, 'segmentation': vol})['image']                     # T x 1 x tz x ty x tx
            blank = torch.zeros((min(tb, tiles.shape[0]),) + tuple(tiles.shape[2:]), dtype=torch.uint8, device=tiles.device)
            labs = []
            for k in range(0, tiles.shape[0], tb):
                logits = self.model(tiles[k:k + tb])
                labs.append(metrics.eval_dice_counts(logits, blank[:logits.shape[0]])[1])
            out.append(self.partition.assemble(torch.cat(labs, 0)))
        return torch.stack(out, 0)

    def eval(self, dataloader):
        """models/segmentation.py:179-201; Dice from exact integer counts computed on the device.
        With config['patch'] the label map of a volume is predict_tiled's (tiles, net, argmax, assemble) and the counts are
        ops.label_overlap_counts of it; everything below acts on that map as it acts on the whole-volume argmax.
        With config['postprocess'] set (lib/evalMetrics.py parse_postprocess: 'largest_cc', or a dict with mode / connectivity / min_size) the
        argmax label map is additionally cleaned on the device (ops.keep_largest_component / remove_small_components) and scored again; those
        numbers go to self.eval_extra (post_dice_per_class, post_dice_avg, components_per_class, removed_frac).  The return value, and with it
        model selection, the scheduler and best_score, stay on the raw Dice.
        With config['surface_metrics'] set (lib/evalMetrics.py parse_surface_metrics: True, or a dict with spacing / connectivity / percentile /
        classes) the argmax label map is also scored by its surface distances on the device (ops.surface_distance_stats): self.eval_extra
        gains hd95_per_class, assd_per_class, hd_per_class (NaN-means over the volumes), hd95_avg and assd_avg (NaN-means over the classes)
        and surface_undefined_frac (the share of (volume, class) pairs without a defined distance); with `postprocess` as well, the same for
        the cleaned map under post_*.  The return value does not change."""
        post = metrics.parse_postprocess(self.config.get('postprocess'))
        surf = metrics.parse_surface_metrics(self.config.get('surface_metrics'))
        surf_raw, surf_post = [], []                                               # per batch: the dicts of metrics.surface_distances
        n_class = self.config["n_classes"]
        tiled = getattr(self, 'patch', None) is not None                           # (the joint experiment borrows this method for a view without it)
        self.eval_extra = {}
        with torch.no_grad():
            self.model.eval()
            dice_per_class = torch.zeros(n_class - 1, dtype=torch.float64)
            post_dice = torch.zeros(n_class - 1, dtype=torch.float64)
            components = np.zeros(n_class - 1, dtype=np.float64)
            kept = total = 0
            n_vol = 0
            pred = images = truths = None
            for j, (images, truths, name) in enumerate(dataloader):
                if tiled:
                    truth = truths.to(self.device)
                    lab = self.predict_tiled(images.to(self.device))
                    counts = ops.label_overlap_counts(lab, truth, n_class)
                    d = metrics.dice_from_counts(counts)[:, 1:]
                    if surf is not None:
                        surf_raw.append(metrics.surface_distances(lab, truth, n_class, **surf))
                    pred = lab
                elif post is None and surf is None:
                    pred = self.model(images.to(self.device))
                    d = metrics.metricEval('dice', pred, truths.to(self.device))   # [N][C-1]
                else:
                    pred = self.model(images.to(self.device))
                    truth = truths.to(self.device)
                    counts, lab = metrics.eval_dice_counts(pred, truth)            # the counts metricEval('dice', ...) is computed from
                    d = metrics.dice_from_counts(counts)[:, 1:]
                    if surf is not None:
                        surf_raw.append(metrics.surface_distances(lab, truth, n_class, **surf))
                if post is not None:
                    clean, stats = metrics.postprocess_labels(lab, n_class, post, return_stats=True)
                    pc = ops.label_overlap_counts(clean, truth, n_class)
                    post_dice += torch.from_numpy(metrics.dice_from_counts(pc)[:, 1:].sum(0))
                    components += stats[:, 1:, 0].sum(0).cpu().numpy()
                    kept += int(pc[:, 1:, 0].sum())
                    total += int(counts[:, 1:, 0].sum())
                    if surf is not None:
                        surf_post.append(metrics.surface_distances(clean, truth, n_class, **surf))
                dice_per_class += torch.from_numpy(d.sum(0))
                n_vol += d.shape[0]                                                # average over VOLUMES (loaders may batch > 1)
            dice_per_class = (dice_per_class / max(n_vol, 1)).float()
            dice_avg = dice_per_class.mean()
            if post is not None:
                post_dice = (post_dice / max(n_vol, 1)).float()
                self.eval_extra = {'post_dice_per_class': post_dice, 'post_dice_avg': post_dice.mean(),
                                   'components_per_class': components / max(n_vol, 1),      # per class, averaged over the volumes
                                   'removed_frac': (total - kept) / float(total) if total else 0.0}
            if surf_raw:
                self.eval_extra.update(self._surface_summary(surf_raw, ''))
            if surf_post:
                self.eval_extra.update(self._surface_summary(surf_post, 'post_'))
            sample_for_vis = {'img': images, 'truth': truths, 'pred': pred}
        return dice_per_class, dice_avg, sample_for_vis

    @staticmethod
    def _surface_summary(batches, prefix):
        """The eval_extra entries of one label map's surface distances: `batches` = metrics.surface_distances of every batch."""
        cols = {k: np.concatenate([b[k] for b in batches], 0) for k in ('hd_pct', 'assd', 'hd')}       # [volumes][K']

        def nanmean(a, axis=None):                                                 # (np.nanmean warns on an all-NaN slice)
            ok = ~np.isnan(a)
            with np.errstate(invalid='ignore', divide='ignore'):
                return np.where(ok, a, 0.0).sum(axis) / ok.sum(axis)
        out = {prefix + 'hd95_per_class': nanmean(cols['hd_pct'], 0), prefix + 'assd_per_class': nanmean(cols['assd'], 0),
               prefix + 'hd_per_class': nanmean(cols['hd'], 0)}
        out[prefix + 'hd95_avg'] = float(nanmean(out[prefix + 'hd95_per_class']))
        out[prefix + 'assd_avg'] = float(nanmean(out[prefix + 'assd_per_class']))
        out[prefix + 'surface_undefined_frac'] = float(np.isnan(cols['assd']).mean())
        return out

    def _surface_suffix(self):
        """', HD95 Avg: x.xx, ASSD Avg: x.xx' after an eval with config['surface_metrics'], else ''."""
        extra = getattr(self, 'eval_extra', None) or {}
        if 'hd95_avg' not in extra:
            return ''
        return ', HD95 Avg: {:.2f}, ASSD Avg: {:.2f}'.format(extra['hd95_avg'], extra['assd_avg'])

    def _post_suffix(self):
        """', post-processed Dice Avg: x.xxxx (n.n components / class)' after an eval with config['postprocess'] (followed by the cleaned
        map's ', HD95 Avg: x.xx, ASSD Avg: x.xx' with config['surface_metrics'] as well), else ''."""
        extra = getattr(self, 'eval_extra', None) or {}
        if 'post_dice_avg' not in extra:
            return ''
        text = ', post-processed Dice Avg: {:.4f} ({:.1f} components / class)'.format(float(extra['post_dice_avg']),
                                                                                     float(np.mean(extra['components_per_class'])))
        if 'post_hd95_avg' in extra:
            text += ', HD95 Avg: {:.2f}, ASSD Avg: {:.2f}'.format(extra['post_hd95_avg'], extra['post_assd_avg'])
        return text

    def validate(self):
        if self.current_epoch % self.config['valid_epoch_period'] == 0:
            start_time = time.time()
            dice_per_class, dice_avg, samples = self.eval(self.validation_data_loader)
            if self.scheduler is not None:
                if self.config['lr_mode'] == 'plateau':
                    self.scheduler.step(dice_avg)
                else:
                    self.scheduler.step()
            is_best = False
            if dice_avg > self.best_score:
                is_best = True
                self.best_score = dice_avg
            if parallel.rank() != 0:
                return
            if self.writer is not None:
                self.writer.add_scalar('validation_{}/dice_avg'.format(self.config['data']), dice_avg, global_step=self.global_step)
            print("Validation: Dice Avg: {:.4f} ({:.3f} sec) {}{}".format(float(dice_avg), time.time() - start_time,
                                                                           datetime.datetime.now().strftime("%D %H:%M:%S"), self._surface_suffix() + self._post_suffix()))
            if self.current_epoch % self.config['save_ckpts_epoch_period'] == 0:
                self.save_checkpoint({'epoch': self.current_epoch,
                                      'model_state_dict': self.model.state_dict(),
                                      'optimizer_state_dict': self.optimizer.state_dict(),
                                      'best_score': self.best_score},
                                     is_best, self.ckpoint_dir)

    def test(self, best=True, if_log=True):
        """models/segmentation.py:253-274: reload the best checkpoint and report Dice on the test loader."""
        self.setup_model()
        ckpoint_file = os.path.join(self.ckpoint_dir, 'model_best.pth.tar' if best else 'checkpoint.pth.tar')
        last_epoch, best_score = self.initialize_model(self.model, optimizer=None, ckpoint_path=ckpoint_file)
        if self.validation_data_loader is None and nifti_data.is_nifti(self.config):        # test only: the loaders were never built
            self.setup_train_data()
        loader = self.config.get('testing_data_loader') or getattr(self, 'testing_data_loader', None) or self.validation_data_loader
        dice_per_class, dice_avg, samples = self.eval(loader)
        print('Testing Model: {} ({} epochs)  Dice_avg: {}{}'.format(ckpoint_file, last_epoch, float(dice_avg), self._surface_suffix() + self._post_suffix()))
        return dice_per_class, dice_avg
