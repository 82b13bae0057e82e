"""DeepAtlasExperiment: joint training of the registration and the segmentation net from few labelled volumes -- what the reference
names as its goal and lists as TODO (README.md:15-19).

Two models, two FlatAdams, step = models/joint.py DeepAtlasJointStep (unchanged; weights lam_sim / lam_reg / lam_anat / lam_sp from the
config).  `num_labeled` of the training volumes -- the first k after a shuffle seeded with random_seed -- have a manual segmentation; a
pair whose moving volume is unlabelled reaches the step as seg_m=None (the registration phase then warps the segmentation net's own
prediction and the segmentation phase has no supervised term).  config['pairs'] chooses the enumeration (lib/datasets.py
SyntheticRegDataset): 'fixed_labeled' (default) leaves out the pairs whose fixed volume is unlabelled; 'any_labeled' adds those with a labelled
moving volume, which reach the step as seg_t=None (the warped manual label is the fixed image's pseudo-label); 'all' adds the pairs with no
label on either side (both None: image similarity and smoothness only, the segmentation net is not touched; single process only).  The DeepAtlas
recipe pre-trains each net alone: config['seg_resume_dir'] / config['reg_resume_dir'] name checkpoint files of SegmentationExperiment /
RegistrationExperiment to start from.  Validation = segmentation Dice exactly as SegmentationExperiment.eval computes it + the
registration metrics of models/registration.py.  Two checkpoint files per save, seg_checkpoint.pth.tar / reg_checkpoint.pth.tar (and
seg_ / reg_model_best.pth.tar, each with its own best flag), carrying seg_best_score / reg_best_score: the keys models/base.py:96-101
reads.  config['resume_dir'] is the directory that holds the two checkpoint files: both nets and both optimisers are restored.
config['atlas_fusion'] ('majority' | 'local', default None: off) adds the registration net's score as a segmenter: every validation volume is
segmented from the labelled training volumes by multi-atlas label fusion (models/registration.py eval_atlas_fusion), reported as atlas_dice_*.
config['sim_loss'] / config['sim_settings'] / config['moving_remap']: the image similarity of the registration phase and the synthetic pairs'
moving-image remap, as in models/registration.py; so are config['lambda_jac'] / config['jac_settings'], the Jacobian folding penalty of the
registration phase (default 0: off).
config['data'] other than 'synthetic' (models/nifti_data.py) trains on the NIfTI volumes of a list file; the labelled volumes are then the first
num_labeled names of the training list.
"""
import datetime
import os
import random
import time

import torch
from torch.utils.data import DataLoader

from .base import BaseExperiment
from . import nifti_data
from .joint import DeepAtlasJointStep
from .registration import (atlas_fusion_text, check_atlas_fusion, check_jac_penalty, check_sim_loss, dataset_volumes, eval_atlas_fusion,
                           eval_registration, jac_name_suffix, refuse_refine)
from .segmentation import SegmentationExperiment, refuse_patch
from ..lib.inference import refuse_tile_blend
from ..lib import datasets as med_data
from ..lib.network_factory import get_network
from ..lib.param_dict import save_dict_to_json
from ..optim import FlatAdam
from .. import ops
from .. import parallel

try:
    from tensorboardX import SummaryWriter
except Exception:                                             # tensorboardX is optional here
    SummaryWriter = None


class _SegEvalView(object):
    """What SegmentationExperiment.eval reads of its experiment: the segmentation Dice here is that method, not a restatement."""

    def __init__(self, model, config, device):
        self.model, self.config, self.device = model, config, device


class DeepAtlasExperiment(BaseExperiment):
    def __init__(self, config):
        super(DeepAtlasExperiment, self).__init__(config)
        self.device = torch.device(self.config.get('device', 'cuda'))
        cfg = self.config
        refuse_patch(cfg, 'joint')
        refuse_tile_blend(cfg, 'joint')
        refuse_refine(cfg, 'joint')
        if cfg['debug_mode']:
            print("Debug mode")
            cfg['print_batch_period'] = cfg['valid_epoch_period'] = 2
        if cfg['batch_size'] != 1:
            raise ValueError('DeepAtlasExperiment trains one pair per step (labelled and unlabelled moving volumes cannot share a batch)')
        if cfg['num_labeled'] < 1:
            raise ValueError('joint training needs at least one labelled volume (the fixed image of every pair)')
        pairs = cfg.get('pairs', 'fixed_labeled')
        if pairs not in med_data.SyntheticRegDataset.PAIR_MODES:
            raise ValueError("config['pairs'] must be one of %s, got %r" % (', '.join(med_data.SyntheticRegDataset.PAIR_MODES), pairs))
        if pairs == 'all' and parallel.world_size() > 1:
            raise ValueError("pairs='all' needs a single process: a rank whose pair has no label skips its segmentation phase and would miss the "
                             "gradient all-reduce the other ranks enter")
        nifti_data.refuse_synthetic_only(cfg, ('misalign', 'report_tre'))
        self.atlas_fusion, self.atlas_fusion_max = check_atlas_fusion(cfg)
        self.sim_loss, self.sim_settings = check_sim_loss(cfg)
        self.lambda_jac, self.jac_settings = check_jac_penalty(cfg)
        self.exp_name = self.experiment_name(cfg)
        run_dir = "debug_joint" if cfg['debug_mode'] else self.exp_name
        self.ckpoint_dir = os.path.join(cfg['log_dir'], run_dir, str(cfg['random_seed']))
        self.writer = None
        self.global_step = 0
        self.current_epoch = 1
        self.seg_best_score = self.reg_best_score = 0
        self.training_data_loader = self.config.get('training_data_loader')
        self.validation_data_loader = self.config.get('validation_data_loader')              # segmentation volumes
        self.validation_pair_loader = self.config.get('validation_pair_loader')              # registration pairs
        print("Init experiment {} seed {}".format(self.exp_name, self.config['random_seed']))

    @staticmethod
    def experiment_name(cfg):
        """Joint_<seg model>_<reg model>_<data dir name>_<n>samples_<k>labeled_<e>epochs_sim<..>_reg<..>_anat<..>_sp<..>_lr_<lr>[_scheduler_<mode>][_pairs<mode>][_<sim_loss>][_moving<remap>][_jac<lambda_jac>]"""
        parts = ['Joint_', cfg['model'], '_', cfg['reg_model'], '_', os.path.basename(cfg['data_dir']), '_%ssamples' % cfg['num_samples'],
                 '_%slabeled' % cfg['num_labeled'], '_%sepochs' % cfg['n_epochs'],
                 '_sim%s_reg%s_anat%s_sp%s' % (cfg['lambda_sim'], cfg['lambda_reg'], cfg['lambda_anat'], cfg['lambda_sp']), '_lr_%s' % cfg['learning_rate']]
        if cfg['lr_mode'] != 'const':
            parts.append('_scheduler_%s' % cfg['lr_mode'])
        if cfg.get('pairs', 'fixed_labeled') != 'fixed_labeled':
            parts.append('_pairs%s' % cfg['pairs'])
        if (cfg.get('sim_loss') or 'ncc') != 'ncc':
            parts.append('_%s' % cfg['sim_loss'])
        if cfg.get('moving_remap'):
            parts.append('_moving%s' % cfg['moving_remap'])
        parts.append(jac_name_suffix(cfg))
        return ''.join(str(v) for v in parts)

    @staticmethod
    def labeled_subset(n_volumes, num_labeled, seed):
        """The volumes that have a manual segmentation: the first `num_labeled` of range(n_volumes) after a shuffle seeded with `seed`."""
        idx = list(range(n_volumes))
        random.Random(seed).shuffle(idx)
        return sorted(idx[:max(0, min(int(num_labeled), n_volumes))])

    # ---- setup ---------------------------------------------------------------------------------
    def setup_log(self):
        if parallel.rank() != 0:
            return
        if not os.path.isdir(self.ckpoint_dir):
            os.makedirs(self.ckpoint_dir)
        save_dict_to_json(self.config, os.path.join(self.ckpoint_dir, "train_config.json"))
        if SummaryWriter is not None:
            self.writer = SummaryWriter(self.ckpoint_dir)

    def setup_nifti_data(self):
        """Pairs and validation volumes over the reference's list-file datasets (models/nifti_data.py).  The labelled volumes are the first
        num_labeled names of the training list; the validation list feeds both the segmentation and the pair validation."""
        cfg = self.config
        remap = {'moving_remap': cfg['moving_remap']} if cfg.get('moving_remap') else {}
        training_vols = validation_vols = None
        if self.training_data_loader is None:
            training_vols = nifti_data.seg_dataset(cfg, 'training_list_file', 'data_dir', n_samples=max(cfg['num_samples'], 2))
            if training_vols is None:
                raise ValueError("config['data'] = %r needs config['training_list_file']" % (cfg['data'],))
        if self.validation_data_loader is None or self.validation_pair_loader is None:
            validation_vols = nifti_data.seg_dataset(cfg, 'validation_list_file', 'valid_data_dir')
            if validation_vols is None:
                raise ValueError("config['data'] = %r needs config['validation_list_file']" % (cfg['data'],))
        nifti_data.check_shapes([training_vols, validation_vols], [cfg['model'], cfg['reg_model']])
        if training_vols is not None:
            self.labeled = list(range(max(0, min(int(cfg['num_labeled']), len(training_vols)))))
            training_data = med_data.NiftiRegDataset(training_vols, labeled=self.labeled, pairs=cfg.get('pairs', 'fixed_labeled'), **remap)
            sampler = parallel.distributed_sampler(training_data, shuffle=True, seed=cfg['random_seed'])
            self.training_data_loader = DataLoader(training_data, batch_size=1, shuffle=sampler is None, sampler=sampler, num_workers=0)
        if self.validation_data_loader is None:
            self.validation_data_loader = DataLoader(validation_vols, batch_size=1, shuffle=False, num_workers=0)
        if self.validation_pair_loader is None:
            self.validation_pair_loader = DataLoader(med_data.NiftiRegDataset(validation_vols, **remap), batch_size=1, shuffle=False, num_workers=0)

    def setup_train_data(self):
        cfg = self.config
        if nifti_data.is_nifti(cfg):
            return self.setup_nifti_data()
        shape, C = cfg['synthetic_shape'], cfg['n_classes']
        remap = {'moving_remap': cfg['moving_remap']} if cfg.get('moving_remap') else {}
        if self.training_data_loader is None:
            n = max(cfg['num_samples'], 2)
            self.labeled = self.labeled_subset(n, cfg['num_labeled'], cfg['random_seed'])
            training_data = med_data.get_reg_dataset(cfg['data'])(n, shape, C, seed=cfg['random_seed'], labeled=self.labeled,
                                                                      pairs=cfg.get('pairs', 'fixed_labeled'), **remap)
            sampler = parallel.distributed_sampler(training_data, shuffle=True, seed=cfg['random_seed'])
            self.training_data_loader = DataLoader(training_data, batch_size=1, shuffle=sampler is None, sampler=sampler, num_workers=0)
        n_valid = max(cfg.get('num_valid_samples', 2), 2)
        if self.validation_data_loader is None:
            data = med_data.get_seg_dataset(cfg['data'])(n_valid, shape, C, seed=cfg['random_seed'] + 1000)
            self.validation_data_loader = DataLoader(data, batch_size=1, shuffle=False, num_workers=0)
        if self.validation_pair_loader is None:
            data = med_data.get_reg_dataset(cfg['data'])(n_valid, shape, C, seed=cfg['random_seed'] + 1000, **remap)
            self.validation_pair_loader = DataLoader(data, batch_size=1, shuffle=False, num_workers=0)

    def setup_model(self):
        self.seg_model = get_network(self.config['model'])(**self.config['model_settings']).to(self.device)
        self.reg_model = get_network(self.config['reg_model'])(**self.config.get('reg_model_settings', {})).to(self.device)

    def setup_optimizer(self):
        cfg = self.config
        self.seg_optimizer = FlatAdam(self.seg_model.parameters(), lr=cfg['learning_rate'])
        self.reg_optimizer = FlatAdam(self.reg_model.parameters(), lr=cfg['learning_rate'])
        ops.enable_async_wgrad(bool(cfg.get('async_wgrad', True)))
        ops.set_matrix_precision(cfg.get('matrix_precision') or ops.DEFAULT_MATRIX_PRECISION)
        # (make_scheduler replaces the config's milestone fractions by epoch numbers: hand the second call the fractions again)
        fractions = list(cfg.get('milestones') or [])
        self.seg_scheduler = SegmentationExperiment.make_scheduler(self.seg_optimizer, cfg)
        self.reg_scheduler = SegmentationExperiment.make_scheduler(self.reg_optimizer, dict(cfg, milestones=fractions))
        self.step = DeepAtlasJointStep(self.seg_model, self.seg_optimizer, self.reg_model, self.reg_optimizer, cfg['n_classes'],
                                       lam_sim=cfg['lambda_sim'], lam_reg=cfg['lambda_reg'], lam_anat=cfg['lambda_anat'], lam_sp=cfg['lambda_sp'],
                                       sim_loss=self.sim_loss, sim_settings=self.sim_settings,
                                       lam_jac=self.lambda_jac, jac_settings=self.jac_settings)

    def initialize_models(self):
        """Resume (both nets, both optimisers, from the two files in config['resume_dir']) or start: each net from its pre-training
        checkpoint (config['seg_resume_dir'] / ['reg_resume_dir'], weights only) or from its own weights_init().  Returns the epochs done."""
        cfg = self.config
        if cfg.get('resume_dir'):
            e_s, self.seg_best_score = self.initialize_model(self.seg_model, self.seg_optimizer, os.path.join(cfg['resume_dir'], 'seg_checkpoint.pth.tar'))
            e_r, self.reg_best_score = self.initialize_model(self.reg_model, self.reg_optimizer, os.path.join(cfg['resume_dir'], 'reg_checkpoint.pth.tar'))
            if e_s != e_r:
                raise ValueError('the two checkpoints in %s are from different epochs (%d, %d)' % (cfg['resume_dir'], e_s, e_r))
            return e_s
        self.initialize_model(self.seg_model, None, cfg.get('seg_resume_dir') or None)
        self.initialize_model(self.reg_model, None, cfg.get('reg_resume_dir') or None)
        ops.bump_weights_epoch()
        return 0

    # ---- training ------------------------------------------------------------------------------
    def train(self):
        self.setup_train()
        print("Training {}".format(self.exp_name))
        finished_epoch = self.initialize_models()
        parallel.broadcast_parameters(self.seg_optimizer, model=self.seg_model)
        parallel.broadcast_parameters(self.reg_optimizer, model=self.reg_model)
        parallel.pin_host_resources()
        self.current_epoch = finished_epoch + 1
        for epoch in range(self.current_epoch, self.config['n_epochs'] + 1):
            self.train_one_epoch()
            self.validate()
            self.current_epoch += 1
        if self.writer is not None:
            self.writer.close()
        print('Finished Training: {}'.format(self.exp_name))

    def train_step(self, batch):
        """One joint step on a (moving image, fixed image, moving seg, fixed seg, has_moving_seg, name[, has_fixed_seg]) batch of one pair.
        Returns the step's dict of loss terms; for an unlabelled moving volume (seg_m=None) it has no supervised term 'sup'.  An unlabelled
        fixed volume (the seventh element, present in the wider pair modes) reaches the step as seg_t=None."""
        im_m, im_t, seg_m, seg_t, has = batch[:5]
        d = self.device
        labelled = bool(torch.as_tensor(has).all())
        fixed_labelled = bool(torch.as_tensor(batch[6]).all()) if len(batch) > 6 else True
        out = self.step(im_m.to(d, non_blocking=True), im_t.to(d, non_blocking=True), seg_m.to(d, non_blocking=True) if labelled else None,
                        seg_t.to(d, non_blocking=True) if fixed_labelled else None)
        if not labelled:
            out.pop('sup', None)
        return out

    def train_one_epoch(self):
        running = {'loss_reg': 0.0, 'loss_seg': 0.0}
        if self.step.jac is not None:
            running['jac'] = 0.0                   # the folding penalty of the registration phase, logged only when it is on
        iters_per_epoch = max(self.config['samples_per_epoch'] // parallel.world_size(), 1)
        train_data_iter = None
        period = self.config['print_batch_period']
        for i in range(iters_per_epoch):
            try:
                batch = next(train_data_iter)
            except (StopIteration, TypeError):
                train_data_iter = iter(self.training_data_loader)
                batch = next(train_data_iter)
            self.global_step = (self.current_epoch - 1) * iters_per_epoch + (i + 1)
            out = self.train_step(batch)
            for k in running:
                running[k] += out[k].item()
            if i % period == period - 1:
                if parallel.rank() == 0:
                    div = period if i > 0 else 1
                    jac_text = ' jac: {:.3e}'.format(running['jac'] / div) if 'jac' in running else ''
                    print('Epoch[{}/{}] it {} reg loss: {:.3f} seg loss: {:.3f}{} lr:{} {}'.format(
                        self.current_epoch, self.config['n_epochs'], i + 1, running['loss_reg'] / div, running['loss_seg'] / div, jac_text,
                        self.seg_optimizer.param_groups[0]['lr'], datetime.datetime.now().strftime("%D %H:%M:%S")))
                    if self.writer is not None:
                        for k in running:
                            self.writer.add_scalar('loss/training_' + k, running[k] / period, global_step=self.global_step)
                running = {k: 0.0 for k in running}

    def eval(self, seg_loader=None, pair_loader=None):
        """{'seg_dice_per_class', 'seg_dice_avg'} exactly as SegmentationExperiment.eval computes them + the dict of eval_registration."""
        view = _SegEvalView(self.seg_model, self.config, self.device)
        dice_per_class, dice_avg, _ = SegmentationExperiment.eval(view, seg_loader or self.validation_data_loader)
        res = eval_registration(self.reg_model, pair_loader or self.validation_pair_loader, self.config['n_classes'], self.device)
        res['seg_dice_per_class'], res['seg_dice_avg'] = dice_per_class, float(dice_avg)
        if self.atlas_fusion:
            res.update(eval_atlas_fusion(self.reg_model, self.atlas_volumes(), dataset_volumes(seg_loader or self.validation_data_loader),
                                         self.config['n_classes'], self.device, mode=self.atlas_fusion))
        return res

    def atlas_volumes(self):
        """The atlases of config['atlas_fusion']: the labelled training volumes in index order, at most atlas_fusion_max of them."""
        if self.training_data_loader is None:
            self.setup_train_data()
        labeled = getattr(self, 'labeled', None)
        if labeled is None:                                   # a loader handed in through the config: its dataset knows its labelled volumes
            labeled = sorted(self.training_data_loader.dataset.labeled)
        return dataset_volumes(self.training_data_loader, labeled, first=self.atlas_fusion_max)

    def validate(self):
        if self.current_epoch % self.config['valid_epoch_period'] != 0:
            return
        start_time = time.time()
        res = self.last_validation = self.eval()
        scores = {'seg': res['seg_dice_avg'], 'reg': res['dice_avg']}
        best = {}
        for net, sched in (('seg', self.seg_scheduler), ('reg', self.reg_scheduler)):
            if sched is not None:
                if self.config['lr_mode'] == 'plateau':
                    sched.step(scores[net])
                else:
                    sched.step()
            # (the first validation of a run always leaves a best file, also when its score is 0 or NaN: test() reloads it)
            best[net] = not os.path.isfile(os.path.join(self.ckpoint_dir, net + '_model_best.pth.tar'))
            if scores[net] > getattr(self, net + '_best_score'):
                best[net] = True
                setattr(self, net + '_best_score', scores[net])
        if parallel.rank() != 0:
            return
        if self.writer is not None:
            tag = 'validation_{}/'.format(self.config['data'])
            for k in ('seg_dice_avg', 'dice_avg', 'identity_dice_avg', 'nonpos_frac', 'det_mean', 'det_std'):
                self.writer.add_scalar(tag + k, res[k], global_step=self.global_step)
        print("Validation: seg Dice Avg: {:.4f}{}  registration Dice Avg: {:.4f} (identity {:.4f})  det J {:.4f} +- {:.4f}, folding {:.3%} "
              "({:.3f} sec) {}".format(scores['seg'], atlas_fusion_text(res), scores['reg'], res['identity_dice_avg'], res['det_mean'], res['det_std'],
                                       res['nonpos_frac'], time.time() - start_time, datetime.datetime.now().strftime("%D %H:%M:%S")))
        if self.current_epoch % self.config['save_ckpts_epoch_period'] == 0:
            for net, model, opt in (('seg', self.seg_model, self.seg_optimizer), ('reg', self.reg_model, self.reg_optimizer)):
                self.save_checkpoint({'epoch': self.current_epoch,
                                      'model_state_dict': model.state_dict(),
                                      'optimizer_state_dict': opt.state_dict(),
                                      net + '_best_score': getattr(self, net + '_best_score')},
                                     best[net], self.ckpoint_dir, prefix=net)

    def test(self, best=True, if_log=True):
        """Reload the best (or the last) pair of checkpoints and report the validation metrics on the test loaders."""
        self.setup_model()
        if self.validation_data_loader is None or self.validation_pair_loader is None:
            self.setup_train_data()
        name = 'model_best.pth.tar' if best else 'checkpoint.pth.tar'
        files = {net: os.path.join(self.ckpoint_dir, net + '_' + name) for net in ('seg', 'reg')}
        e_s, _ = self.initialize_model(self.seg_model, optimizer=None, ckpoint_path=files['seg'])
        e_r, _ = self.initialize_model(self.reg_model, optimizer=None, ckpoint_path=files['reg'])
        ops.bump_weights_epoch()
        res = self.eval(self.config.get('testing_data_loader'), self.config.get('testing_pair_loader'))
        print('Testing Models: {} ({} epochs), {} ({} epochs)  seg Dice_avg: {}  registration Dice_avg: {} (identity {})  folding fraction: {}{}'.format(
            files['seg'], e_s, files['reg'], e_r, res['seg_dice_avg'], res['dice_avg'], res['identity_dice_avg'], res['nonpos_frac'], atlas_fusion_text(res)))
        return res
