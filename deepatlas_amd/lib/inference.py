"""From a trained segmentation net to a label map: blended sliding-window inference (the project's own; after nnU-Net and MONAI's
sliding_window_inference) and the way back from the prepared grid to a scan's own grid.

SlidingWindowPredictor tiles a volume with lib/transforms.py's Partition, runs the net over chunks of tiles, and adds every tile's softmax
probabilities, weighted by a separable window that favours the tile's centre, into one accumulator (ops.blend_accumulate: one HIP kernel per
chunk, the softmax kept in registers, the covering tiles of a voxel added in a fixed order); optionally the same for mirrored copies of the
tiles (test-time augmentation), the un-mirroring folded into the kernel's index arithmetic.  ops.blend_finalize takes the argmax.
RecordedPreprocess runs config['preprocess'] and notes what restore_native needs to map a label map back to the grid of the file.
Registration: frame_of turns such a record into the per-axis map prepared index -> native index, and RegistrationPredictor takes a pair of
prepared scans to one field and carries the NATIVE moving data onto the fixed file's grid through it (ops.warp_to_grid: one interpolation).
Out of scope: averaging raw logits instead of probabilities, per-class probability maps, checkpoint ensembling, rotations as test-time
augmentation, bf16 accumulators, HIP-graph capture, 2-D inputs, tiled registration, the inverse direction, joint checkpoints.
"""
import numpy as np
import torch

from . import transforms as med_transforms
from .. import ops

MIRROR_AXES = ('z', 'y', 'x')
TILE_BLEND_DEFAULTS = {'window': 'gaussian', 'sigma_scale': 0.125, 'mirror': []}


def parse_mirror(mirror):
    """A subset of the axes 'z', 'y', 'x' (a string like 'zy', or a sequence) -> the list in (z, y, x) order."""
    if mirror is None:
        return []
    axes = list(mirror)
    bad = [a for a in axes if a not in MIRROR_AXES]
    if bad or len(set(axes)) != len(axes):
        raise ValueError("mirror takes distinct axes out of 'z', 'y', 'x', got %r" % (mirror,))
    return [a for a in MIRROR_AXES if a in axes]


def parse_tile_blend(spec, patch=None):
    """config['tile_blend'] -> None (off) or the full dict {'window': 'gaussian' | 'constant', 'sigma_scale': a positive float, 'mirror': axes
    out of 'z', 'y', 'x'}.  Accepted: None, 'gaussian', 'constant', or a dict with any of the three keys.  `patch` is the experiment's parsed
    config['patch']: blending acts on the evaluation tiles, so a spec without it is a ValueError."""
    if spec is None:
        return None
    if isinstance(spec, str):
        spec = {'window': spec}
    if not isinstance(spec, dict):
        raise ValueError("config['tile_blend'] must be None, 'gaussian', 'constant' or a dict, got %r" % (spec,))
    unknown = sorted(set(spec) - set(TILE_BLEND_DEFAULTS))
    if unknown:
        raise ValueError("config['tile_blend'] takes %s, got %s" % (sorted(TILE_BLEND_DEFAULTS), ', '.join(repr(k) for k in unknown)))
    out = dict(TILE_BLEND_DEFAULTS)
    out.update({k: v for k, v in spec.items() if v is not None})
    if out['window'] not in med_transforms.IMPORTANCE_WINDOWS:
        raise ValueError("config['tile_blend']['window'] %r: 'gaussian' or 'constant'" % (out['window'],))
    s = out['sigma_scale']
    if isinstance(s, bool) or not isinstance(s, (int, float)) or not 0.0 < float(s) < float('inf'):
        raise ValueError("config['tile_blend']['sigma_scale'] must be a positive finite number, got %r" % (s,))
    out['sigma_scale'] = float(s)
    out['mirror'] = parse_mirror(out['mirror'])
    if patch is None:
        raise ValueError("config['tile_blend'] blends the evaluation tiles of patch mode: it needs config['patch']")
    return out


def refuse_tile_blend(cfg, what):
    """Blended tiled inference is the segmentation experiment's alone: the `what` experiment raises when given config['tile_blend']."""
    if cfg.get('tile_blend') is not None:
        raise ValueError("config['tile_blend'] (blended tiled inference) is not implemented for the %s experiment" % what)


class SlidingWindowPredictor(object):
    """Blended sliding-window inference of a single-channel volume.  tile / overlap are (z, y, x); Partition's geometry: per axis the tiles
    advance by tile - 2 overlap over the volume reflect-padded by `overlap`.  window / sigma_scale: lib.transforms.importance_window.  mirror:
    a subset of ('z', 'y', 'x'); all 2^|mirror| flip combinations are run, in ascending mask order (ops.BLEND_FLIP_BITS), and averaged.
    The accumulator holds D H W K float32: 3 GB for a 160 x 384 x 384 volume with 32 classes; the tile logits of one chunk come on top.
    The result does not depend on tile_batch, bit for bit."""

    def __init__(self, model, n_class, tile, overlap, tile_batch=4, window='gaussian', sigma_scale=0.125, mirror=()):
        self.model = model
        self.n_class = int(n_class)
        if not 2 <= self.n_class <= ops.BLEND_MAX_CLASSES:
            raise ValueError('n_class must lie in 2 ... %d, got %r' % (ops.BLEND_MAX_CLASSES, n_class))
        self.tile = tuple(int(v) for v in tile)
        self.overlap = tuple(int(v) for v in overlap)
        if len(self.tile) != 3 or len(self.overlap) != 3 or any(o < 0 or t - 2 * o < 1 for t, o in zip(self.tile, self.overlap)):
            raise ValueError('tile and overlap take three integers (z, y, x) with 0 <= 2 * overlap < tile, got %r and %r' % (tile, overlap))
        self.tile_batch = int(tile_batch)
        if self.tile_batch < 1:
            raise ValueError('tile_batch must be >= 1, got %r' % (tile_batch,))
        self.window = med_transforms.importance_window(self.tile, window, sigma_scale)
        self.mirror = parse_mirror(mirror)
        bits = [ops.BLEND_FLIP_BITS[a] for a in self.mirror]
        self.masks = sorted(sum(b for j, b in enumerate(bits) if m >> j & 1) for m in range(1 << len(bits)))
        self.partition = med_transforms.Partition(tuple(reversed(self.tile)), tuple(reversed(self.overlap)))

    def predict(self, image, return_conf=False, return_acc=False):
        """image D x H x W (device float32) -> labels uint8 D x H x W; with return_conf also the confidence float32 D x H x W (the winning
        class's share of the accumulated weight), with return_acc also the accumulator D x H x W x K."""
        if image.dim() != 3:
            raise ValueError('predict takes one D x H x W volume, got shape %s' % (tuple(image.shape),))
        was_training = self.model.training
        with torch.no_grad():
            self.model.eval()
            tiles = self.partition({'image': image, 'segmentation': image})['image']               # T x 1 x tz x ty x tx
            D, H, W = (int(s) for s in image.shape)
            acc = torch.zeros((D, H, W, self.n_class), dtype=torch.float32, device=tiles.device)
            for mask in self.masks:
                dims = [2 + k for k, a in enumerate(MIRROR_AXES) if mask & ops.BLEND_FLIP_BITS[a]]
                seen = torch.flip(tiles, dims) if dims else tiles
                for k in range(0, seen.shape[0], self.tile_batch):
                    logits = ops.materialize_logits(self.model(seen[k:k + self.tile_batch]))
                    ops.blend_accumulate(acc, logits, k, self.tile, self.overlap, self.window, mask)
            out = ops.blend_finalize(acc, return_conf=return_conf)
        self.model.train(was_training)
        out = out if return_conf else (out,)
        if return_acc:
            out = out + (acc,)
        return out if len(out) > 1 else out[0]

    def predict_batch(self, images):
        """images N x 1 x D x H x W -> labels uint8 N x D x H x W."""
        if images.dim() != 5 or images.shape[1] != 1:
            raise ValueError('predict_batch takes N x 1 x D x H x W, got shape %s' % (tuple(images.shape),))
        return torch.stack([self.predict(images[n, 0]) for n in range(images.shape[0])], 0)


# ---- the way back to the file's grid -------------------------------------------------------------------------------------------------
class RecordedPreprocess(object):
    """config['preprocess'] as training applied it (lib.transforms.make_preprocess), run step by step while noting what restore_native needs:
    record = {'native_size': (D, H, W), 'native_spacing': (x, y, z), 'steps': [...]} with one entry per step that changed the grid, in the
    order they ran: ('resample', size before (D, H, W), spacing before (x, y, z), spacing after (x, y, z)) and ('flip',) when left_to_right
    fired (predict_seg.py appends ('crop', size before, CropTensor's six counts) for config['crop_size']).  label_filter, percentile_rescale
    and normalize change no geometry and leave no entry."""

    def __init__(self, spec):
        self.steps = med_transforms.make_preprocess(spec)

    def __call__(self, sample):
        size = tuple(int(s) for s in np.shape(sample['image'])[-3:])
        spacing = tuple(float(s) for s in (sample.get('spacing') or (1.0, 1.0, 1.0)))
        record = {'native_size': size, 'native_spacing': spacing, 'steps': []}
        for t in self.steps:
            before = tuple(int(s) for s in np.shape(sample['image'])[-3:])
            sp_before = tuple(float(s) for s in (sample.get('spacing') or (1.0, 1.0, 1.0)))
            sample = t(sample)
            if isinstance(t, med_transforms.Resample):
                record['steps'].append(('resample', before, sp_before, tuple(float(s) for s in sample['spacing'])))
            elif isinstance(t, med_transforms.LeftToRight) and 'LEFT' in sample['name']:
                record['steps'].append(('flip',))
        return sample, record


def restore_native(labels, record, interpolator='nearest', resample=None):
    """A D x H x W map on the prepared grid (labels; or, with interpolator 'linear', a float map such as the confidence) -> the grid of the
    file, by undoing record['steps'] last to first: a flip by the same flip (ops.resample_volume with scale -1 along z), a resample by
    ops.resample_volume onto the size before it with the reciprocal scale (native index n reads prepared index n * spacing_before /
    spacing_after).  `resample` (default ops.resample_volume) is the one function all of this goes through: a host test passes a numpy
    restatement with the same signature."""
    resample = resample or ops.resample_volume
    out = labels
    for step in reversed(record['steps']):
        D, H, W = (int(s) for s in out.shape[-3:])
        if step[0] == 'flip':
            out = resample(out, (D, H, W), (-1.0, 1.0, 1.0), (float(D - 1), 0.0, 0.0), 'nearest', 0)
        elif step[0] == 'resample':
            _, size, sp_before, sp_after = step
            scale = tuple(sp_before[k] / sp_after[k] for k in (2, 1, 0))                           # (D, H, W) order
            out = resample(out, tuple(int(s) for s in size), scale, (0.0, 0.0, 0.0), interpolator, 0)
        elif step[0] == 'crop':                                                                    # CropTensor: the cut-off border comes back as 0
            _, size, c = step
            full = out.new_zeros(tuple(out.shape[:-3]) + tuple(int(s) for s in size))
            full[..., c[0]:c[0] + D, c[1]:c[1] + H, c[2]:c[2] + W] = out
            out = full
        else:
            raise ValueError('unknown record step %r' % (step,))
    if tuple(int(s) for s in out.shape[-3:]) != tuple(record['native_size']):
        raise ValueError('the map came back as %s, the file holds %s' % (tuple(out.shape[-3:]), tuple(record['native_size'])))
    return out


def prepare(path, name, cfg):
    """(the file's Volume, image 1 x D x H x W on the device, record for restore_native)."""
    from . import transforms as T
    from .nifti import read_nifti
    from ..models import nifti_data
    vol = read_nifti(path)
    sample, record = RecordedPreprocess(cfg.get('preprocess'))({'image': vol.array, 'name': name, 'spacing': vol.spacing})
    sample = T.SitkToTensor()(sample)
    if nifti_data.is_nifti(cfg) and cfg.get('crop_size'):
        before = tuple(int(s) for s in sample['image'].shape[-3:])
        sample = T.CropTensor(cfg['crop_size'])(sample)
        record['steps'].append(('crop', before, tuple(int(v) for v in T.CropTensor(cfg['crop_size']).crop_size)))
    return vol, sample['image'], record


# ---- registration: from the prepared grid's field to the files' grids -------------------------------------------------------------------
def frame_of(record, prepared_size):
    """The frame of a prepared grid inside its file: per axis, (D, H, W) order, the pair (a, b) of float64 with native index = a * prepared
    index + b.  Composed from record['steps'], last to first, each step mapping the index after it to the index before it: a resample
    n = (spacing after / spacing before) p (restore_native's rule), a flip p -> (D - 1) - p along D, a crop p -> p + c.  A negative a is a flip.
    prepared_size is the (D, H, W) the record's last step left; a record that does not lead from it back to record['native_size'] raises."""
    size = tuple(int(s) for s in prepared_size)
    if len(size) != 3:
        raise ValueError('prepared_size takes three extents (D, H, W), got %r' % (prepared_size,))
    a = [np.float64(1.0)] * 3
    b = [np.float64(0.0)] * 3
    for step in reversed(record['steps']):
        if step[0] == 'flip':
            scale, offset = (-1.0, 1.0, 1.0), (float(size[0] - 1), 0.0, 0.0)
        elif step[0] == 'resample':
            _, before, sp_before, sp_after = step
            scale, offset = tuple(sp_after[k] / sp_before[k] for k in (2, 1, 0)), (0.0, 0.0, 0.0)
            size = tuple(int(s) for s in before)
        elif step[0] == 'crop':
            _, before, c = step
            if len(c) != 6 or any(int(c[k]) < 0 or int(c[k]) + size[k] + int(c[k + 3]) != int(before[k]) for k in range(3)):
                raise ValueError('the crop %r of %r does not hold a grid of %r' % (tuple(c), tuple(before), size))
            scale, offset = (1.0, 1.0, 1.0), tuple(float(c[k]) for k in range(3))
            size = tuple(int(s) for s in before)
        else:
            raise ValueError('unknown record step %r' % (step,))
        a, b = [np.float64(scale[k]) * a[k] for k in range(3)], [np.float64(scale[k]) * b[k] + np.float64(offset[k]) for k in range(3)]
    if size != tuple(int(s) for s in record['native_size']):
        raise ValueError('the record leads from %s back to %s, the file holds %s' % (tuple(prepared_size), size, tuple(record['native_size'])))
    return tuple((a[k], b[k]) for k in range(3))


class RegistrationPredictor(object):
    """A trained registration net on one pair.  field(): the prepared pair -> one displacement field 1 x 3 x D x H x W on the prepared grid
    (WarpFn's units); with affine_init ('rigid' | 'affine') the pair is pre-aligned first (evalMetrics.affine_align with affine_settings),
    the net sees (aligned moving, fixed) and its field is composed with the affine by ops.affine_disp, exactly as eval_registration does.
    With refine (a dict of lib/refine.py refine_field keywords) that field is then refined on this very pair: against the ORIGINAL prepared moving
    image and the fixed one, so with affine_init it is the composed field that is refined -- the only one that maps the fixed frame onto the
    original moving image.  net_field() is the field before that step and refined() the step alone, for callers that report both.
    apply(): data on the MOVING FILE's grid -> the FIXED FILE's grid through that field (ops.warp_to_grid)."""

    def __init__(self, model, affine_init=None, affine_settings=None, refine=None):
        self.model = model
        self.affine_init = affine_init
        self.affine_settings = dict(affine_settings or {})
        self.refine = dict(refine) if refine is not None else None

    @staticmethod
    def _pair(moving_prepared, fixed_prepared):
        im_m, im_t = (t.reshape((1, 1) + tuple(t.shape[-3:])) for t in (moving_prepared, fixed_prepared))
        if tuple(im_m.shape) != tuple(im_t.shape):
            raise ValueError('the prepared pair differs in shape: %s and %s' % (tuple(im_m.shape[2:]), tuple(im_t.shape[2:])))
        return im_m, im_t

    def field(self, moving_prepared, fixed_prepared):
        disp = self.net_field(moving_prepared, fixed_prepared)
        return disp if self.refine is None else self.refined(moving_prepared, fixed_prepared, disp)

    def refined(self, moving_prepared, fixed_prepared, disp):
        """`disp` refined on this pair with the predictor's refine settings (lib/refine.py refine_field; the images as float32)."""
        from .refine import refine_field
        im_m, im_t = self._pair(moving_prepared, fixed_prepared)
        return refine_field(im_m.float(), im_t.float(), disp, **self.refine)

    def net_field(self, moving_prepared, fixed_prepared):
        """The field the net predicts (with affine_init composed with the affine), before any refinement."""
        from . import evalMetrics as metrics
        im_m, im_t = self._pair(moving_prepared, fixed_prepared)
        was_training = self.model.training
        with torch.no_grad():
            self.model.eval()
            if self.affine_init is None:
                disp = self.model(im_m, im_t)[0]
            else:
                theta, im_a = metrics.affine_align(im_m, im_t, mode=self.affine_init, **self.affine_settings)
                disp = ops.affine_disp(theta, self.model(im_a, im_t)[0])
        self.model.train(was_training)
        return disp.detach()

    def apply(self, moving_native, disp, fixed_vol, fixed_record, moving_vol, moving_record, order=1, default=0, prefiltered=False, world=False):
        """moving_native: D x H x W or C x D x H x W device data on the moving file's grid (its raw intensities, its labels, or with
        prefiltered=True their B-spline coefficients).  Returns it on the fixed file's grid; with world=True also the displacement in
        millimetres between the two files' world frames (fixed_vol.affine, moving_vol.affine), 3 x D x H x W."""
        prepared = tuple(int(s) for s in disp.shape[2:])
        return ops.warp_to_grid(moving_native, disp, fixed_record['native_size'], frame_of(fixed_record, prepared), frame_of(moving_record, prepared),
                                order=order, default=default, prefiltered=prefiltered,
                                world=(fixed_vol.affine, moving_vol.affine) if world else None)
