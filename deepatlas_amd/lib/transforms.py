"""Tensor-level transforms (lib/transforms.py) on the device: mask_to_one_hot / SegMaskToOneHot (:652-689), and the data path of
SURVEY.md row f4 -- SitkToTensor's clamp + cast (:71-92), CropTensor (:124-158), Partition's overlap tiling with reflect padding
and both assemble modes (:508-649), the two random spatial augmentations RandomRigidTransform (:202-259) and
RandomBSplineTransform (:161-199) as device resamples, and the intensity half: the reference's two image filters GaussianBlur
(:293-306) and BilateralFilter (:308-320) and the project's own RandomIntensityTransform (bias field, gamma, gain / offset, noise) as
device kernels.  The preprocessing transforms the reference runs through SimpleITK are device kernels too (csrc/preprocess.hip): Resample to
a voxel size (:9-57), Normalization (:59-68), LeftToRight (:269-284), SegmentationLabelFilter (:692-706), IdentityTransform, and the
project's own PercentileRescale; they act on the raw arrays lib/nifti.py reads.  Every class takes numpy arrays (what
sitk.GetArrayFromImage returns) or tensors and hands back DEVICE tensors, so a loader thread only uploads the raw volume once.
Patch sampling, RandomCrop (:322-388) and BalancedRandomCrop (:391-505), runs on the device as well (csrc/crop.hip): the class count of every
crop window as a separable sliding sum, a uniform pick among the starts that pass, one batched gather.  importance_window gives the per-axis
tables that weight a tile in blended sliding-window inference (lib/inference.py).
Out of scope: reorientation by the affine, oblique resampling, anti-aliasing on down-sampling and B-spline interpolation.
"""
import math

import numpy as np
import torch

from .. import ops
from .. import _native as nat
from .._native import call, ptr, stream


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _to_device_array(a):
    """numpy array / tensor / SimpleITK image -> contiguous device tensor in its own dtype."""
    if not torch.is_tensor(a):
        if not isinstance(a, np.ndarray):
            try:                                     # a SimpleITK image, when the module is present
                import SimpleITK as sitk
                a = sitk.GetArrayFromImage(a)
            except ImportError:
                a = np.asarray(a)
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(_device()).contiguous()


_SIGNED_OF = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _is_integer(dtype):
    return not (dtype.is_floating_point or dtype.is_complex)


def _is_unsigned(dtype):
    return dtype in (torch.uint8, torch.uint16, torch.uint32, torch.uint64)


def _clamp_source(a):
    """numpy array / tensor / SimpleITK image -> contiguous device tensor in one of da_clamp01_to_f32's five dtypes whose clamp-then-cast equals the
    clamp of `a` IN ITS OWN DTYPE followed by the cast to float32 (the numpy original).  Every conversion is exact: float16 / bfloat16 widen; bool,
    int8 and uint16 widen; the integer types no kernel dtype holds (uint32, int64, uint64) are clamped to {0, 1} BEFORE they are narrowed -- in numpy
    ahead of the upload for an array, on the tensor's device otherwise, where an unsigned type is read through its signed view (its clamp to [0, 1] is
    `x != 0`; torch implements neither clamp nor comparisons for the wide unsigned types)."""
    if not torch.is_tensor(a) and not isinstance(a, np.ndarray):
        try:                                         # a SimpleITK image, when the module is present
            import SimpleITK as sitk
            a = sitk.GetArrayFromImage(a)
        except ImportError:
            a = np.asarray(a)
    if isinstance(a, np.ndarray):
        if a.dtype.kind in 'iu' and a.dtype.itemsize >= 4 and a.dtype != np.int32:
            a = np.clip(a, 0, 1).astype(np.uint8)
        elif a.dtype.kind not in 'biuf':
            raise ValueError('SitkToTensor: an image of dtype %s has no clamp to [0, 1]' % a.dtype)
        a = torch.from_numpy(np.ascontiguousarray(a))
    if a.dtype in ops.PREPROCESS_DTYPE_CODE:
        return a.to(_device()).contiguous()
    if a.dtype.is_complex:
        raise ValueError('SitkToTensor: an image of dtype %s has no clamp to [0, 1]' % a.dtype)
    if a.dtype.is_floating_point:                    # float16, bfloat16
        return a.to(_device()).contiguous().to(torch.float64)
    a = a.contiguous()
    if a.dtype == torch.bool:
        return a.to(_device()).to(torch.uint8)
    if a.dtype == torch.int8:
        return a.to(_device()).to(torch.int16)
    if a.dtype == torch.uint16:
        return a.view(torch.int16).to(_device()).to(torch.int32) & 0xFFFF
    if _is_unsigned(a.dtype):                        # uint32, uint64
        return (a.view(_SIGNED_OF[a.element_size()]).to(_device()) != 0).to(torch.uint8)
    return a.to(_device()).clamp(0, 1).to(torch.uint8)          # int64


def _exact_for_copy(t, what, as_float=False):
    """A device tensor `t` in a dtype the copy kernels move (4 bytes per element, or 1) that holds exactly t's integer values, or ValueError naming the
    dtype: there is no silent wrap.  4-byte tensors pass as they are, 1-byte ones too unless as_float (an image: float32, exact).  2-byte integers
    widen to int32.  8-byte integers become int32 when every value fits int32 (as_float: float32 when every magnitude is at most 2^24), which costs one
    min / max read-back.  Floating types of other widths go to float32, the rounding SitkToTensor's cast applies as well."""
    if t.element_size() == 4 or (t.element_size() == 1 and not as_float):
        return t
    if t.dtype.is_complex:
        raise ValueError('%s: dtype %s is not supported' % (what, t.dtype))
    if t.dtype.is_floating_point:
        return t.float()
    if t.element_size() == 2:
        t = t.to(torch.int32) if t.dtype == torch.int16 else t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    elif t.element_size() == 8:
        s = t if t.dtype == torch.int64 else t.contiguous().view(torch.int64)
        lo, hi = (int(s.min()), int(s.max())) if s.numel() else (0, 0)
        lo_ok, hi_ok = (-2 ** 24, 2 ** 24) if as_float else (-2 ** 31, 2 ** 31 - 1)
        if (t.dtype == torch.uint64 and lo < 0) or lo < lo_ok or hi > hi_ok:
            raise ValueError('%s: the %s values do not all fit %s exactly (the tensor spans [%d, %d] read as int64); convert it yourself'
                             % (what, t.dtype, 'float32' if as_float else 'int32', lo, hi))
        t = s.to(torch.int32)
    return t.float() if as_float else t


def mask_to_one_hot(mask, n_classes):
    """lib/transforms.py:675-689: B x 1 x D x M x N index mask -> B x C x D x M x N float one-hot."""
    return ops.one_hot(mask, n_classes)


class SegMaskToOneHot:
    """lib/transforms.py:652-673."""

    def __init__(self, n_classes, dtype=torch.float):
        self.n_classes = n_classes
        self.dtype = dtype

    def __call__(self, sample):
        sample['segmentation_onehot'] = self.one_mask_to_one_hot(sample['segmentation'])
        return sample

    def one_mask_to_one_hot(self, mask):
        """mask D x M x N -> C x D x M x N."""
        return ops.one_hot(mask.unsqueeze(0).unsqueeze(0), self.n_classes)[0].to(self.dtype)


class SitkToTensor(object):
    """lib/transforms.py:71-92: image -> float32 clamped to [0, 1] with a leading channel axis (1 x D x H x W), segmentation ->
    uint8 (D x H x W).  The clamp compares in the source dtype and then casts, like the numpy original; one kernel, on the device."""

    def __call__(self, sample):
        img = _clamp_source(sample['image'])
        out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
        call('da_clamp01_to_f32', ptr(img), ops.PREPROCESS_DTYPE_CODE[img.dtype], ptr(out), img.numel(), stream())
        sample['image'] = out.unsqueeze(0)
        if 'segmentation' in sample.keys():
            sample['segmentation'] = _to_device_array(sample['segmentation']).to(torch.uint8)
        return sample


class CropTensor(object):
    """lib/transforms.py:124-158: crop_size [z, y, x] (both sides) or [z_lo, y_lo, x_lo, z_hi, y_hi, x_hi] voxels off a C x D x H x W
    image and its D x H x W segmentation, as fresh contiguous device tensors from one copy kernel.  Every integer dtype keeps its values (and
    8-byte integers their dtype); float64 / float16 come back as float32."""

    def __init__(self, crop_size):
        crop_size = list(crop_size)
        if len(crop_size) == 3:
            self.crop_size = crop_size + crop_size
        elif len(crop_size) == 6:
            self.crop_size = crop_size
        else:
            raise ValueError("crop size should be of length 3 or 6, but {} is given".format(len(crop_size)))

    def _crop(self, t, lead, size):
        c = self.crop_size
        D, H, W = size
        Do, Ho, Wo = D - c[0] - c[3], H - c[1] - c[4], W - c[2] - c[5]
        t = t.to(_device())                       # host tensors are uploaded: there is no host implementation of this path
        wide = None
        if t.element_size() == 8 and _is_integer(t.dtype):
            # a crop only moves elements: an 8-byte integer is moved as the two 4-byte halves it consists of (a row of 2 W), exact for every value
            wide, t = t.dtype, t.contiguous().view(torch.int32)
        else:
            t = _exact_for_copy(t, 'CropTensor').contiguous()
        k = 2 if wide is not None else 1
        out = torch.empty(tuple(t.shape[:-3]) + (Do, Ho, k * Wo), dtype=t.dtype, device=t.device)
        call('da_crop3d', ptr(t), ptr(out), t.element_size(), lead, D, H, k * W, c[0], c[1], k * c[2], Do, Ho, k * Wo, stream())
        return out if wide is None else out.view(wide)

    def __call__(self, sample):
        img = sample['image']
        size = tuple(img.shape[1:4])
        sample['image'] = self._crop(img, img.shape[0], size)
        if 'segmentation' in sample.keys():
            sample['segmentation'] = self._crop(sample['segmentation'], 1, size)
        return sample


class Partition(object):
    """lib/transforms.py:508-649: overlap-tile strategy.  tile_size / overlap_size are given in SimpleITK order (x, y, z) and
    flipped to numpy order, as in the reference.  __call__ produces the N x 1 x tz x ty x tx tiles from the reflect-padded volume
    without materialising the padding; assemble() puts predicted tiles back (core copy, or per-voxel majority vote).
    The kernels move 1- and 4-byte elements: other integer widths are converted only where that is exact (_exact_for_copy) and raise a
    ValueError naming the dtype otherwise; the vote takes labels 0 ... 255 and refuses anything else the same way."""

    def __init__(self, tile_size, overlap_size, padding_mode='reflect', mode="pred"):
        self.tile_size = np.flipud(np.asarray(tile_size))
        self.overlap_size = np.flipud(np.asarray(overlap_size))
        if padding_mode != 'reflect':
            raise NotImplementedError("device Partition implements numpy.pad mode 'reflect' (the reference's default)")
        self.padding_mode = padding_mode
        self.mode = mode

    def _geom(self, shape):
        self.image_size = np.array(shape)
        self.effective_size = self.tile_size - self.overlap_size * 2
        self.tiles_grid_size = np.ceil(self.image_size / self.effective_size).astype(int)
        self.padded_size = self.effective_size * self.tiles_grid_size + self.overlap_size * 2 - self.image_size

    def _tiles(self, vol):
        D, H, W = vol.shape
        n = int(np.prod(self.tiles_grid_size))
        tiles = torch.empty((n,) + tuple(int(v) for v in self.tile_size), dtype=vol.dtype, device=vol.device)
        (ka, ta), (kb, ov) = ops._int3_array(self.tile_size), ops._int3_array(self.overlap_size)
        call('da_partition_tiles', ptr(vol), ptr(tiles), vol.element_size(), D, H, W, ta, ov, stream())
        return tiles

    def __call__(self, sample):
        image = _exact_for_copy(_to_device_array(sample['image']), "Partition: sample['image']", as_float=True)
        self.image = sample['image']
        self.name = sample.get('name')
        self._geom(tuple(image.shape))
        sample['image'] = self._tiles(image).unsqueeze(1)
        seg = _to_device_array(sample['segmentation'])
        if self.mode == 'pred':
            sample['segmentation'] = seg.unsqueeze(0)
        else:
            sample['segmentation'] = self._tiles(_exact_for_copy(seg, "Partition: sample['segmentation']")).unsqueeze(1)
        return sample

    def assemble(self, tiles, is_vote=False, if_itk=False, crop_size=None, data_type=None):
        """tiles: N x tz x ty x tx (device).  Returns a device tensor D x H x W (the reference returns numpy float64 / uint8, or a
        SimpleITK image when if_itk, which needs the host library)."""
        if if_itk:
            raise NotImplementedError('if_itk=True needs SimpleITK on the host; call with if_itk=False and wrap the result there')
        t = tiles.to(_device())
        if is_vote:
            if t.dtype != torch.uint8:              # the vote kernel reads uint8 labels: anything else must fit, and is refused by name if it does not
                # (a wide unsigned type is read through its signed view: what turns negative there is above 255 as well)
                s = t.contiguous().view(_SIGNED_OF[t.element_size()]) if _is_unsigned(t.dtype) else t
                if t.dtype.is_complex or (s.numel() and not bool(((s >= 0) & (s <= 255) & (s == s.to(torch.uint8))).all())):
                    raise ValueError('Partition.assemble(is_vote=True): the %s tiles hold labels above 255 (or negative / fractional ones); '
                                     'the vote takes labels 0 ... 255' % (t.dtype,))
                t = s.to(torch.uint8)
        else:
            t = _exact_for_copy(t, 'Partition.assemble: tiles')
        t = t.contiguous()
        D, H, W = (int(v) for v in self.image_size)
        out = torch.empty((D, H, W), dtype=t.dtype, device=t.device)
        (ka, ta), (kb, ov) = ops._int3_array(self.tile_size), ops._int3_array(self.overlap_size)
        call('da_assemble_tiles', ptr(t), ptr(out), t.element_size(), D, H, W, ta, ov, 1 if is_vote else 0, stream())
        if data_type:
            out = out.to(data_type if isinstance(data_type, torch.dtype) else torch.from_numpy(np.zeros(1, dtype=data_type)).dtype)
        if crop_size:                                                   # zero a border of crop_size (x, y, z), :633-637
            keep = torch.zeros_like(out)
            sl = (slice(crop_size[2], -crop_size[2]), slice(crop_size[0], -crop_size[0]), slice(crop_size[1], -crop_size[1]))
            keep[sl] = out[sl]
            out = keep
        return out


# ---- random spatial augmentation (lib/transforms.py:161-290) ----------------------------------------------------------------------
# Device tensors carry no geometry: they follow SitkToTensor's convention (image C x D x H x W float32, segmentation D x H x W), axes in
# SimpleITK order x = W, y = H, z = D, origin 0, identity direction, spacing sample.get('spacing', (1, 1, 1)) given as (x, y, z).  The
# parameter draws and the host-side geometry are the small pure functions below; ops.spatial_resample does the resample on the device.

def _rotation_zxy(angles):
    """sitk.Euler3DTransform with ComputeZYX off: R = Rz Rx Ry (right-handed), angles (x, y, z) in radians."""
    ax, ay, az = (float(a) for a in angles)
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def rigid_index_affine(angles, translation, spacing, rotation_center):
    """3 x 4 fp64 index-space matrix A of the rigid map, q = A[:, :3] i + A[:, 3] for an output index i = (x, y, z).
    Physical point p = S i maps to R (p - c) + c + t (sitk.Euler3DTransform about c with translation t), c = S rotation_center (an
    index, (x, y, z)), S = diag(spacing); dividing by S gives the input index: A = [S^-1 R S | S^-1 (c + t - R c)]."""
    S = np.asarray(spacing, dtype=np.float64)
    R = _rotation_zxy(angles)
    c = S * np.asarray(rotation_center, dtype=np.float64)
    t = np.asarray(translation, dtype=np.float64)
    A = np.empty((3, 4))
    A[:, :3] = R * S[None, :] / S[:, None]
    A[:, 3] = (c + t - R @ c) / S
    return A


def draw_rigid(ratio, rotation_angles, translation, spacing):
    """One sample's draws, in the reference's order (:224-242): the coin np.random.rand(1) against `ratio`, then normal(0, angle / 2)
    for x, y, z (degrees -> radians), then normal(0, translation / 2) * spacing for x, y, z.  Returns None when the coin fails (nothing
    more is drawn), else (angles in radians, translation in physical units), both (x, y, z)."""
    if not np.random.rand(1)[0] < ratio:
        return None
    angles = [np.random.normal(0, rotation_angles[k] / 2) * np.pi / 180 for k in range(3)]
    trans = [np.random.normal(0, translation[k] / 2) * spacing[k] for k in range(3)]
    return np.array(angles), np.array(trans)


def bspline_grid(size, mesh_size, order):
    """Control grid (gx, gy, gz) = mesh_size + order of sitk.BSplineTransformInitializer(img, mesh_size, order) on a volume of `size`
    voxels, both (x, y, z).  Orders 1, 2, 3; every axis needs >= 2 voxels (the domain spans the voxel centres [0, size - 1])."""
    if order not in (1, 2, 3):
        raise ValueError('bspline_order %r: orders 1, 2 and 3 are supported' % (order,))
    if len(mesh_size) != 3 or min(int(m) for m in mesh_size) < 1:
        raise ValueError('mesh_size must be three positive integers (x, y, z)')
    if min(int(s) for s in size) < 2:
        raise ValueError('a B-spline transform needs >= 2 voxels per axis, got size %s' % (tuple(size),))
    return tuple(int(m) + order for m in mesh_size)


def bspline_kernel(u, order):
    """Centred uniform B-spline of `order` (1 hat, 2 quadratic, 3 cubic) at u, fp64."""
    a = np.abs(np.asarray(u, dtype=np.float64))
    if order == 1:
        return np.where(a < 1, 1 - a, 0.0)
    if order == 2:
        return np.where(a < 0.5, 0.75 - a * a, np.where(a < 1.5, 0.5 * (1.5 - a) ** 2, 0.0))
    return np.where(a < 1, (4 - 6 * a * a + 3 * a ** 3) / 6, np.where(a < 2, (2 - a) ** 3 / 6, 0.0))


def bspline_support(i, size, mesh, order):
    """Support of output index i along one axis: grid coordinate g = i M / (size - 1) + (order - 1) / 2, start = floor(g - (order - 1) / 2)
    clamped to <= M - 1 (the limit from inside at the upper face: ITK's InsideValidRegion nudge), weights B(g - start - k), k = 0..order."""
    g = i * mesh / (size - 1) + (order - 1) / 2
    start = np.minimum(np.floor(g - (order - 1) / 2).astype(np.int64), mesh - 1)
    k = np.arange(order + 1)
    w = bspline_kernel(np.asarray(g)[..., None] - (np.asarray(start)[..., None] + k), order)
    return start, w


def draw_bspline(ratio, n_params, deform_scale, random_mode):
    """One sample's draws, in the reference's order (:178-188): the coin np.random.rand(1), then ONE vector of all n_params parameters,
    normal(0, deform_scale / 2, n) ('Normal') or random(n) * deform_scale ('Uniform').  Then, as the reference's code does, the first third
    is set to 0.  The reference's comment calls that third the z displacement; in ITK's parameter layout it is the X component (all x
    coefficients, then y, then z), so x is the axis that stays undeformed.  Returns None when the coin fails."""
    if not np.random.rand(1)[0] < ratio:
        return None
    if random_mode == 'Normal':
        p = np.random.normal(0, deform_scale / 2, n_params)
    elif random_mode == 'Uniform':
        p = np.random.random(n_params) * deform_scale
    else:
        raise ValueError("random_mode %r: 'Normal' or 'Uniform'" % (random_mode,))
    p[0:int(len(p) / 3)] = 0
    return p


def bspline_coefficients(params, grid):
    """Flat ITK parameter vector -> 3 x gz x gy x gx array (component x, y, z; each grid flattened with x fastest), physical units."""
    gx, gy, gz = grid
    return np.asarray(params, dtype=np.float64).reshape(3, gz, gy, gx)


_IDENTITY_3x4 = np.eye(3, 4)


def _as_batch(sample):
    img = sample['image']
    seg = sample.get('segmentation')
    single = img.dim() == 4
    if img.dim() not in (4, 5):
        raise ValueError('image must be C x D x H x W or N x C x D x H x W')
    imgs = img.unsqueeze(0) if single else img
    segs = None if seg is None else (seg.unsqueeze(0) if single else seg)
    return imgs, segs, single


def _store(sample, img, seg, single):
    if img is not None:
        sample['image'] = img[0] if single else img
    if seg is not None:
        sample['segmentation'] = seg[0] if single else seg
    return sample


def _check_interpolator(interpolator):
    if interpolator not in ops.AUG_INTERPOLATORS:
        raise NotImplementedError("interpolator %r: the device resample implements 'linear' and 'nearest' (no sitkBSpline)" % (interpolator,))
    return interpolator


class RandomBSplineTransform(object):
    """lib/transforms.py:161-199 on the device: random B-spline deformation of an image and its segmentation.
    sample['image'] C x D x H x W float32 (or a batch N x C x D x H x W), sample['segmentation'] D x H x W (or N x D x H x W) uint8 / int64.
    Per sample: the coin against `ratio`, then the draws of draw_bspline.  Geometry of sitk.BSplineTransformInitializer(img, mesh_size,
    bspline_order) (mesh_size (x, y, z)): per axis M + order control points over the voxel centres [0, size - 1] (bspline_support); the
    displacement is in physical units, input index = i + d(i) / spacing.  Resample as sitk.Resample onto the image's own grid: inside
    (-0.5 <= q < size - 0.5) the image is trilinear with neighbours clamped to the volume ('linear') or nearest ('nearest'), labels
    nearest floor(q + 0.5); outside 0.1 for the image, 0 for labels.  Samples whose coin fails are copied unchanged in the same launch;
    when every coin fails the sample is returned untouched with no device call.  Returns fresh device tensors otherwise."""

    def __init__(self, mesh_size=(3, 3, 3), bspline_order=2, deform_scale=1.0, ratio=0.5, interpolator='linear', random_mode='Normal'):
        if bspline_order not in (1, 2, 3):
            raise ValueError('bspline_order %r: orders 1, 2 and 3 are supported' % (bspline_order,))
        self.mesh_size = mesh_size
        self.bspline_order = bspline_order
        self.deform_scale = deform_scale
        self.ratio = ratio  # control the probability of conduct transform
        self.interpolator = _check_interpolator(interpolator)
        self.random_mode = random_mode

    def draw(self, n, size):
        """The draws of n samples of `size` (x, y, z) voxels, sample after sample: a list of flat parameter vectors or None."""
        grid = bspline_grid(size, self.mesh_size, self.bspline_order)
        n_params = 3 * grid[0] * grid[1] * grid[2]
        return [draw_bspline(self.ratio, n_params, self.deform_scale, self.random_mode) for _ in range(n)]

    def __call__(self, sample):
        imgs, segs, single = _as_batch(sample)
        D, H, W = (int(s) for s in imgs.shape[-3:])
        grid = bspline_grid((W, H, D), self.mesh_size, self.bspline_order)
        params = self.draw(imgs.shape[0], (W, H, D))
        if all(p is None for p in params):
            return sample
        spacing = np.asarray(sample.get('spacing', (1.0, 1.0, 1.0)), dtype=np.float64)
        coef = np.zeros((len(params), 3, grid[2], grid[1], grid[0]))
        for k, p in enumerate(params):
            if p is not None:
                coef[k] = bspline_coefficients(p, grid) / spacing[:, None, None, None]
        affine = np.broadcast_to(_IDENTITY_3x4, (len(params), 3, 4))
        img, seg = ops.spatial_resample(imgs, segs, affine, coef, self.bspline_order, self.interpolator)
        return _store(sample, img, seg, single)


class RandomRigidTransform(object):
    """lib/transforms.py:202-259 on the device: random rigid (sitk.Euler3DTransform) transform of an image and / or its segmentation.
    Tensors as RandomBSplineTransform.  Per sample: the coin against `ratio`, then the draws of draw_rigid.  The rotation R = Rz Rx Ry
    (ComputeZYX off) acts about c = spacing * rotation_center, an index (x, y, z) defaulting to (W, H, D) // 2; output point p = S i reads
    the input at R (p - c) + c + t, composed on the host in fp64 into one index-space 3 x 4 matrix per sample (rigid_index_affine).
    Resample rules as RandomBSplineTransform.  mode 'both', 'img' or 'seg' (the other tensor is left as it is); anything else raises
    ValueError."""

    def __init__(self, ratio=1.0, rotation_center=None, rotation_angles=(0.0, 0.0, 0.0), translation=(0.0, 0.0, 0.0),
                 interpolator='linear', mode='both'):
        if mode not in ('both', 'img', 'seg'):
            raise ValueError('Wrong rigid transformation mode :{}!'.format(mode))
        self.rotation_center = rotation_center
        self.rotation_angles = rotation_angles
        self.translation = translation
        self.interpolator = _check_interpolator(interpolator)
        self.ratio = ratio
        self.mode = mode

    def draw(self, n, spacing=(1.0, 1.0, 1.0)):
        """The draws of n samples, sample after sample: a list of (angles, translation) or None."""
        return [draw_rigid(self.ratio, self.rotation_angles, self.translation, spacing) for _ in range(n)]

    def __call__(self, sample):
        imgs, segs, single = _as_batch(sample)
        D, H, W = (int(s) for s in imgs.shape[-3:])
        spacing = tuple(float(s) for s in sample.get('spacing', (1.0, 1.0, 1.0)))
        params = self.draw(imgs.shape[0], spacing)
        if all(p is None for p in params):
            return sample
        center = self.rotation_center if self.rotation_center else (np.array((W, H, D)) // 2).tolist()
        affine = np.stack([_IDENTITY_3x4 if p is None else rigid_index_affine(p[0], p[1], spacing, center) for p in params])
        img, seg = ops.spatial_resample(imgs if self.mode in ('both', 'img') else None,
                                        segs if self.mode in ('both', 'seg') else None, affine, interpolator=self.interpolator)
        return _store(sample, img, seg, single)


# ---- intensity augmentation (lib/transforms.py:293-320, and the project's own pointwise transform) -------------------------------
def _bessel_i_scaled(n, t):
    """e^-t I_n(t), fp64, from the ascending series sum_k (t / 2)^(2 k + n) / (k! (k + n)!) (all terms positive: no cancellation)."""
    h = 0.5 * float(t)
    term = 1.0
    for j in range(1, n + 1):
        term *= h / j
    total, k = 0.0, 0
    while True:
        total += term
        k += 1
        term *= h * h / (k * (k + n))
        if term <= total * 1e-18:
            return np.exp(-float(t)) * total


def discrete_gaussian_taps(variance, maximum_kernel_width, maximum_error):
    """ITK's GaussianOperator (what sitk.DiscreteGaussian convolves with per axis, useImageSpacing off): c_i = e^-t I_i(t), t = variance.
    c_0 and c_1 always; terms i >= 2 are appended while the running sum c_0 + 2 sum c_i is below 1 - maximum_error, stopping when a term
    falls below sum * eps or the number of coefficients exceeds maximum_kernel_width; normalised by the sum and mirrored.  fp64 vector of
    odd length.  The reference's defaults (0.5, 1, 0.9) give the 3 taps [0.163, 0.673, 0.163]; variance 0 gives [0, 1, 0]."""
    t = float(variance)
    if t < 0:
        raise ValueError('variance must be >= 0')
    cap = 1.0 - float(maximum_error)
    coeff = [_bessel_i_scaled(0, t), _bessel_i_scaled(1, t)]
    total = coeff[0] + 2.0 * coeff[1]
    i = 2
    while total < cap:
        coeff.append(_bessel_i_scaled(i, t))
        total += 2.0 * coeff[i]
        if coeff[i] < total * np.finfo(np.float64).eps:
            break
        if len(coeff) > maximum_kernel_width:
            break
        i += 1
    c = np.asarray(coeff, dtype=np.float64) / total
    return np.concatenate([c[:0:-1], c])


def _draw_coins(ratio, n):
    """One coin np.random.rand(1)[0] < ratio per sample, sample after sample."""
    return [bool(np.random.rand(1)[0] < ratio) for _ in range(n)]


class GaussianBlur(object):
    """lib/transforms.py:293-306 on the device: sitk.DiscreteGaussian(img, variance, maximumKernelWidth, maximumError, useImageSpacing=False)
    of the image; the segmentation is never touched.  Tensors as RandomRigidTransform (single sample or batch); per sample one coin against
    `ratio`; samples whose coin fails are copied unchanged in the same launch, and when every coin fails the sample is returned untouched
    with no device call.  variance: one number, or (x, y, z)."""

    def __init__(self, variance=0.5, maximumKernelWidth=1, maximumError=0.9, ratio=1.0):
        self.variance = variance
        self.maximumKernelWidth = maximumKernelWidth
        self.maximumError = maximumError
        self.ratio = ratio

    def taps(self):
        var = self.variance if np.ndim(self.variance) else [self.variance] * 3
        return [discrete_gaussian_taps(v, self.maximumKernelWidth, self.maximumError) for v in var]

    def draw(self, n):
        return _draw_coins(self.ratio, n)

    def __call__(self, sample):
        imgs, _, single = _as_batch(sample)
        coins = self.draw(imgs.shape[0])
        if not any(coins):
            return sample
        return _store(sample, ops.gaussian_blur(imgs, self.taps(), apply=coins), None, single)


class BilateralFilter(object):
    """lib/transforms.py:308-320 on the device: sitk.Bilateral(img, domainSigma, rangeSigma, numberOfRangeGaussianSamples) of the image
    (ops.bilateral_filter states the definition), with the spacing sample.get('spacing', (1, 1, 1)) as (x, y, z).  Coins, batching and the
    untouched segmentation as GaussianBlur."""

    def __init__(self, domainSigma=0.5, rangeSigma=0.06, numberOfRangeGaussianSamples=50, ratio=1.0):
        self.domainSigma = domainSigma
        self.rangeSigma = rangeSigma
        self.numberOfRangeGaussianSamples = numberOfRangeGaussianSamples
        self.ratio = ratio

    def draw(self, n):
        return _draw_coins(self.ratio, n)

    def __call__(self, sample):
        imgs, _, single = _as_batch(sample)
        coins = self.draw(imgs.shape[0])
        if not any(coins):
            return sample
        spacing = tuple(float(s) for s in sample.get('spacing', (1.0, 1.0, 1.0)))
        out = ops.bilateral_filter(imgs, self.domainSigma, self.rangeSigma, self.numberOfRangeGaussianSamples, spacing, apply=coins)
        return _store(sample, out, None, single)


def _uniform(rng):
    return float(np.random.uniform(rng[0], rng[1]))


class RandomIntensityTransform(object):
    """The project's own intensity augmentation (the reference has none) for scanner-to-scanner variation, one fused device pass
    (ops.intensity_augment): smooth multiplicative bias field exp(b), b a B-spline of `bias_order` over bias_mesh + bias_order control
    points per axis; gamma clamp01(x)^g (inverted, 1 - (1 - x)^g, with probability gamma_invert_prob); gain x + offset; additive Gaussian
    noise; clamp to [0, 1].  A range of None turns its stage off.  Per sample, in this order: the coin against `ratio`; gamma uniform in
    its range; the invert coin (drawn only when gamma_invert_prob > 0); gain; offset; the noise sigma, each uniform in its range; the
    bias coefficients as ONE vector normal(0, bias_scale / 2, gx gy gz); one 32-bit noise seed.  Only enabled stages draw, and a failed
    coin draws nothing more.  The segmentation is never touched; when every coin fails the sample is returned untouched with no device
    call."""

    def __init__(self, ratio=1.0, gamma=(0.7, 1.5), gamma_invert_prob=0.0, gain=(0.75, 1.25), offset=None, noise_std=(0.0, 0.05),
                 bias_scale=None, bias_mesh=(2, 2, 2), bias_order=2, clamp=True):
        if bias_order not in (1, 2, 3):
            raise ValueError('bias_order %r: orders 1, 2 and 3 are supported' % (bias_order,))
        self.ratio = ratio
        self.gamma = gamma
        self.gamma_invert_prob = gamma_invert_prob
        self.gain = gain
        self.offset = offset
        self.noise_std = noise_std
        self.bias_scale = bias_scale
        self.bias_mesh = bias_mesh
        self.bias_order = bias_order
        self.clamp = clamp

    def _draw_one(self, grid):
        if not np.random.rand(1)[0] < self.ratio:
            return None
        p = {'clamp': bool(self.clamp)}
        if self.gamma is not None:
            p['gamma'] = _uniform(self.gamma)
            if self.gamma_invert_prob > 0:
                p['invert'] = bool(np.random.rand(1)[0] < self.gamma_invert_prob)
        if self.gain is not None:
            p['gain'] = _uniform(self.gain)
        if self.offset is not None:
            p['offset'] = _uniform(self.offset)
        if self.noise_std is not None:
            p['noise_std'] = _uniform(self.noise_std)
        if self.bias_scale is not None:
            gx, gy, gz = grid
            p['bias_coef'] = np.random.normal(0, self.bias_scale / 2, gx * gy * gz).reshape(gz, gy, gx)
        if self.noise_std is not None:
            p['seed'] = int(np.random.randint(0, 2 ** 32, dtype=np.int64))
        return p

    def draw(self, n, size):
        """The draws of n samples of `size` (x, y, z) voxels, sample after sample: a list of parameter dicts (ops.intensity_params, plus
        'bias_coef' gz x gy x gx when the bias field is on) or None."""
        grid = bspline_grid(size, self.bias_mesh, self.bias_order) if self.bias_scale is not None else None
        return [self._draw_one(grid) for _ in range(n)]

    def __call__(self, sample):
        imgs, _, single = _as_batch(sample)
        D, H, W = (int(s) for s in imgs.shape[-3:])
        params = self.draw(imgs.shape[0], (W, H, D))
        if all(p is None for p in params):
            return sample
        coef = None
        if self.bias_scale is not None:
            gx, gy, gz = bspline_grid((W, H, D), self.bias_mesh, self.bias_order)
            coef = np.zeros((len(params), gz, gy, gx))
            for k, p in enumerate(params):
                if p is not None:
                    coef[k] = p['bias_coef']
        return _store(sample, ops.intensity_augment(imgs, params, coef, self.bias_order), None, single)


# ---- random crops (lib/transforms.py:322-505) on csrc/crop.hip -----------------------------------------------------------------------------
def crop_min_count(threshold, size):
    """The smallest integer n >= 0 with n / size > threshold in float64 -- the reference's comparison np.sum(seg_crop == c) / seg_crop.size >
    threshold (:455, :473) as a bound on the integer count.  Found by adjusting around floor(threshold * size); a threshold >= 1 gives
    size + 1 (no window passes), a negative one 0."""
    size = int(size)
    if size < 1:
        raise ValueError('size must be positive')
    t = np.float64(threshold)
    if not np.isfinite(t):
        raise ValueError('threshold must be finite')
    if t < 0:
        return 0
    n = int(min(max(np.floor(t * size), 0), size + 1))
    while n > 0 and np.float64(n - 1) / np.float64(size) > t:
        n -= 1
    while n <= size and not np.float64(n) / np.float64(size) > t:
        n += 1
    return n


def _crop_seed(random_state):
    """The one 32-bit seed of a call: from random_state when given, else from np.random as the other transforms draw."""
    rs = random_state if random_state is not None else np.random
    return int(rs.randint(0, 2 ** 32, dtype=np.int64))


def _crop_output_size(output_size):
    assert isinstance(output_size, (int, tuple))
    if isinstance(output_size, int):
        return (output_size, output_size, output_size)
    assert len(output_size) == 3
    return output_size


def _crop_labels(segs):
    """Labels in a dtype the crop kernels read: uint8, int32 and int64 as they are, other integers as int32."""
    if segs.dtype in ops.CROP_LABEL_DTYPE_CODE:
        return segs
    return segs.to(torch.int32)


def _crop_batch(sample):
    imgs, segs, single = _as_batch(sample)
    if segs is None:
        raise ValueError("the crops need sample['segmentation'] (the reference crops both)")
    imgs = imgs.to(_device())
    if imgs.dtype != torch.float32:
        imgs = imgs.float()
    return imgs, _crop_labels(segs.to(_device())), single


class RandomCrop(object):
    """lib/transforms.py:322-388 on the device: one random crop of output_size (an int, or (x, y, z) in SimpleITK order, flipped to numpy
    order as Partition flips) from the image and, at the same start, the segmentation.  Tensors as RandomRigidTransform: one sample
    (C x D x H x W, D x H x W) or a batch.  The start is uniform over random_3d_coordinates' domain, max(S - w, 1) starts per axis
    (ops.sample_crop_starts, unconditioned).  The reference's own lines 357-359 compare the wrong way round (`size_old < size_new`) and so
    always crop at start 0, and its threshold test (:381) sets a flag nothing reads: `threshold` is kept for the signature and has no effect
    here either; the evident intent, a uniform start, is what is implemented.  Unlike the reference, random_state is honoured: it yields the
    one 32-bit seed per call (np.random does otherwise)."""

    def __init__(self, output_size, threshold=-0, random_state=None):
        self.output_size = _crop_output_size(output_size)
        self.threshold = threshold
        self.random_state = random_state

    def __call__(self, sample):
        imgs, segs, single = _crop_batch(sample)
        window = tuple(int(v) for v in np.flipud(np.asarray(self.output_size)))
        starts, _ = ops.sample_crop_starts(segs, window, [None], [0], _crop_seed(self.random_state))
        img, seg = ops.crop_gather(imgs, segs, starts, window)
        return _store(sample, img, seg, single)


class BalancedRandomCrop(object):
    """lib/transforms.py:391-494 on the device: crops that alternate between the classes.  The reference's state machine is kept:
    current_class starts at 2 and advances per patch through 2, 3, 0, 1, 2, ...; tag 0 is an unconditioned crop, tag 1 asks for a share of
    class 1 above threshold[0], tags 2 and 3 for a share of class 2 above threshold[1] (threshold: a float, or a 2-tuple).  Where the
    reference redraws until np.sum(seg_crop == c) / size > threshold, the device picks uniformly among the starts that pass
    (ops.sample_crop_starts with crop_min_count), which is the distribution that loop converges to; where none passes -- the reference
    would loop forever -- the start with the largest count is taken.  sample['class'] holds the tags: an int for a single sample with
    patches = 1, else a list, sample-major.
    The project's own generalisations: classes, a list of labels (None: unconditioned) to cycle through from its first entry instead, with
    threshold a float or a sequence of the same length and the position in the list as tag; patches, the number of crops per sample (a
    single sample with patches = 1 returns a single sample, as the reference does, anything else a batch of N * patches); include_last, the
    domain S - w + 1 instead of random_3d_coordinates' max(S - w, 1); and random_state, honoured as in RandomCrop."""

    def __init__(self, output_size, threshold=0.01, random_state=None, classes=None, patches=1, include_last=False):
        self.output_size = _crop_output_size(output_size)
        if classes is None:
            assert isinstance(threshold, (float, tuple))
            if isinstance(threshold, float):
                self.threshold = (threshold, threshold, threshold)
            else:
                assert len(threshold) == 2
                self.threshold = threshold
            self.cycle = [(None, 0.0), (1, self.threshold[0]), (2, self.threshold[1]), (2, self.threshold[1])]
            self.current_class = 2  # tag that which class should be focused on currently
        else:
            classes = list(classes)
            if not classes:
                raise ValueError('classes must name at least one label (or None)')
            thr = [float(threshold)] * len(classes) if np.ndim(threshold) == 0 else [float(t) for t in threshold]
            if len(thr) != len(classes):
                raise ValueError('threshold must be a float or hold one value per entry of classes')
            self.threshold = tuple(thr)
            self.cycle = [(None if c is None else int(c), t) for c, t in zip(classes, thr)]
            self.current_class = 0
        if int(patches) < 1:
            raise ValueError('patches must be >= 1')
        self.patches = int(patches)
        self.include_last = bool(include_last)
        self.random_state = random_state

    def _next_tags(self, n):
        tags = []
        for _ in range(n):
            tags.append(self.current_class)
            self.current_class = self.current_class + 1
            if self.current_class > len(self.cycle) - 1:
                self.current_class = 0
        return tags

    def __call__(self, sample):
        imgs, segs, single = _crop_batch(sample)
        window = tuple(int(v) for v in np.flipud(np.asarray(self.output_size)))
        size = window[0] * window[1] * window[2]
        N, P = int(imgs.shape[0]), self.patches
        tags = self._next_tags(N * P)
        seed = _crop_seed(self.random_state)

        def draw(lab, t, sample0):
            return ops.sample_crop_starts(lab, window, [self.cycle[k][0] for k in t], [crop_min_count(self.cycle[k][1], size) for k in t],
                                          seed, sample0=sample0, include_last=self.include_last)[0]
        if all(tags[n * P:(n + 1) * P] == tags[:P] for n in range(N)):
            starts = draw(segs, tags[:P], 0)
        else:                                            # the samples' tag sequences differ: one call per sample, the same draws
            starts = torch.cat([draw(segs[n:n + 1], tags[n * P:(n + 1) * P], n) for n in range(N)], 0)
        img, seg = ops.crop_gather(imgs, segs, starts, window)
        if single and P == 1:
            sample['class'] = tags[0]
            return _store(sample, img, seg, True)
        sample['class'] = tags
        return _store(sample, img, seg, False)


AUGMENTATIONS = {'rigid': RandomRigidTransform, 'bspline': RandomBSplineTransform, 'blur': GaussianBlur, 'bilateral': BilateralFilter,
                 'intensity': RandomIntensityTransform}
CROPS = {'crop': RandomCrop, 'balanced_crop': BalancedRandomCrop}       # patch sampling: they change the sample's shape


def make_augmentation(spec):
    """SegmentationExperiment's config['augment']: [[name, kwargs], ...] with name 'rigid', 'bspline', 'blur', 'bilateral', 'intensity',
    'crop' or 'balanced_crop' -> the transforms, in order.  (A config file has lists where the crops' asserts want tuples: output_size and
    threshold are converted.)"""
    out = []
    for name, kwargs in (spec or []):
        if name not in AUGMENTATIONS and name not in CROPS:
            raise ValueError("augmentation %r: one of %s" % (name, sorted(AUGMENTATIONS) + sorted(CROPS)))
        kwargs = dict(kwargs or {})
        if name in CROPS:
            for k in ('output_size', 'threshold'):
                if isinstance(kwargs.get(k), list):
                    kwargs[k] = tuple(kwargs[k])
        out.append((CROPS if name in CROPS else AUGMENTATIONS)[name](**kwargs))
    return out


# ---- preprocessing of raw volumes (lib/transforms.py:9-68, :262-284, :692-706) on csrc/preprocess.hip ------------------------------
# These act on the sample dict before or after SitkToTensor: image D x H x W or C x D x H x W, numpy or tensor, in the file's own dtype;
# sample['spacing'] is (x, y, z) = (W, H, D) axis, (1, 1, 1) when absent.

class Compose(object):
    """torchvision.transforms.Compose's contract (the reference composes its sample transforms with it): the transforms, in order."""

    def __init__(self, transforms):
        self.transforms = [t for t in transforms if t is not None]

    def __call__(self, sample):
        for t in self.transforms:
            sample = t(sample)
        return sample


def _to_kernel_volume(a):
    """numpy / tensor -> contiguous device tensor in a dtype the preprocessing kernels read (float32, float64, int16, uint8, int32); other
    dtypes are converted on upload, as SitkToTensor does."""
    t = _to_device_array(a)
    if t.dtype in ops.PREPROCESS_DTYPE_CODE:
        return t
    if t.dtype.is_floating_point:
        return t.to(torch.float32)
    if t.dtype in (torch.int8, torch.bool):
        return t.to(torch.int16 if t.dtype == torch.int8 else torch.uint8)
    return t.to(torch.int32)


class IdentityTransform(object):
    """lib/transforms.py:262-266."""

    def __call__(self, sample):
        return sample


class Resample(object):
    """lib/transforms.py:9-57 on the device: resample image and segmentation to `voxel_size` (one number, or (x, y, z)).  Per axis
    new_size = int(math.ceil(old_spacing * old_size / voxel_size)), output index o reads input index o * voxel_size / old_spacing (same origin and
    direction), by the table rule of ops.resample_axis_table; outside voxels get 0; sample['spacing'] is updated.  interpolator 'nearest' is
    the default for image and segmentation because that is what the reference executes (it passes interpolator 1, SimpleITK's nearest
    neighbour, although its docstring says linear); 'linear' applies to the image only (float32 out), the segmentation is always nearest.
    No anti-aliasing when down-sampling."""

    def __init__(self, voxel_size, interpolator='nearest'):
        if isinstance(voxel_size, (int, float)):
            voxel_size = (voxel_size,) * 3
        if len(voxel_size) != 3 or not all(float(v) > 0 and math.isfinite(float(v)) for v in voxel_size):
            raise ValueError('voxel_size: one positive number, or three (x, y, z); got %r' % (voxel_size,))
        if interpolator not in ops.RESAMPLE_INTERPOLATORS:
            raise ValueError("interpolator %r: 'nearest' or 'linear'" % (interpolator,))
        self.voxel_size = tuple(float(v) for v in voxel_size)
        self.interpolator = interpolator

    @staticmethod
    def new_size(old_size, old_spacing, voxel_size):
        """(x, y, z) sizes: the reference's :35-38."""
        return tuple(int(math.ceil(old_spacing[i] * old_size[i] / voxel_size[i])) for i in range(3))

    def __call__(self, sample):
        img = _to_kernel_volume(sample['image'])
        D, H, W = (int(s) for s in img.shape[-3:])
        spacing = tuple(float(s) for s in (sample.get('spacing') or (1.0, 1.0, 1.0)))
        nx, ny, nz = self.new_size((W, H, D), spacing, self.voxel_size)
        scale = tuple(self.voxel_size[k] / spacing[k] for k in (2, 1, 0))                     # (D, H, W) order
        sample['image'] = ops.resample_volume(img, (nz, ny, nx), scale, (0.0, 0.0, 0.0), self.interpolator, 0)
        if sample.get('segmentation') is not None:
            seg = _to_kernel_volume(sample['segmentation'])
            sample['segmentation'] = ops.resample_volume(seg, (nz, ny, nx), scale, (0.0, 0.0, 0.0), 'nearest', 0)
        sample['spacing'] = self.voxel_size
        return sample


class Normalization(object):
    """lib/transforms.py:59-68 on the device: ITK's NormalizeImageFilter, (x - mean) / sigma with the unbiased sigma over the finite voxels, as
    float32 (mean and sigma from two passes in double, rounded to float32 for the pointwise pass).  A constant volume gives zeros."""

    def __call__(self, sample):
        img = _to_kernel_volume(sample['image'])
        _, mean, var = ops.volume_moments(img)
        sample['image'] = ops.affine_intensity(img, mean, math.sqrt(var), clamp=False)
        return sample


class PercentileRescale(object):
    """The project's own transform (the reference's datasets were rescaled offline): (x - P_lo) / (P_hi - P_lo) as float32 with the exact `lo`
    / `hi` percentiles of the volume (numpy's linear rule), clamped to [0, 1] unless clamp=False -- the step raw MR intensities need before
    SitkToTensor's clamp to [0, 1] means anything.  P_hi == P_lo gives zeros."""

    def __init__(self, lo=0.5, hi=99.5, clamp=True):
        if not 0.0 <= float(lo) < float(hi) <= 100.0:
            raise ValueError('percentiles need 0 <= lo < hi <= 100, got %r and %r' % (lo, hi))
        self.lo, self.hi, self.clamp = float(lo), float(hi), bool(clamp)

    def __call__(self, sample):
        img = _to_kernel_volume(sample['image'])
        p_lo, p_hi = ops.volume_percentiles(img, (self.lo, self.hi))
        sample['image'] = ops.affine_intensity(img, p_lo, p_hi - p_lo, clamp=self.clamp)
        return sample


class LeftToRight(object):
    """lib/transforms.py:269-284 on the device: flips numpy axis 0 (z) of image and segmentation when 'LEFT' is in sample['name'] (a left knee
    shown as a right one).  Bit-exact; anything else passes through untouched."""

    @staticmethod
    def _flip0(vol):
        t = _to_kernel_volume(vol)
        D, H, W = (int(s) for s in t.shape[-3:])
        return ops.resample_volume(t, (D, H, W), (-1.0, 1.0, 1.0), (float(D - 1), 0.0, 0.0), 'nearest', 0)

    def __call__(self, sample):
        if 'LEFT' in sample['name']:
            sample['image'] = self._flip0(sample['image'])
            if sample.get('segmentation') is not None:
                sample['segmentation'] = self._flip0(sample['segmentation'])
        return sample


class SegmentationLabelFilter(object):
    """lib/transforms.py:692-706 on the device: every label in `ignore_labels` becomes 0, through one look-up table.  uint8 labels use a
    256-entry table; other integer labels are taken as int32 with a 65536-entry table, and labels outside it map to 0."""

    def __init__(self, ignore_labels):
        self.ignore_labels = [int(l) for l in ignore_labels]

    def __call__(self, sample):
        if sample.get('segmentation') is not None:
            seg = _to_kernel_volume(sample['segmentation'])
            if seg.dtype not in (torch.uint8, torch.int32):
                seg = seg.to(torch.int32)
            n = 256 if seg.dtype == torch.uint8 else ops.LABEL_LUT_MAX
            lut = np.arange(n, dtype=np.int32)
            for l in self.ignore_labels:
                if 0 <= l < n:
                    lut[l] = 0
            sample['segmentation'] = ops.label_lut(seg, lut)
        return sample


PREPROCESSING = {'resample': Resample, 'percentile_rescale': PercentileRescale, 'normalize': Normalization, 'left_to_right': LeftToRight,
                 'label_filter': SegmentationLabelFilter, 'identity': IdentityTransform}


def make_preprocess(spec):
    """config['preprocess']: [[name, kwargs], ...] with name 'resample', 'percentile_rescale', 'normalize', 'left_to_right', 'label_filter' or
    'identity' -> the transforms, in order (they run ahead of SitkToTensor)."""
    out = []
    for name, kwargs in (spec or []):
        if name not in PREPROCESSING:
            raise ValueError("preprocess step %r: one of %s" % (name, sorted(PREPROCESSING)))
        out.append(PREPROCESSING[name](**dict(kwargs or {})))
    return out


IMPORTANCE_WINDOWS = ('gaussian', 'constant')


def importance_window(tile, kind='gaussian', sigma_scale=0.125):
    """The per-axis tables (z, y, x) of the window that weights a tile's probabilities in blended sliding-window inference
    (ops.blend_accumulate; lib/inference.py): three float32 numpy vectors of tile[k] entries, the window is their product.
    'gaussian': exp(-(l - (t - 1) / 2)^2 / (2 (sigma_scale t)^2)), evaluated in float64 and rounded to float32 -- MONAI's / nnU-Net's
    window; being separable it needs no minimum clamp.  'constant': ones (plain averaging of the overlapping tiles)."""
    if kind not in IMPORTANCE_WINDOWS:
        raise ValueError("window %r: 'gaussian' or 'constant'" % (kind,))
    if len(tile) != 3 or any(int(t) != t or int(t) < 1 for t in tile):
        raise ValueError('tile takes three positive integers (z, y, x), got %r' % (tile,))
    sigma_scale = float(sigma_scale)
    if kind == 'gaussian' and not (sigma_scale > 0 and math.isfinite(sigma_scale)):
        raise ValueError('sigma_scale must be positive and finite, got %r' % (sigma_scale,))
    out = []
    for t in (int(v) for v in tile):
        if kind == 'constant':
            out.append(np.ones(t, dtype=np.float32))
        else:
            l = np.arange(t, dtype=np.float64)
            out.append(np.exp(-(l - (t - 1) / 2.0) ** 2 / (2.0 * (sigma_scale * t) ** 2)).astype(np.float32))
    return tuple(out)
