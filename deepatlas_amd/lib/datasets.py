"""Volume datasets: the synthetic ones of the BASELINE configs, and the reference's NIfTI list-file datasets (lib/datasets.py:16-328: a text
file of scan names plus a directory of .nii / .nii.gz files) read through lib/nifti.py instead of SimpleITK, with every transform of a
sample running on the device (lib/transforms.py).

Samples follow the reference's tuple convention (image 1 x D x H x W float in [0,1], segmentation D x H x W uint8,
name) (lib/datasets.py:150-166), so SegmentationExperiment consumes them unchanged.
"""
import os
from collections.abc import Sequence

import torch
from torch.utils.data import Dataset


def structured_labels(shape, n_classes, seed=0):
    """Blocky label map, a function of coordinates (Dice-parity inputs must be structured)."""
    D, H, W = shape
    z = torch.arange(D).view(D, 1, 1)
    y = torch.arange(H).view(1, H, 1)
    x = torch.arange(W).view(1, 1, W)
    bz, by, bx = max(D // 8, 1), max(H // 8, 1), max(W // 8, 1)
    lab = ((z // bz) * 5 + (y // by) * 3 + (x // bx) + seed) % n_classes
    return lab.to(torch.uint8)


class SyntheticSegDataset(Dataset):
    def __init__(self, n_samples, shape, n_classes, seed=230, noise=0.1):
        self.n, self.shape, self.n_classes, self.seed, self.noise = n_samples, tuple(shape), n_classes, seed, noise

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + i)
        lab = structured_labels(self.shape, self.n_classes, seed=i)
        img = lab.float() / max(self.n_classes - 1, 1) + self.noise * torch.rand(self.shape, generator=g)
        img = img.clamp_(0, 1).unsqueeze(0)
        return img, lab, 'synthetic_%d' % i


class SyntheticPairDataset(Dataset):
    """(moving image, target image, moving seg, target seg) pairs for the registration / joint configs."""

    def __init__(self, n_pairs, shape, n_classes, seed=230):
        self.seg = SyntheticSegDataset(n_pairs + 1, shape, n_classes, seed)
        self.n = n_pairs

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        im, sm, _ = self.seg[i]
        it, st_, _ = self.seg[i + 1]
        return im, it, sm, st_


def synthetic_batch_on_device(n, shape, n_classes, seed=230, device='cuda', structured=False, noise=0.1, sample0=0):
    """synthetic volumes generated in HBM by the HIP kernel da_synth_volume (no host tensor, no PCIe copy).
    Returns (image n x 1 x D x H x W float32 in [0,1], labels n x D x H x W uint8).  structured=False: iid throughput inputs
    (SURVEY.md 8d); structured=True: the blocky label / noisy image volumes of SyntheticSegDataset's kind (Dice-parity inputs)."""
    from .. import _native as nat
    D, H, W = (int(s) for s in shape)
    img = torch.empty((n, 1, D, H, W), dtype=torch.float32, device=device)
    lab = torch.empty((n, D, H, W), dtype=torch.uint8, device=device)
    nat.require_cuda(img)
    with torch.cuda.device(img.device):
        nat.call('da_synth_volume', nat.ptr(img), nat.ptr(lab), n, D, H, W, int(n_classes), 1 if structured else 0, float(noise),
                 int(seed) & 0xffffffff, int(sample0), nat.stream())
    return img, lab


class SegDataSetOAIZIB(Dataset):
    """lib/datasets.py:16-166: scans named in list files (one name per line; `txt_files` one file or a sequence of files, read in order as one
    list), stored under `data_dir` as NAME_image.nii.gz / NAME_masks.nii.gz.
    n_samples: an int keeps the first n lines, a sequence the lines with those indices (counted over all files), None all; anything else is a
    TypeError.  A sample is built as {'image', 'segmentation', 'name', 'spacing'} with the raw numpy arrays of lib/nifti.py (nz, ny, nx) and the
    file's spacing (x, y, z), run through pre_transform (once, at construction, when `preload`: the prepared device tensors are then kept) and
    through running_transform at every access.  __getitem__ returns (image, segmentation, name); with with_seg=False the segmentation is not
    read and the slot holds an empty tensor.  A missing file raises ValueError at load.  Meant for DataLoader(num_workers=0): the transforms
    launch kernels."""

    IMAGE_PATTERN = ('', '%s_image.nii.gz')
    SEGMENTATION_PATTERN = ('', '%s_masks.nii.gz')

    def __init__(self, txt_files, data_dir, with_seg=True, preload=False, pre_transform=None, running_transform=None, n_samples=None,
                 shuffle=False):
        self.n_samples = n_samples
        self.data_dir = data_dir
        self.with_seg = with_seg
        self.preload = preload
        self.pre_transform = pre_transform
        self.running_transform = running_transform
        self.shuffle = shuffle
        self.image_list, self.segmentation_list, self.name_list = self.read_image_segmentation_list(txt_files, data_dir, n_samples)
        if preload:
            self.sample_list = [self.load_sample(n, i, s if with_seg else None, pre_transform)
                                for i, s, n in zip(self.image_list, self.segmentation_list, self.name_list)]
        self.length = len(self.image_list)
        if shuffle:
            self.shuffle_id = torch.randperm(self.length)

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        if self.shuffle:
            i = int(self.shuffle_id[i])
        sample = self.get_sample(i)
        seg = sample.get('segmentation')
        return sample['image'], (seg if seg is not None else torch.empty(0, dtype=torch.uint8)), sample['name']

    def get_sample(self, i):
        if self.preload:
            sample = dict(self.sample_list[i])                # (a shallow copy: a running transform replaces entries, never the kept tensors)
        else:
            sample = self.load_sample(self.name_list[i], self.image_list[i], self.segmentation_list[i] if self.with_seg else None, self.pre_transform)
        if self.running_transform:
            sample = self.running_transform(sample)
        return sample

    @staticmethod
    def load_sample(name, image_file_name, segmentation_file_name=None, pre_transform=None):
        from .nifti import read_nifti
        if not os.path.exists(image_file_name):
            raise ValueError(image_file_name + ' not exist!')
        if segmentation_file_name and not os.path.exists(segmentation_file_name):
            raise ValueError(segmentation_file_name + ' not exist!')
        vol = read_nifti(image_file_name)
        sample = {'image': vol.array}
        if segmentation_file_name:
            sample['segmentation'] = read_nifti(segmentation_file_name).array
        sample['name'] = name
        sample['spacing'] = vol.spacing
        if pre_transform:
            sample = pre_transform(sample)
        return sample

    @classmethod
    def read_image_segmentation_list(cls, text_files, data_root='', n_samples=None):
        """(image paths, segmentation paths, names) of the kept lines; lines are counted over all files, kept or not."""
        if n_samples is not None and (isinstance(n_samples, (bool, str)) or not isinstance(n_samples, (int, Sequence))):
            raise TypeError("n_samples should be None, or int, or a sequence of int but get {}".format(type(n_samples)))
        if isinstance(text_files, str):
            text_files = [text_files]
        image_list, segmentation_list, name_list = [], [], []
        count = 0
        for text_file in text_files:
            with open(text_file) as f:
                for line in f:
                    index, count = count, count + 1
                    if isinstance(n_samples, int):
                        if index >= n_samples:
                            continue
                    elif n_samples is not None and index not in n_samples:
                        continue
                    name = line.strip("\n")
                    name_list.append(name)
                    image_list.append(os.path.join(data_root, cls.IMAGE_PATTERN[0], cls.IMAGE_PATTERN[1] % name))
                    segmentation_list.append(os.path.join(data_root, cls.SEGMENTATION_PATTERN[0], cls.SEGMENTATION_PATTERN[1] % name))
        return image_list, segmentation_list, name_list


class SegDataSetOASIS(SegDataSetOAIZIB):
    """lib/datasets.py:204-237: NAME_image.nii.gz / NAME_seg.nii.gz (lines counted as in SegDataSetOAIZIB; the reference's OASIS variant
    forgets to count the lines it skips, which is not copied)."""
    SEGMENTATION_PATTERN = ('', '%s_seg.nii.gz')


class SegDataSetBrains(SegDataSetOAIZIB):
    """lib/datasets.py:240-282 (LPBA40, CUMC12, IBSR18, MGH10): brain_affine_icbm_hist_matched/NAME.nii, label_affine_icbm_reID/NAME.nii."""
    IMAGE_PATTERN = ('brain_affine_icbm_hist_matched', '%s.nii')
    SEGMENTATION_PATTERN = ('label_affine_icbm_reID', '%s.nii')


class SegDataSetMindBoggle(SegDataSetOAIZIB):
    """lib/datasets.py:285-328: image_in_MNI152_normalized/NAME.nii.gz, label_31_reID_merged/NAME.nii.gz."""
    IMAGE_PATTERN = ('image_in_MNI152_normalized', '%s.nii.gz')
    SEGMENTATION_PATTERN = ('label_31_reID_merged', '%s.nii.gz')


NIFTI_SEG_DATASETS = {'OAI': SegDataSetOAIZIB, 'OASIS': SegDataSetOASIS, 'LPBA40': SegDataSetBrains, 'CUMC12': SegDataSetBrains,
                      'IBSR18': SegDataSetBrains, 'MGH10': SegDataSetBrains, 'MindBoggle': SegDataSetMindBoggle}


def get_seg_dataset(name):
    if name == 'synthetic':
        return SyntheticSegDataset
    if name in NIFTI_SEG_DATASETS:
        return NIFTI_SEG_DATASETS[name]
    raise KeyError("dataset '%s': 'synthetic' or one of the NIfTI list-file datasets %s" % (name, ', '.join(sorted(NIFTI_SEG_DATASETS))))


class SyntheticRegDataset(Dataset):
    """Ordered (moving, fixed) pairs over the volumes of a SyntheticSegDataset, enumerated as the reference's pairwise datasets do
    (lib/datasets.py:344-359): pair id -> fixed = id // (n - 1), moving = id % (n - 1), plus one when >= fixed; n (n - 1) pairs, no
    self-pairs.  Sample: (moving image, fixed image, moving segmentation, fixed segmentation, has_moving_seg, name).

    labeled: the volume indices that have a manual segmentation (None: all).  For an unlabelled MOVING volume the segmentation slot
    holds zeros and has_moving_seg is False (a flag, because default collation cannot batch None); the experiment turns it into
    seg_m=None.

    pairs: which of the n (n - 1) ordered pairs are enumerated, always in the reference's order with the excluded ones removed.
      'fixed_labeled' (default): the pairs whose FIXED volume is labelled; the 6-tuple above.
      'any_labeled': those, and the pairs with a labelled moving and an unlabelled fixed volume (the joint step's seg_t=None case: the warped
                     manual label is the fixed image's training target).
      'all':         every pair, the ones with no label on either side included (registration by image similarity alone).
    In the two wider modes a sample carries a seventh element has_fixed_seg, and an unlabelled fixed volume's segmentation slot holds zeros.

    moving_remap: None (default) | 'invert' (1 - x) | 'fold' (|2 x - 1|), applied to the MOVING image only: a pair of two "modalities" whose
    intensities are related by a decreasing / a non-monotonic map -- what a similarity for multi-modal registration has to cope with.  The
    segmentations are untouched."""

    PAIR_MODES = ('fixed_labeled', 'any_labeled', 'all')
    MOVING_REMAPS = (None, 'invert', 'fold')

    @staticmethod
    def remap_intensity(img, mode):
        """The intensity map of `moving_remap` on an image in [0, 1]."""
        if mode is None:
            return img
        if mode == 'invert':
            return 1.0 - img
        if mode == 'fold':
            return (2.0 * img - 1.0).abs()
        raise ValueError("moving_remap must be None, 'invert' or 'fold', got %r" % (mode,))

    def __init__(self, n_volumes, shape, n_classes, seed=230, labeled=None, pairs='fixed_labeled', moving_remap=None):
        if n_volumes < 2:
            raise ValueError('a pairwise dataset needs at least two volumes')
        if moving_remap not in self.MOVING_REMAPS:
            raise ValueError("moving_remap must be None, 'invert' or 'fold', got %r" % (moving_remap,))
        self.moving_remap = moving_remap
        if pairs not in self.PAIR_MODES:
            raise ValueError("pairs must be one of %s, got %r" % (', '.join(self.PAIR_MODES), pairs))
        self.pair_mode = pairs
        self.seg = SyntheticSegDataset(n_volumes, shape, n_classes, seed)
        self.n = n_volumes
        self.labeled = set(range(n_volumes)) if labeled is None else set(int(i) for i in labeled)
        keep = {'fixed_labeled': lambda m, f: f in self.labeled,
                'any_labeled': lambda m, f: f in self.labeled or m in self.labeled,
                'all': lambda m, f: True}[pairs]
        self.pairs = [p for p in (self.pair_of(i, n_volumes) for i in range(n_volumes * (n_volumes - 1))) if keep(*p)]

    @staticmethod
    def pair_of(pair_id, n):
        """(moving, fixed) volume indices of pair `pair_id` among n volumes."""
        fixed, moving = pair_id // (n - 1), pair_id % (n - 1)
        if moving >= fixed:
            moving += 1
        return moving, fixed

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        m, f = self.pairs[i]
        im, sm, name_m = self.seg[m]
        it, st_, name_f = self.seg[f]
        if self.moving_remap is not None:
            im = self.remap_intensity(im, self.moving_remap)
        has = m in self.labeled
        if not has:
            sm = torch.zeros_like(sm)
        name = '%s_to_%s' % (name_m, name_f)
        if self.pair_mode == 'fixed_labeled':
            return im, it, sm, st_, has, name
        has_fixed = f in self.labeled
        if not has_fixed:
            st_ = torch.zeros_like(st_)
        return im, it, sm, st_, has, name, has_fixed


class NiftiRegDataset(SyntheticRegDataset):
    """Ordered (moving, fixed) pairs over the volumes of a list-file dataset `seg_dataset` (any dataset of (image, segmentation, name) samples):
    SyntheticRegDataset's pair enumeration, `labeled` / `pairs` / `moving_remap` and sample tuples, with self.seg replaced."""

    def __init__(self, seg_dataset, labeled=None, pairs='fixed_labeled', moving_remap=None):
        n_volumes = len(seg_dataset)
        if n_volumes < 2:
            raise ValueError('a pairwise dataset needs at least two volumes')
        if moving_remap not in self.MOVING_REMAPS:
            raise ValueError("moving_remap must be None, 'invert' or 'fold', got %r" % (moving_remap,))
        if pairs not in self.PAIR_MODES:
            raise ValueError("pairs must be one of %s, got %r" % (', '.join(self.PAIR_MODES), pairs))
        self.moving_remap = moving_remap
        self.pair_mode = pairs
        self.seg = seg_dataset
        self.n = n_volumes
        self.labeled = set(range(n_volumes)) if labeled is None else set(int(i) for i in labeled)
        keep = {'fixed_labeled': lambda m, f: f in self.labeled,
                'any_labeled': lambda m, f: f in self.labeled or m in self.labeled,
                'all': lambda m, f: True}[pairs]
        self.pairs = [p for p in (self.pair_of(i, n_volumes) for i in range(n_volumes * (n_volumes - 1))) if keep(*p)]


def get_reg_dataset(name):
    """'synthetic': SyntheticRegDataset.  A NIfTI dataset name: a factory with the list-file signature plus labeled / pairs / moving_remap."""
    if name == 'synthetic':
        return SyntheticRegDataset
    if name in NIFTI_SEG_DATASETS:
        seg_type = NIFTI_SEG_DATASETS[name]

        def factory(txt_files, data_dir, with_seg=True, preload=False, pre_transform=None, running_transform=None, n_samples=None, shuffle=False,
                    labeled=None, pairs='fixed_labeled', moving_remap=None):
            seg = seg_type(txt_files, data_dir, with_seg=with_seg, preload=preload, pre_transform=pre_transform,
                           running_transform=running_transform, n_samples=n_samples, shuffle=shuffle)
            return NiftiRegDataset(seg, labeled=labeled, pairs=pairs, moving_remap=moving_remap)
        return factory
    raise KeyError("dataset '%s': 'synthetic' or one of the NIfTI list-file datasets %s" % (name, ', '.join(sorted(NIFTI_SEG_DATASETS))))
