"""Synthetic volume datasets for the BASELINE configs (the reference's NIfTI list-file datasets,
lib/datasets.py:16-478, are host file I/O and out of scope).

Samples follow the reference's tuple convention (image 1 x D x H x W float in [0,1], segmentation D x H x W uint8,
name) (lib/datasets.py:150-166), so SegmentationExperiment consumes them unchanged.
"""
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


def get_seg_dataset(name):
    if name == 'synthetic':
        return SyntheticSegDataset
    raise KeyError("dataset '%s': only 'synthetic' is available (NIfTI datasets need SimpleITK, out of scope)" % name)


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


def get_reg_dataset(name):
    if name == 'synthetic':
        return SyntheticRegDataset
    raise KeyError("dataset '%s': only 'synthetic' is available (NIfTI datasets need SimpleITK, out of scope)" % name)
