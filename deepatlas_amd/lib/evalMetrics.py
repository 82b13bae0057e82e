"""Evaluation Dice on the device (models/segmentation.py:188-194 + lib/evalMetrics.py:17-21,58-68,184-217).

The reference copies 629 MB of logits to the host and makes 31 numpy passes per volume; here one kernel does the
first-max argmax and exact integer overlap counts, so the per-class Dice 2|P&T|/(|P|+|T|) is bit-equal to the
reference's scipy value whenever the argmax is equal (NaN when a class is absent from both, like scipy).
"""
import numpy as np
import torch

from .. import ops


def eval_dice_counts(logits, truth):
    """(counts[N][C][3] int64 on device, pred uint8)."""
    return ops.argmax_dice_counts(logits, truth)


def dice_from_counts(counts):
    """counts[..., 3] = (|P|, |T|, |P&T|) -> float64 numpy Dice, NaN where |P|+|T| == 0."""
    c = counts.detach().cpu().numpy().astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return 2.0 * c[..., 2] / (c[..., 0] + c[..., 1])


def _as_device_labels(a):
    """numpy / torch label map (bool masks included) -> one flattened uint8 / int64 sample on the current device."""
    t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype.is_floating_point:
        t = t.to(torch.int64)
    if not t.is_cuda:
        t = t.to(torch.device('cuda', torch.cuda.current_device()))
    return t.reshape(1, -1)


def metricEval(eval_metric, output, gt, num_labels=None):
    """lib/evalMetrics.py:17-100.  Two call forms:
      * the accelerated evaluation loop (models/segmentation.py:188-194 collapsed into one kernel): metricEval('dice', logits N x C x D x H x W,
        truth N x D x H x W) -> per-class Dice of classes 1..C-1 for every volume, ndarray [N][C-1];
      * the reference's own signature on LABEL MAPS (numpy or torch, bool masks included), `output` and `gt` squeezed and flattened as one
        volume: 'iou' = mean over the num_labels labels of |P & T| / |P | T| (0 for a label absent from gt; lib/evalMetrics.py:36-57);
        'dice' (num_labels == 2) = 2 |P & T| / (|P| + |T|) of the non-zero voxels (1 - scipy dice, :59-68; NaN when both are empty);
        'recall' = TP / |T|, 'precision' = TP / |P| of label 1 (:73-100; ZeroDivisionError when the denominator is empty, as there).
      All four come from the three integer counts per label of ONE pass over the two maps (da_label_overlap_counts)."""
    if eval_metric == 'dice' and torch.is_tensor(output) and output.dtype.is_floating_point and output.dim() == 5:
        counts, _ = eval_dice_counts(output, gt)
        return dice_from_counts(counts)[:, 1:]
    if eval_metric not in ('iou', 'dice', 'recall', 'precision'):
        raise ValueError('Invalid evaluation metric value: %r' % (eval_metric,))
    if num_labels is None:
        raise ValueError('num_labels is required for label-map metrics')
    if eval_metric != 'iou' and num_labels != 2:
        raise NotImplementedError('%s evaluation score is only implemented for 2 labels' % eval_metric)
    p, t = _as_device_labels(output), _as_device_labels(gt)
    if p.shape != t.shape:
        raise AssertionError('pred shape %s gt shape %s' % (tuple(p.shape), tuple(t.shape)))
    c = ops.label_overlap_counts(p, t, num_labels)[0].cpu().numpy().astype(np.float64)      # [num_labels][3] = (|P|, |T|, |P & T|)
    if eval_metric == 'iou':
        union = c[:, 0] + c[:, 1] - c[:, 2]
        present = c[:, 1] != 0
        per = np.zeros(num_labels)
        per[present] = c[present, 2] / union[present]
        return float(per.sum() / float(num_labels))
    n_p, n_t, tp = c[1]
    if eval_metric == 'dice':
        with np.errstate(invalid='ignore', divide='ignore'):
            return float(np.float64(2.0 * tp) / np.float64(n_p + n_t))
    if eval_metric == 'recall':
        return tp / n_t if n_t != 0 else (_ for _ in ()).throw(ZeroDivisionError('float division by zero'))
    return tp / n_p if n_p != 0 else (_ for _ in ()).throw(ZeroDivisionError('float division by zero'))


def _n_class_of(*masks):
    """`max(torch.unique(a).max(), torch.unique(b).max()) + 1` of the reference (lib/evalMetrics.py:198, lib/loss.py:367)."""
    return int(max(int(m.max().item()) for m in masks)) + 1


def get_multiclass_dice(pred, truth, n_class=None, eps=1e-11):
    """lib/evalMetrics.py:184-217: per-class Dice of two index masks, background (class 0) dropped: scores B x (n_class-1)
    float32 = 2|P&T| / (|P| + |T| + eps).  The reference builds both one-hot tensors and sums them in fp32 (exact below
    2^24 voxels); here the counts are exact integers from one pass over the two label maps.
    `truth` may also be a one-hot B x C x D x M x N mask (lib/evalMetrics.py:207-208)."""
    assert pred.shape[0] == truth.shape[0]
    assert pred.shape[-3:] == truth.shape[-3:]
    if pred.dim() + 1 == truth.dim():                 # one-hot truth -> index mask (exact for 0/1 masks)
        oh = truth
        if n_class is None:
            n_class = oh.shape[1]
        if not bool(((oh == 0) | (oh == 1)).all()) or not bool((oh.sum(1) == 1).all()):
            raise NotImplementedError('soft (non one-hot) truth is outside the accelerated eval path')
        truth = oh.argmax(1)
    if n_class is None:
        n_class = _n_class_of(truth, pred)
    c = ops.label_overlap_counts(pred, truth, n_class).to(torch.float32)
    return (2. * c[:, 1:, 2]) / ((c[:, 1:, 0] + c[:, 1:, 1]) + eps)


def cal_metric_from_counts(n_pred, n_gt, n_both, eps=1e-11):
    """lib/evalMetrics.py:151-181 cal_metric from the three counts of one (sample, label): -1 everywhere when the label is
    absent from the ground truth."""
    res = {'iou': -1, 'dice': -1, 'recall': -1, 'precision': -1}
    if n_gt != 0:
        tp = float(n_both); fn = float(n_gt - n_both); fp = float(n_pred - n_both)
        union = float(n_pred + n_gt - n_both)
        res['iou'] = tp / (union + eps)
        res['recall'] = tp / (tp + fn + eps)
        res['precision'] = tp / (tp + fp + eps)
        res['dice'] = 2 * tp / (2 * tp + fn + fp + eps)
    return res


def get_multi_metric(pred, gt, eval_label_list=None, rm_bg=False):
    """lib/evalMetrics.py:103-148: iou / dice / recall / precision per (sample, label) plus the label- and batch-averages
    that skip the -1 entries; same dictionary layout (float64 numpy arrays).  pred / gt: device label maps B x ...
    (the reference takes numpy arrays and makes one host pass per label and sample over Python sets)."""
    pred_t = pred if torch.is_tensor(pred) else torch.as_tensor(np.asarray(pred))
    gt_t = gt if torch.is_tensor(gt) else torch.as_tensor(np.asarray(gt))
    dev = pred_t.device if pred_t.is_cuda else (gt_t.device if gt_t.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    pred_t, gt_t = pred_t.to(dev), gt_t.to(dev)
    if int(min(int(pred_t.min().item()), int(gt_t.min().item()))) < 0:
        raise ValueError('labels must be non-negative')
    n_class = _n_class_of(gt_t, pred_t)
    counts = ops.label_overlap_counts(pred_t, gt_t, n_class).cpu().numpy()          # B x n_class x 3
    label_list = np.nonzero(counts[:, :, 1].sum(0))[0].tolist()                       # == np.unique(gt).tolist()
    if rm_bg:
        label_list = label_list[1:]
    if eval_label_list is not None:
        for label in eval_label_list:
            assert label in label_list, "label {} is not in label_list".format(label)
        label_list = eval_label_list
    num_label, num_batch = len(label_list), counts.shape[0]
    metrics = ['iou', 'dice', 'recall', 'precision']
    multi_metric_res = {m: np.zeros([num_batch, num_label]) for m in metrics}
    label_avg_res = {m: np.zeros([num_batch, 1]) for m in metrics}
    batch_avg_res = {m: np.zeros([1, num_label]) for m in metrics}
    for l, lab in enumerate(label_list):
        for b in range(num_batch):
            r = cal_metric_from_counts(int(counts[b, lab, 0]), int(counts[b, lab, 1]), int(counts[b, lab, 2]))
            for m in metrics:
                multi_metric_res[m][b][l] = r[m]
    with np.errstate(invalid='ignore'), __import__('warnings').catch_warnings():
        __import__('warnings').simplefilter('ignore', category=RuntimeWarning)
        for m in metrics:
            for s_ in range(num_batch):
                row = multi_metric_res[m][s_]
                label_avg_res[m][s_] = float(np.mean(row[np.where(row != -1)]))
            for l in range(num_label):
                col = multi_metric_res[m][:, l]
                batch_avg_res[m][:, l] = float(np.mean(col[np.where(col != -1)]))
    return {'multi_metric_res': multi_metric_res, 'label_avg_res': label_avg_res, 'batch_avg_res': batch_avg_res,
            'label_list': label_list}


def registration_dice(seg_m, seg_t, disp, n_class):
    """Hard-label registration Dice (the DeepAtlas registration metric): the moving segmentation warped with the predicted deformation
    (nearest neighbour, ops.warp_labels_nearest) against the target segmentation, classes 1..n_class-1, for every pair of the batch:
    float64 ndarray [N][n_class-1], NaN where a class is absent from both maps (the convention of metricEval('dice', ...)).
    seg_m / seg_t: N x D x H x W label maps, disp: N x 3 x D x H x W; one kernel, exact integer counts."""
    return dice_from_counts(ops.reg_label_counts(seg_m, seg_t, disp, n_class))[:, 1:]


def jacobian_stats(disp):
    """Regularity of the deformation x -> x + u(x): per-sample float64 arrays `mean`, `std` (population), `min`, `max` of det J,
    `n_nonpos` = number of voxels with det J <= 0 (folding) and `nonpos_frac` = that number over the voxel count."""
    s = ops.jacobian_det(disp).cpu().numpy()
    n_vox = float(np.prod(disp.shape[2:]))
    return {'mean': s[:, 5].copy(), 'std': np.sqrt(s[:, 6]), 'min': s[:, 2].copy(), 'max': s[:, 3].copy(),
            'n_nonpos': s[:, 4].copy(), 'nonpos_frac': s[:, 4] / n_vox}


def inverse_consistency(disp_ab, disp_ba):
    """How far the two directions' fields are from being inverses of each other: per-sample float64 arrays of the composition residual
    r(x) = u_ab(x) + u_ba(x + u_ab(x)) in voxels: `mean_vox` (mean Euclidean norm), `rms_vox`, `max_vox`, and `outside_frac` = the share of
    voxels whose sample point x + u_ab(x) leaves the volume (u_ba reads zeros there).  ops.inverse_consistency_stats on the host."""
    s = ops.inverse_consistency_stats(disp_ab, disp_ba)
    return {k: v.cpu().numpy() for k, v in s.items()}


def invert_deformation(disp, **kw):
    """The inverse field of `disp` (ops.invert_field; `kw` are its max_iters and tol_vox) and how well the iteration did: returns
    (inverse N x 3 x D x H x W on the device, dict of per-sample float64 arrays): `max_update_vox` (the largest final update, infinite for a
    non-finite field), `unconverged_frac` (share of voxels whose final update exceeds tol_vox), `mean_iters` (updates per voxel) and
    `outside_frac` (share of voxels whose inverse point lies outside the volume, where the field was extrapolated by its border value)."""
    inv, stats = ops.invert_field(disp, return_stats=True, **kw)
    s = stats.cpu().numpy()
    n_vox = float(np.prod(disp.shape[2:]))
    return inv, {'max_update_vox': s[:, 0].copy(), 'unconverged_frac': s[:, 1] / n_vox, 'mean_iters': s[:, 2] / n_vox, 'outside_frac': s[:, 3] / n_vox}


def _landmark_norms(diff, spacing):
    """Per-sample (mean, std, max) of |spacing * diff| over the rows of `diff` (N x P x 3 float64 numpy) that are finite; NaN without one."""
    e = np.sqrt(((diff * np.asarray(spacing, dtype=np.float64).reshape(1, 1, 3)) ** 2).sum(-1))
    out = np.full((3, e.shape[0]), np.nan)
    for n in range(e.shape[0]):
        row = e[n][np.isfinite(e[n])]
        if row.size:
            out[:, n] = row.mean(), row.std(), row.max()
    return out


def target_registration_error(disp, fixed_points, moving_points, spacing=(1, 1, 1)):
    """Landmark error of a predicted field: the fixed-frame landmarks f (N x P x 3, voxel index coordinates (x, y, z)) are carried into the
    moving frame, f + s u(f) (ops.transport_points), and compared with their moving-frame partners m: per-sample float64 arrays `tre_mean`,
    `tre_std`, `tre_max` of |spacing * (f + s u(f) - m)| over the P pairs, and `initial_mean`, `initial_max`, the same for disp = 0.
    `spacing` is the voxel size per (x, y, z) axis; pairs with a NaN in either point are skipped."""
    f = torch.as_tensor(fixed_points, dtype=torch.float32, device=disp.device)
    m = torch.as_tensor(moving_points, dtype=torch.float32)
    if f.dim() != 3 or tuple(f.shape) != tuple(m.shape):
        raise ValueError('fixed_points and moving_points must both be N x P x 3, got %s and %s' % (tuple(f.shape), tuple(m.shape)))
    if len(spacing) != 3:
        raise ValueError('spacing takes one voxel size per axis (x, y, z), got %r' % (spacing,))
    skip = (~torch.isfinite(f).all(-1)).cpu().numpy() | (~torch.isfinite(m).all(-1)).cpu().numpy()
    moved = ops.transport_points(disp, torch.nan_to_num(f)).cpu().double().numpy()
    f64, m64 = f.cpu().double().numpy(), m.cpu().double().numpy()
    moved[skip] = np.nan
    f64[skip] = np.nan
    tre = _landmark_norms(moved - m64, spacing)
    init = _landmark_norms(f64 - m64, spacing)
    return {'tre_mean': tre[0], 'tre_std': tre[1], 'tre_max': tre[2], 'initial_mean': init[0], 'initial_max': init[2]}


def known_deformation_field(names, size, amp_vox, lip, device):
    """One smooth random field per name, N x 3 x D x H x W float32 in normalised units on `device`: a 4 x 4 x 4 lattice of normal values per
    component from a generator seeded by zlib.crc32(name), trilinearly up-sampled (align_corners=True) to `size`, scaled to a largest
    displacement of amp_vox voxels and then, if needed, down until its Lipschitz bound -- the largest difference of the displacement between
    axis-adjacent voxels, in voxels, times sqrt(3) -- is at most `lip`."""
    import zlib
    D, H, W = (int(s) for s in size)
    fields = []
    for name in names:
        g = torch.Generator().manual_seed(zlib.crc32(str(name).encode()) & 0xffffffff)
        lattice = torch.randn((1, 3, 4, 4, 4), generator=g, dtype=torch.float64)
        u = torch.nn.functional.interpolate(lattice, size=(D, H, W), mode='trilinear', align_corners=True)
        u = u * (float(amp_vox) / float(u.pow(2).sum(1).sqrt().max()))
        step = max(float((u[:, :, 1:] - u[:, :, :-1]).pow(2).sum(1).sqrt().max()), float((u[:, :, :, 1:] - u[:, :, :, :-1]).pow(2).sum(1).sqrt().max()),
                   float((u[..., 1:] - u[..., :-1]).pow(2).sum(1).sqrt().max()))
        bound = step * 3.0 ** 0.5
        if bound > lip:
            u = u * (lip / bound)
        fields.append(u)
    scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)], dtype=torch.float64).view(1, 3, 1, 1, 1)
    return (torch.cat(fields, 0) * scale).float().to(device)


def known_deformation_tre(model, image, names, amp_vox=3.0, n_points=1000, lip=0.5):
    """Landmark error of a registration net against a deformation whose inverse is known.  Every image of the batch (N x 1 x D x H x W) is
    deformed by a smooth random field g (known_deformation_field, seeded by the sample's name): moving = WarpFn(image, g), that is
    moving(x) = image(x + g(x)).  The net registers moving to image and wants moving(x + u(x)) ~ image(x), so u(x) + g(x + u(x)) = 0: the true
    answer u* is the inverse of g, ops.invert_field(g, tol_vox=1e-4, max_iters=64).  n_points landmarks f per sample, uniform and at least
    amp_vox + 1 voxels from every face (seeded by the name as well), are carried through both fields (ops.transport_points).
    Returns a dict of per-sample float64 arrays: `tre_mean_vox`, `tre_max_vox` of |s (u(f) - u*(f))|, `tre_initial_mean_vox` = the mean of
    |s u*(f)| (what no registration leaves) and `truth_unconverged_frac`, the share of voxels at which u* did not converge."""
    import zlib
    N = int(image.shape[0])
    D, H, W = (int(s) for s in image.shape[2:])
    if len(names) != N:
        raise ValueError('known_deformation_tre needs one name per image, got %d names for %d images' % (len(names), N))
    margin = float(amp_vox) + 1.0
    if min(D, H, W) - 1 <= 2 * margin:
        raise ValueError('a volume of %s has no point %g voxels from every face' % ((D, H, W), margin))
    with torch.no_grad():
        g = known_deformation_field(names, (D, H, W), amp_vox, lip, image.device)
        moving = ops.WarpFn.apply(image.float(), g)[0]
        truth, stats = ops.invert_field(g, tol_vox=1e-4, max_iters=64, return_stats=True)
        u = model(moving, image)[0].detach().float()
        pts = []
        for name in names:
            gen = torch.Generator().manual_seed((zlib.crc32(str(name).encode()) + 1) & 0xffffffff)
            r = torch.rand((int(n_points), 3), generator=gen, dtype=torch.float64)
            lo = torch.tensor([margin] * 3, dtype=torch.float64)
            hi = torch.tensor([W - 1 - margin, H - 1 - margin, D - 1 - margin], dtype=torch.float64)
            pts.append(lo + r * (hi - lo))
        f = torch.stack(pts).float().to(image.device)
        at_truth = ops.transport_points(truth, f).cpu().double().numpy()
        at_pred = ops.transport_points(u, f).cpu().double().numpy()
    tre = _landmark_norms(at_truth - at_pred, (1, 1, 1))
    init = _landmark_norms(at_truth - f.cpu().double().numpy(), (1, 1, 1))
    return {'tre_mean_vox': tre[0], 'tre_max_vox': tre[2], 'tre_initial_mean_vox': init[0],
            'truth_unconverged_frac': stats[:, 1].cpu().numpy() / float(D * H * W)}


def affine_align(moving, fixed, **kw):
    """Affine pre-alignment of a batch of pairs (lib/affine.py affine_register; `kw` are its arguments: mode, sim, sim_settings, levels,
    iters, lr, init): returns (theta N x 3 x 4, the moving images resampled with it, N x 1 x D x H x W), both on the device, no autograd.
    ops.affine_disp(theta, u) turns theta and a field u predicted on the aligned image into the one field that warps the ORIGINAL moving
    image and its labels."""
    from . import affine
    theta = affine.affine_register(moving, fixed, **kw)
    with torch.no_grad():
        aligned = ops.AffineWarpFn.apply(moving.detach(), theta)
    return theta, aligned


def atlas_label_fusion(labels, disp, weights=None, n_targets=None):
    """Multi-atlas label fusion (ops.label_fusion): the atlas label maps `labels` (K x D x H x W, or (N K) x D x H x W per target) warped
    with the fields `disp` ((N K) x 3 x D x H x W, atlas index fastest) and voted per voxel -- majority vote, or weighted by `weights`
    (N x K per atlas, N x K x D x H x W per voxel).  N comes from `weights`, else from shared K x D x H x W maps, else from `n_targets`
    (default 1: without it an unweighted batch of per-target maps is one target with N K atlases).  Returns the fused map, uint8 N x D x H x W."""
    return ops.label_fusion(labels, disp, weights, n_targets=n_targets)


ATLAS_FUSION_MODES = ('majority', 'local')


def atlas_segmentation(reg_model, atlas_images, atlas_labels, target_image, mode='majority', radius=2, sigma=0.1, chunk=4):
    """Registration-based segmentation of one image from K labelled atlases: the registration net (in eval mode, `chunk` pairs at a time)
    registers every atlas image (moving) to the target image (fixed), the atlas label maps are warped with those fields (nearest
    neighbour) and fused per voxel.  mode 'majority': every atlas one vote.  mode 'local': locally weighted voting -- the atlas images
    are warped with the same fields (ops.WarpFn) and atlas k votes at voxel x with exp(-m_k(x) / (2 sigma^2)), m_k the mean squared
    difference to the target over the (2 radius + 1)^3 window (ops.local_msd_weights).
    atlas_images: K x 1 x D x H x W (or K x D x H x W) float32, atlas_labels: K x D x H x W uint8 / int64, target_image: any shape with
    D H W voxels; all on the registration net's device.  Returns (fused uint8 1 x D x H x W, confidence float32 1 x D x H x W).
    Its Dice: dice_from_counts(ops.label_overlap_counts(fused, truth, n_class))."""
    if mode not in ATLAS_FUSION_MODES:
        raise ValueError("mode must be one of %s, got %r" % (', '.join(ATLAS_FUSION_MODES), mode))
    if atlas_images.dim() == 4:
        atlas_images = atlas_images[:, None]
    K = int(atlas_images.shape[0])
    D, H, W = (int(s) for s in atlas_images.shape[-3:])
    if tuple(atlas_labels.shape) != (K, D, H, W):
        raise ValueError('atlas_labels must be K x D x H x W matching atlas_images')
    target = target_image.reshape(1, 1, D, H, W)
    chunk = max(int(chunk), 1)
    was_training = reg_model.training
    fields, warped = [], []
    with torch.no_grad():
        reg_model.eval()
        try:
            for k0 in range(0, K, chunk):
                im = atlas_images[k0:k0 + chunk]
                disp = reg_model(im, target.expand(im.shape[0], 1, D, H, W).contiguous())[0]
                fields.append(disp)
                if mode == 'local':
                    warped.append(ops.WarpFn.apply(im, disp)[0])
        finally:
            reg_model.train(was_training)
        disp = fields[0] if len(fields) == 1 else torch.cat(fields, 0)
        weights = None
        if mode == 'local':
            w = warped[0] if len(warped) == 1 else torch.cat(warped, 0)
            weights = ops.local_msd_weights(w.reshape(1, K, D, H, W), target[:, 0], radius=radius, sigma=sigma)
        return ops.label_fusion(atlas_labels, disp, weights, return_confidence=True, n_targets=1)


def largest_component_filter(pred, n_class, connectivity=6):
    """The usual clean-up of a predicted label map before it is scored or used: of every class 1..n_class-1 only the largest connected
    component of each sample stays, every island becomes background (ops.keep_largest_component, on the device).  pred: N x D x H x W
    uint8 / int32 / int64; returns a map of the same dtype."""
    return ops.keep_largest_component(pred, n_class, connectivity=connectivity)


def component_stats(labels, n_class, connectivity=6):
    """How fragmented a label map is, per sample and class: a dict of numpy arrays [N][n_class] -- `n_components` (int64), `voxels` (int64,
    the class's voxel count) and `largest_frac` (float64, the share of the class's voxels that lie in its largest component; NaN for a class
    without voxels).  Row 0 (background) is 0 / NaN."""
    _, stats = ops.keep_largest_component(labels, n_class, connectivity=connectivity, return_stats=True)
    s = stats.cpu().numpy()
    with np.errstate(invalid='ignore', divide='ignore'):
        frac = s[:, :, 1].astype(np.float64) / s[:, :, 2].astype(np.float64)
    return {'n_components': s[:, :, 0].copy(), 'largest_frac': frac, 'voxels': s[:, :, 2].copy()}


POSTPROCESS_MODES = ('largest_cc', 'min_size')


def parse_postprocess(spec):
    """config['postprocess'] -> None or the dict {'mode', 'connectivity', 'min_size'}.  Accepted: None, 'largest_cc', or a dict with 'mode' in
    POSTPROCESS_MODES and optionally 'connectivity' (6 / 18 / 26, default 6) and 'min_size' (>= 1; required for mode 'min_size')."""
    if spec is None:
        return None
    if isinstance(spec, str):
        spec = {'mode': spec}
    if not isinstance(spec, dict):
        raise ValueError("postprocess must be None, 'largest_cc' or a dict, got %r" % (spec,))
    unknown = set(spec) - {'mode', 'connectivity', 'min_size'}
    if unknown:
        raise ValueError('postprocess: unknown keys %s' % sorted(unknown))
    mode = spec.get('mode')
    if mode not in POSTPROCESS_MODES:
        raise ValueError('postprocess mode must be one of %s, got %r' % (', '.join(POSTPROCESS_MODES), mode))
    connectivity = spec.get('connectivity', 6)
    if connectivity not in ops.CC_CONNECTIVITIES:
        raise ValueError('postprocess connectivity must be 6, 18 or 26, got %r' % (connectivity,))
    min_size = spec.get('min_size')
    if mode == 'min_size':
        if min_size is None or int(min_size) < 1:
            raise ValueError("postprocess mode 'min_size' needs min_size >= 1, got %r" % (min_size,))
        min_size = int(min_size)
    elif min_size is not None:
        raise ValueError("postprocess: min_size belongs to mode 'min_size'")
    return {'mode': mode, 'connectivity': int(connectivity), 'min_size': min_size}


def postprocess_labels(pred, n_class, post, return_stats=False):
    """Applies a parsed postprocess setting (parse_postprocess) to a label map N x D x H x W on the device."""
    if post['mode'] == 'largest_cc':
        return ops.keep_largest_component(pred, n_class, connectivity=post['connectivity'], return_stats=return_stats)
    return ops.remove_small_components(pred, n_class, post['min_size'], connectivity=post['connectivity'], return_stats=return_stats)


SURFACE_METRIC_KEYS = ('spacing', 'connectivity', 'percentile', 'classes')


def parse_surface_metrics(spec):
    """config['surface_metrics'] -> None (off) or the keyword dict of surface_distances.  Accepted: None, True, or a dict with any of the
    keys `spacing` (sD, sH, sW), `connectivity` (6 / 18 / 26), `percentile` (in (0, 100]) and `classes`; the defaults are unit spacing,
    6, 95 and the classes 1 .. n_class - 1."""
    if spec is None or spec is False:
        return None
    if spec is True:
        spec = {}
    if not isinstance(spec, dict):
        raise ValueError('surface_metrics must be None, True or a dict, got %r' % (spec,))
    unknown = set(spec) - set(SURFACE_METRIC_KEYS)
    if unknown:
        raise ValueError('surface_metrics: unknown keys %s' % sorted(unknown))
    connectivity = spec.get('connectivity', 6)
    if connectivity not in ops.SURFACE_CONNECTIVITIES:
        raise ValueError('surface_metrics connectivity must be 6, 18 or 26, got %r' % (connectivity,))
    percentile = float(spec.get('percentile', 95.0))
    if not 0.0 < percentile <= 100.0:
        raise ValueError('surface_metrics percentile must be in (0, 100], got %r' % (spec.get('percentile'),))
    spacing = tuple(float(v) for v in spec.get('spacing', (1.0, 1.0, 1.0)))
    if len(spacing) != 3 or not all(0.0 < v < float('inf') for v in spacing):
        raise ValueError('surface_metrics spacing must be three positive finite numbers, got %r' % (spec.get('spacing'),))
    classes = spec.get('classes')
    return {'spacing': spacing, 'connectivity': int(connectivity), 'percentile': percentile,
            'classes': None if classes is None else [int(c) for c in classes]}


def surface_distances(pred, truth, n_class, **kw):
    """Surface-distance metrics per sample and class (ops.surface_distance_stats, on the device): a dict of numpy arrays [N][K'], one per
    column of ops.SURFACE_STATS -- the surface voxel counts `n_pred` and `n_truth` (int64), and `hd`, `hd_pct` (the `percentile`-th
    percentile, HD95 by default), `assd`, `asd_pred_truth`, `asd_truth_pred` (float64, NaN where the class is absent from either map).
    pred: logits N x C x D x H x W (argmaxed as eval_dice_counts does) or a label map N x D x H x W; truth: a label map.
    kw: classes, spacing, connectivity, percentile."""
    truth = truth.to(pred.device)
    if truth.dtype not in (torch.uint8, torch.int32, torch.int64):
        truth = truth.long()
    if pred.dim() == 5:
        pred = eval_dice_counts(pred, truth)[1]
    truth = truth.reshape(pred.shape)
    s = ops.surface_distance_stats(pred, truth, n_class, **kw).cpu().numpy()
    out = {name: s[:, :, i].copy() for i, name in enumerate(ops.SURFACE_STATS)}
    out['n_pred'] = out['n_pred'].astype(np.int64)
    out['n_truth'] = out['n_truth'].astype(np.int64)
    return out
