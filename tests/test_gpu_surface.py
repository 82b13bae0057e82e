"""GPU: the surface predicate and the surface-distance metrics (Hausdorff, its percentile, ASSD; deepatlas_amd/csrc/edt.hip) against the
scipy + numpy references of surface_cases.py.  At unit spacing the surface voxel counts and hd are compared by exact equality (d^2 is an
integer, its double root is scipy's own); hd_pct, assd and the two asd within STAT_RTOL = 1e-12, relative."""
import argparse

import numpy as np
import pytest
import torch

import surface_cases as sc

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the cases are read-only arrays)
    return t if dtype is None else t.to(dtype)


def check_stats(got, want, rtol, exact_hd=True, tag=''):
    """got: the op's float64 N x K' x 7 tensor; want: the reference.  Every figure is printed before it is asserted."""
    g = got.cpu().numpy()
    assert got.dtype == torch.float64 and g.shape == want.shape, (tag, g.shape, want.shape)
    ok = ~np.isnan(want)
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(ok & (want != 0), np.abs(g - want) / np.abs(want), np.abs(g - np.where(ok, want, 0.0)))
    worst = float(np.nanmax(np.where(ok, rel, 0.0)[..., 2:])) if ok[..., 2:].any() else 0.0
    print('%s: %d defined of %d segments, largest relative distance of a metric from the reference %.3e (bound %.1e)'
          % (tag, int(ok[..., 2].sum()), ok[..., 2].size, worst, rtol))
    assert np.array_equal(g[..., :2], want[..., :2]), tag                    # the surface voxel counts
    assert np.array_equal(np.isnan(g), np.isnan(want)), tag                  # NaN exactly where a class is absent from a map
    if exact_hd:
        assert np.array_equal(g[..., 2], want[..., 2], equal_nan=True), tag
    assert np.all(np.abs(g[ok] - want[ok]) <= rtol * np.abs(want[ok])), (tag, worst)


# ---- the surface predicate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', sc.CONNECTIVITIES)
@pytest.mark.parametrize('shape', sc.SURFACE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_label_surface_equals_the_erosion_reference(shape, connectivity):
    from deepatlas_amd import ops
    labels = sc.blocky_labels(shape, 4, block=sc.BLOCK, seed=11, n=2)
    want = sc.label_surface(labels, connectivity)
    for dtype in (torch.uint8, torch.int32, torch.int64):
        t = dev(labels, dtype)
        before = t.clone()
        got = ops.label_surface(t, connectivity)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), (shape, connectivity, dtype)
        assert torch.equal(t, before)
    # the samples do not see each other: each sample alone gives its half
    for n in range(2):
        assert np.array_equal(ops.label_surface(dev(labels[n:n + 1]), connectivity).cpu().numpy(), want[n:n + 1])
    # one label everywhere: the surface is the volume's shell -- every face, edge and corner
    full = np.full((1,) + tuple(shape), 3, dtype=np.uint8)
    assert np.array_equal(ops.label_surface(dev(full), connectivity).cpu().numpy(), sc.label_surface(full, connectivity))


# ---- the metrics at unit spacing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('name', sc.STAT_IDS)
def test_stats_at_unit_spacing(name, kind):
    from deepatlas_amd import ops
    pred, truth = sc.case_maps(name, kind)
    n_class = sc.STAT_CASES[name][2]
    got = ops.surface_distance_stats(dev(pred), dev(truth), n_class)
    check_stats(got, sc.case_reference(name, kind), sc.STAT_RTOL, tag='%s/%s' % (name, kind))


@pytest.mark.parametrize('connectivity', (18, 26))
def test_stats_at_the_other_connectivities(connectivity):
    from deepatlas_amd import ops
    for name in ('small', 'chunks'):
        pred, truth = sc.case_maps(name, 'noisy')
        got = ops.surface_distance_stats(dev(pred), dev(truth), sc.STAT_CASES[name][2], connectivity=connectivity)
        check_stats(got, sc.case_reference(name, 'noisy', connectivity=connectivity), sc.STAT_RTOL, tag='%s/conn%d' % (name, connectivity))


@pytest.mark.parametrize('percentile', (50.0, 95.0, 100.0))
def test_percentiles(percentile):
    from deepatlas_amd import ops
    for name in ('small', 'tall', 'K32'):
        pred, truth = sc.case_maps(name, 'shifted')
        got = ops.surface_distance_stats(dev(pred), dev(truth), sc.STAT_CASES[name][2], percentile=percentile)
        check_stats(got, sc.case_reference(name, 'shifted', percentile=percentile), sc.STAT_RTOL, tag='%s/p%g' % (name, percentile))
        if percentile == 100.0:
            assert torch.equal(torch.nan_to_num(got[..., 3]), torch.nan_to_num(got[..., 2])), 'the 100th percentile is hd itself'


def test_absent_filling_identical_and_far_apart():
    from deepatlas_amd import ops
    # N = 2, class 2 absent from the prediction of sample 1 only: NaN for that entry alone, its counts still reported
    pred, truth = (a.copy() for a in sc.case_maps('small', 'noisy'))
    assert (truth[1] == 2).any() and (pred[1] == 2).any()
    pred[1][pred[1] == 2] = 0
    want = sc.stats_scipy(pred, truth, [1, 2, 3])
    assert np.isnan(want[1, 1, 2:]).all() and not np.isnan(np.delete(want.reshape(6, 7), 4, 0)).any() and want[1, 1, 1] > 0
    check_stats(ops.surface_distance_stats(dev(pred), dev(truth), 4), want, sc.STAT_RTOL, tag='absent')
    # a class filling a sample of the truth
    pred, truth = (a.copy() for a in sc.case_maps('chunks', 'noisy'))
    truth[0] = 1
    check_stats(ops.surface_distance_stats(dev(pred), dev(truth), 4), sc.stats_scipy(pred, truth, [1, 2, 3]), sc.STAT_RTOL, tag='filling')
    # pred is truth: every defined metric is 0
    t = dev(truth)
    same = ops.surface_distance_stats(t, t, 4).cpu().numpy()
    assert np.array_equal(same[..., 0], same[..., 1]) and np.all(same[..., 2:][~np.isnan(same[..., 2:])] == 0.0)
    assert np.array_equal(same, sc.stats_scipy(truth, truth, [1, 2, 3]), equal_nan=True)
    # two single voxels far apart: the closed form, at unit and at anisotropic spacing
    a, b = np.zeros((1, 9, 70, 11), dtype=np.uint8), np.zeros((1, 9, 70, 11), dtype=np.uint8)
    a[0, 0, 0, 0] = b[0, 8, 69, 10] = 1
    far = ops.surface_distance_stats(dev(a), dev(b), 2).cpu().numpy()[0, 0]
    d = np.sqrt(8.0 ** 2 + 69.0 ** 2 + 10.0 ** 2)
    assert np.array_equal(far, [1, 1, d, d, d, d, d]), far
    far = ops.surface_distance_stats(dev(a), dev(b), 2, spacing=sc.ANISO).cpu().numpy()[0, 0]
    d = np.sqrt((8 * sc.ANISO[0]) ** 2 + (69 * sc.ANISO[1]) ** 2 + (10 * sc.ANISO[2]) ** 2)
    assert np.array_equal(far[:2], [1, 1]) and np.all(np.abs(far[2:] - d) <= sc.ANISO_RTOL * d), far


def test_labels_outside_the_classes_dtypes_class_lists_and_views():
    from deepatlas_amd import ops
    # labels >= n_class belong to no class: maps with labels 0 .. 7 scored with n_class = 4
    truth = sc.blocky_labels((5, 6, 70), 8, block=sc.BLOCK, seed=21, n=2)
    pred = sc.noisy(truth, 8, 22)
    pred[0, 0, 0, :3] = 255
    want = sc.stats_scipy(pred, truth, [1, 2, 3])
    check_stats(ops.surface_distance_stats(dev(pred), dev(truth), 4), want, sc.STAT_RTOL, tag='labels >= n_class')
    # the three dtypes, mixed between pred and truth (255 of the uint8 map stays 255, and a negative label is no class either)
    for pt, tt in ((torch.uint8, torch.int64), (torch.int32, torch.uint8), (torch.int64, torch.int32), (torch.int32, torch.int32)):
        got = ops.surface_distance_stats(dev(pred, pt), dev(truth, tt), 4)
        check_stats(got, want, sc.STAT_RTOL, tag='%s/%s' % (pt, tt))
    neg = dev(pred, torch.int64)
    neg[neg == 255] = -7
    check_stats(ops.surface_distance_stats(neg, dev(truth, torch.int32), 4), want, sc.STAT_RTOL, tag='negative labels')
    # a class list with gaps, the background in it, in another order
    classes = [5, 0, 2]
    got = ops.surface_distance_stats(dev(pred), dev(truth), 8, classes=classes)
    check_stats(got, sc.stats_scipy(pred, truth, classes), sc.STAT_RTOL, tag='classes %r' % classes)
    # non-contiguous views give the result of their contiguous copies and are left untouched
    big_p = torch.zeros((2, 5, 6, 140), dtype=torch.uint8, device=DEV)
    big_p[..., ::2] = dev(pred)
    big_t = dev(truth, torch.int64).permute(0, 3, 1, 2).contiguous()
    vp, vt = big_p[..., ::2], big_t.permute(0, 2, 3, 1)
    assert not vp.is_contiguous() and not vt.is_contiguous()
    snap_p, snap_t = big_p.clone(), big_t.clone()
    check_stats(ops.surface_distance_stats(vp, vt, 4), want, sc.STAT_RTOL, tag='views')
    assert np.array_equal(ops.label_surface(vp).cpu().numpy(), sc.label_surface(pred, 6))
    assert torch.equal(big_p, snap_p) and torch.equal(big_t, snap_t)


# ---- anisotropic spacing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('name', sc.STAT_IDS)
def test_stats_at_anisotropic_spacing(name, kind):
    from deepatlas_amd import ops
    pred, truth = sc.case_maps(name, kind)
    got = ops.surface_distance_stats(dev(pred), dev(truth), sc.STAT_CASES[name][2], spacing=sc.ANISO)
    check_stats(got, sc.case_reference(name, kind, spacing=sc.ANISO), sc.ANISO_RTOL, exact_hd=False, tag='%s/%s aniso' % (name, kind))


# ---- the class-group loop --------------------------------------------------------------------------------------------------------------
def test_group_loop_equals_the_single_class_calls_and_scipy():
    from deepatlas_amd import ops
    pred, truth = sc.group_maps()
    p, t = dev(pred), dev(truth)
    got = ops.surface_distance_stats(p, t, sc.GROUP_LABELS, classes=sc.GROUP_CLASSES)
    assert not torch.isnan(got).any()
    for j, c in enumerate(sc.GROUP_CLASSES):
        one = ops.surface_distance_stats(p, t, sc.GROUP_LABELS, classes=[c])
        assert torch.equal(one[:, 0], got[:, j]), c                            # bit for bit
    cols = [sc.GROUP_CLASSES.index(c) for c in sc.GROUP_CHECKED]
    check_stats(got[:, cols], sc.group_reference(), sc.STAT_RTOL, tag='group loop')


def test_repeats_are_bit_identical():
    from deepatlas_amd import ops
    pred, truth = sc.case_maps('tall', 'noisy')
    p, t = dev(pred), dev(truth)
    first = ops.surface_distance_stats(p, t, 4)
    for _ in range(2):
        again = ops.surface_distance_stats(p, t, 4)
        assert torch.equal(torch.nan_to_num(first, nan=-1.0), torch.nan_to_num(again, nan=-1.0))


def test_eval_metrics_wrapper():
    from deepatlas_amd.lib import evalMetrics as metrics
    pred, truth = sc.case_maps('small', 'noisy')
    want = sc.case_reference('small', 'noisy')
    got = metrics.surface_distances(dev(pred), dev(truth, torch.int64), 4)
    assert list(got) == list(sc.STATS) and got['n_pred'].dtype == np.int64
    check_stats(torch.from_numpy(np.stack([got[k].astype(np.float64) for k in sc.STATS], -1)), want, sc.STAT_RTOL, tag='wrapper')
    # logits are argmaxed first
    logits = torch.nn.functional.one_hot(dev(pred, torch.int64), 4).permute(0, 4, 1, 2, 3).float().contiguous()
    again = metrics.surface_distances(logits, dev(truth, torch.int64), 4)
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in sc.STATS)


# ---- the experiment --------------------------------------------------------------------------------------------------------------------
def _run_experiment(log_root, capsys, **args):
    """One epoch of training with its validation, then test() on the checkpoint it saved; returns the printed text and the last eval's results."""
    import train_seg
    from deepatlas_amd import ops
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                            data_root='./data', log_root=str(log_root), shape=[32, 32, 32], **args)
    exp = SegmentationExperiment(train_seg.build_config(ns))
    ops.set_deterministic(True)
    exp.train()
    dice_per_class, dice_avg = exp.test(best=False)
    return {'exp': exp, 'out': capsys.readouterr().out, 'dice': (dice_per_class.clone(), float(dice_avg)),
            'extra': dict(getattr(exp, 'eval_extra', None) or {})}


def _nanmean(a, axis=None):
    ok = ~np.isnan(a)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(ok, a, 0.0).sum(axis) / ok.sum(axis)


def test_experiment_with_and_without_surface_metrics(tmp_path, capsys):
    """One epoch of SegmentationExperiment on the smallest synthetic configuration (one 32^3 sample).  Without the key: eval_extra empty,
    no suffix, the lines in the parent commit's format.  With it: the raw Dice is the same and the surface entries equal the scipy
    reference on the host copy of the same argmax.  With `postprocess` as well: the post_ entries too."""
    import re
    from deepatlas_amd.lib import evalMetrics as metrics
    plain = _run_experiment(tmp_path / 'a', capsys)
    surf = _run_experiment(tmp_path / 'b', capsys, surface_metrics=True, surface_spacing=None, surface_percentile=None)
    both = _run_experiment(tmp_path / 'c', capsys, surface_metrics=True, surface_spacing=[1.0, 0.7, 2.5], surface_percentile=90.0,
                           postprocess='largest-cc', cc_connectivity=None, cc_min_size=None)
    line = r'Validation: Dice Avg: (\d\.\d{4}|nan) \(\d+\.\d{3} sec\) \d\d/\d\d/\d\d \d\d:\d\d:\d\d'
    hd = r', HD95 Avg: (\d+\.\d\d|nan), ASSD Avg: (\d+\.\d\d|nan)'
    assert 'surface_metrics' not in plain['exp'].config and plain['extra'] == {}
    assert plain['exp']._surface_suffix() == '' and plain['exp']._post_suffix() == '' and 'HD95' not in plain['out']
    val = [l for l in plain['out'].splitlines() if l.startswith('Validation:')]
    assert len(val) == 1 and re.fullmatch(line, val[0]), val
    tst = [l for l in plain['out'].splitlines() if l.startswith('Testing Model:')]
    assert len(tst) == 1 and re.fullmatch(r'Testing Model: \S+checkpoint\.pth\.tar \(1 epochs\)  Dice_avg: ([0-9.e-]+|nan)', tst[0]), tst
    # the raw Dice and the experiment's name do not depend on the key
    for other in (surf, both):
        assert torch.equal(torch.nan_to_num(plain['dice'][0]), torch.nan_to_num(other['dice'][0]))
        assert other['exp'].exp_name == plain['exp'].exp_name
    keys = {'hd95_per_class', 'assd_per_class', 'hd_per_class', 'hd95_avg', 'assd_avg', 'surface_undefined_frac'}
    assert set(surf['extra']) == keys and surf['exp']._post_suffix() == ''
    sval = [l for l in surf['out'].splitlines() if l.startswith('Validation:')]
    assert len(sval) == 1 and re.fullmatch(line + hd, sval[0]), sval
    assert sum(bool(re.search(hd + '$', l)) for l in surf['out'].splitlines() if l.startswith('Testing Model:')) == 1
    assert set(both['extra']) == keys | {'post_' + k for k in keys} | {'post_dice_per_class', 'post_dice_avg', 'components_per_class', 'removed_frac'}
    bval = [l for l in both['out'].splitlines() if l.startswith('Validation:')]
    assert len(bval) == 1 and re.fullmatch(line + hd + r', post-processed Dice Avg: (\d\.\d{4}|nan) \(\d+\.\d components / class\)' + hd, bval[0]), bval

    # the same numbers through the scipy reference from the same argmax (test() evaluated the checkpoint now in exp.model)
    def recompute(run, clean, **kw):
        exp = run['exp']
        n_class = exp.config['n_classes']
        rows = []
        with torch.no_grad():
            exp.model.eval()
            for images, truths, _ in exp.validation_data_loader:
                _, lab = metrics.eval_dice_counts(exp.model(images.to(exp.device)), truths.to(exp.device))
                if clean:
                    lab = metrics.largest_component_filter(lab, n_class)
                rows.append(sc.stats_scipy(lab.cpu().numpy(), truths.numpy().reshape(lab.shape), list(range(1, n_class)), **kw))
        return np.concatenate(rows, 0)

    def compare(extra, prefix, ref, rtol):
        for key, col in (('hd95_per_class', 3), ('assd_per_class', 4), ('hd_per_class', 2)):
            want, got = _nanmean(ref[..., col], 0), extra[prefix + key]
            assert np.array_equal(np.isnan(got), np.isnan(want)), key
            ok = ~np.isnan(want)
            assert np.all(np.abs(got[ok] - want[ok]) <= rtol * np.abs(want[ok])), (prefix, key)
        for key, col in (('hd95_avg', 3), ('assd_avg', 4)):
            want = _nanmean(_nanmean(ref[..., col], 0))
            assert (np.isnan(want) and np.isnan(extra[prefix + key])) or abs(extra[prefix + key] - want) <= 2 * rtol * abs(want), key
        assert extra[prefix + 'surface_undefined_frac'] == np.isnan(ref[..., 4]).mean()
    compare(surf['extra'], '', recompute(surf, False), sc.STAT_RTOL)
    aniso = dict(spacing=(1.0, 0.7, 2.5), percentile=90.0)
    compare(both['extra'], '', recompute(both, False, **aniso), sc.ANISO_RTOL)
    compare(both['extra'], 'post_', recompute(both, True, **aniso), sc.ANISO_RTOL)
