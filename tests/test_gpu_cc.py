"""GPU: connected components, largest-component and minimum-size clean-up (deepatlas_amd/csrc/cc.hip) against the scipy reference of
cc_cases.py.  Every result is an integer and every comparison exact equality.  Every case is checked for the root map, the sizes,
compact=True, both filters and their statistics, at connectivities 6, 18 and 26."""
import numpy as np
import pytest
import torch

import cc_cases as cc

pytestmark = pytest.mark.gpu

N_CLASS = 4
DEV = 'cuda'


def _tile():
    from deepatlas_amd import ops
    return ops.CC_TILE


def check_case(name, batch, n_class=N_CLASS, min_sizes=(1, 2, 5)):
    """All outputs of the three ops on `batch` (numpy N x D x H x W) against the shared reference, at every connectivity."""
    from deepatlas_amd import ops
    lab = torch.from_numpy(np.ascontiguousarray(batch)).to(DEV)
    before = lab.clone()
    for conn in cc.CONNECTIVITIES:
        ref = cc.reference(name, batch, conn, n_class)
        roots, sizes = ops.connected_components(lab, conn, return_sizes=True)
        assert roots.dtype == torch.int32 and sizes.dtype == torch.int32 and tuple(roots.shape) == batch.shape
        assert np.array_equal(roots.cpu().numpy(), ref.roots), (name, conn, 'roots')
        assert np.array_equal(sizes.cpu().numpy(), ref.sizes), (name, conn, 'sizes')
        compact = ops.connected_components(lab, conn, compact=True)
        assert compact.dtype == torch.int32 and np.array_equal(compact.cpu().numpy(), ref.compact), (name, conn, 'compact')
        kept, stats = ops.keep_largest_component(lab, n_class, conn, return_stats=True)
        assert kept.dtype == lab.dtype and stats.dtype == torch.int64 and tuple(stats.shape) == (batch.shape[0], n_class, 3)
        assert np.array_equal(kept.cpu().numpy(), ref.largest), (name, conn, 'largest')
        assert np.array_equal(stats.cpu().numpy(), ref.stats), (name, conn, 'stats')
        assert torch.equal(ops.keep_largest_component(lab, n_class, conn), kept)
        for ms in min_sizes:
            want = np.stack([cc.ref_remove_small(v, r, s, n_class, ms) for v, r, s in zip(batch, ref.class_roots, ref.class_sizes)])
            got, st = ops.remove_small_components(lab, n_class, ms, conn, return_stats=True)
            assert got.dtype == lab.dtype and np.array_equal(got.cpu().numpy(), want), (name, conn, 'min_size', ms)
            assert np.array_equal(st.cpu().numpy(), ref.stats), (name, conn, 'min_size stats', ms)
            assert torch.equal(ops.remove_small_components(lab, n_class, ms, conn), got)
    assert torch.equal(lab, before), 'the input is not modified'
    return lab


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 70), (1, 9, 1), (3, 5, 7), (2, 5, 20)])
def test_small_shapes_and_extents_of_one(shape):
    """Extents of 1, (3, 5, 7) and a shape smaller than one tile (one workgroup, no seam pass); (1, 1, 70) has three tiles in a row."""
    td, th, tw = _tile()
    assert (2 < td or 5 < th or 20 < tw) and 2 <= td and 5 <= th and 20 <= tw
    for density, seed in ((0.31, 11), (0.6, 12), (1.0, 13)):
        check_case('small%s_%s' % (shape, density), cc.noise(shape, density, seed))


@pytest.mark.parametrize('dtype', [np.uint8, np.int32, np.int64])
@pytest.mark.parametrize('which', ['ragged', '17x19x23'])
def test_noise_on_ragged_multi_tile_shapes(which, dtype):
    shape = cc.ragged_shape(_tile()) if which == 'ragged' else (17, 19, 23)
    for density, seed in ((0.12, 21), (0.31, 22), (0.6, 23)):
        check_case('noise_%s_%s_%s' % (which, density, np.dtype(dtype).name), cc.noise(shape, density, seed, dtype=dtype), min_sizes=(1, 3, 40))


@pytest.mark.parametrize('dtype', [np.uint8, np.int64])
def test_labels_outside_n_class_act_as_background(dtype):
    """Labels 1..6 with n_class = 4: 4, 5 and 6 separate the components of 1..3 like background and are 0 in the cleaned maps; a negative
    label (int64) is background everywhere."""
    batch = cc.noise(cc.ragged_shape(_tile()), 0.7, 31, n_labels=6, dtype=dtype)
    if dtype == np.int64:
        batch[0, ::3, ::2, ::5] = -2
        batch[0, 1::3, ::2, 1::5] = 2 ** 40 + 1                # differs from label 1 only above bit 32
    lab = check_case('outside_%s' % np.dtype(dtype).name, batch)
    from deepatlas_amd import ops
    kept = ops.keep_largest_component(lab, N_CLASS)
    assert int(kept.max()) <= 3 and int(kept.min()) == 0


def test_pairs_across_tile_seams():
    """A voxel pair straddling a tile face, edge and corner (every direction a following neighbour can take), all else background: joined
    exactly under the connectivities that join them; two different labels face to face are never joined."""
    from deepatlas_amd import ops
    tile = _tile()
    for kind in ('face', 'edge', 'corner'):
        batch = cc.seam_pairs(kind, tile)
        lab = check_case('seam_' + kind, batch, min_sizes=(1, 2, 3))
        for conn in cc.CONNECTIVITIES:
            roots = ops.connected_components(lab, conn)
            n_comp = [int(torch.unique(r).numel()) - 1 for r in roots]
            assert n_comp == [1 if conn in cc.SEAM_JOINED[kind] else 2] * len(batch), (kind, conn, n_comp)
        two = cc.seam_pairs(kind, tile, second_label=2)
        lab = check_case('seam2_' + kind, two, min_sizes=(1, 2))
        for conn in cc.CONNECTIVITIES:
            assert all(int(torch.unique(r).numel()) == 3 for r in ops.connected_components(lab, conn))


def test_rows_planes_and_samples_do_not_wrap():
    from deepatlas_amd import ops
    for shape in ((3, 5, 7), cc.ragged_shape(_tile())):
        lab = check_case('wrap%s' % (shape,), cc.wrap_around(shape), min_sizes=(1, 2))
        for conn in cc.CONNECTIVITIES:
            roots, sizes = ops.connected_components(lab, conn, return_sizes=True)
            assert int((sizes == 1).sum()) == 6 and int(sizes.sum()) == 6


@pytest.mark.parametrize('which', ['9x8x130', 'ragged'])
def test_serpentine_deep_parent_chains(which):
    """A one-voxel-wide path through every tile, many times: one component of known size whose root is its first voxel; with one voxel
    removed in the middle, two."""
    from deepatlas_amd import ops
    shape = (9, 8, 130) if which == '9x8x130' else cc.ragged_shape(_tile())
    n = len(cc.serpentine_path(shape))
    lab = check_case('serpentine_' + which, cc.serpentine(shape), min_sizes=(1, n, n + 1))
    for conn in cc.CONNECTIVITIES:
        roots, sizes = ops.connected_components(lab, conn, return_sizes=True)
        assert torch.unique(roots).tolist() == [0, 1] and int(sizes[0, 0, 0, 0]) == n and int(sizes.sum()) == n
    cut = check_case('serpentine_cut_' + which, cc.serpentine(shape, cut=True), min_sizes=(1, n // 2))
    for conn in cc.CONNECTIVITIES:
        roots, sizes = ops.connected_components(cut, conn, return_sizes=True)
        assert torch.unique(roots).numel() == 3 and int(roots[0, 0, 0, 0]) == 1 and int(sizes.sum()) == n - 1


def test_extremes():
    from deepatlas_amd import ops
    shape = cc.ragged_shape(_tile())
    V = int(np.prod(shape))
    zero = check_case('zeros', np.zeros((1,) + shape, dtype=np.uint8))
    assert int(ops.connected_components(zero).abs().sum()) == 0
    ones = check_case('ones', np.ones((1,) + shape, dtype=np.uint8), min_sizes=(1, V, V + 1))
    for conn in cc.CONNECTIVITIES:
        roots, sizes = ops.connected_components(ones, conn, return_sizes=True)
        assert bool((roots == 1).all()) and int(sizes[0, 0, 0, 0]) == V and int(sizes.sum()) == V
    board = check_case('checkerboard', cc.checkerboard((17, 19, 23)), min_sizes=(1, 2))
    roots6 = ops.connected_components(board, 6)
    idx = torch.arange(board.numel(), device=DEV, dtype=torch.int32).reshape(board.shape) + 1
    assert torch.equal(roots6, torch.where(board > 0, idx, torch.zeros_like(idx)))          # every voxel its own component
    assert torch.unique(ops.connected_components(board, 26)).tolist() == [0, 1]              # the set half is one component


def test_ties_go_to_the_smallest_root_and_absent_classes_leave_zero_rows():
    from deepatlas_amd import ops
    shape = cc.ragged_shape(_tile())
    two = cc.blobs(shape, [(5, 10, 40), (0, 12, 3)], (2, 3, 4), label=2)
    three = cc.blobs(shape, [(5, 10, 40), (1, 1, 30), (0, 12, 3)], (2, 3, 4), label=1)
    three[0, 6:8, 0:2, 0:2] = 3                                  # a second class; class 2 is absent from this sample
    for name, batch, cls, first in (('tie2', two, 2, (0, 12, 3)), ('tie3', three, 1, (0, 12, 3))):
        lab = check_case(name, batch, min_sizes=(1, 24, 25))
        for conn in cc.CONNECTIVITIES:
            kept, stats = ops.keep_largest_component(lab, N_CLASS, conn, return_stats=True)
            n_blobs = 2 if name == 'tie2' else 3
            assert stats[0, cls].tolist() == [n_blobs, 24, 24 * n_blobs]
            want = cc.blobs(shape, [first], (2, 3, 4), label=cls)
            if name == 'tie3':
                want[0, 6:8, 0:2, 0:2] = 3
                assert stats[0, 2].tolist() == [0, 0, 0] and stats[0, 3].tolist() == [1, 8, 8]
            assert np.array_equal(kept.cpu().numpy(), want)
            assert stats[0, 0].tolist() == [0, 0, 0]


def test_remove_small_components_thresholds():
    """min_size = 1 is the identity, a planted blob stays at its size and goes at its size + 1."""
    from deepatlas_amd import ops
    shape = cc.ragged_shape(_tile())
    batch = cc.blobs(shape, [(2, 6, 28)], (3, 4, 8), label=1)         # 96 voxels across tile seams in every axis
    batch[0, 0, 0, 0:5] = 2
    lab = torch.from_numpy(batch).to(DEV)
    for conn in cc.CONNECTIVITIES:
        assert torch.equal(ops.remove_small_components(lab, N_CLASS, 1, conn), lab)
        at = ops.remove_small_components(lab, N_CLASS, 96, conn)
        assert int((at == 1).sum()) == 96 and int((at == 2).sum()) == 0
        above = ops.remove_small_components(lab, N_CLASS, 97, conn)
        assert int(above.sum()) == 0
    check_case('planted', batch, min_sizes=(1, 5, 6, 96, 97))


def test_batch_of_three_equals_three_single_samples():
    from deepatlas_amd import ops
    shape = cc.ragged_shape(_tile())
    samples = [cc.noise(shape, 0.31, 41), cc.serpentine(shape), cc.blobs(shape, [(5, 10, 40), (0, 12, 3)], (2, 3, 4), label=2)]
    batch = np.concatenate(samples)
    lab = check_case('batch3', batch, min_sizes=(1, 4))
    for conn in cc.CONNECTIVITIES:
        roots, sizes = ops.connected_components(lab, conn, return_sizes=True)
        kept, stats = ops.keep_largest_component(lab, N_CLASS, conn, return_stats=True)
        for n in range(3):
            r1, s1 = ops.connected_components(lab[n:n + 1], conn, return_sizes=True)
            k1, t1 = ops.keep_largest_component(lab[n:n + 1], N_CLASS, conn, return_stats=True)
            assert torch.equal(r1[0], roots[n]) and torch.equal(s1[0], sizes[n]) and torch.equal(k1[0], kept[n]) and torch.equal(t1[0], stats[n])


def test_repeats_are_bit_identical_and_views_equal_their_copies():
    from deepatlas_amd import ops
    shape = cc.ragged_shape(_tile())
    lab = torch.from_numpy(cc.noise(shape, 0.6, 51)).to(DEV)
    first = None
    for _ in range(5):
        roots, sizes = ops.connected_components(lab, 26, return_sizes=True)
        kept, stats = ops.keep_largest_component(lab, N_CLASS, 26, return_stats=True)
        small = ops.remove_small_components(lab, N_CLASS, 7, 26)
        got = (roots, sizes, kept, stats, small)
        if first is None:
            first = got
        assert all(torch.equal(a, b) for a, b in zip(first, got))
    # a non-contiguous view gives the result of its contiguous copy, and is left untouched
    big = torch.from_numpy(cc.noise((shape[0], shape[1], 2 * shape[2]), 0.5, 52)).to(DEV)
    view = big[:, :, :, ::2]
    assert not view.is_contiguous()
    snapshot = big.clone()
    for conn in cc.CONNECTIVITIES:
        assert torch.equal(ops.connected_components(view, conn), ops.connected_components(view.contiguous(), conn))
        assert torch.equal(ops.keep_largest_component(view, N_CLASS, conn), ops.keep_largest_component(view.contiguous(), N_CLASS, conn))
    assert torch.equal(big, snapshot)


def test_eval_metrics_wrappers():
    from deepatlas_amd.lib import evalMetrics as metrics
    shape = cc.ragged_shape(_tile())
    batch = cc.noise(shape, 0.4, 61)
    lab = torch.from_numpy(batch).to(DEV)
    ref = cc.reference('metrics', batch, 18, N_CLASS)
    assert np.array_equal(metrics.largest_component_filter(lab, N_CLASS, connectivity=18).cpu().numpy(), ref.largest)
    s = metrics.component_stats(lab, N_CLASS, connectivity=18)
    assert np.array_equal(s['n_components'], ref.stats[:, :, 0]) and np.array_equal(s['voxels'], ref.stats[:, :, 2])
    with np.errstate(invalid='ignore'):
        assert np.array_equal(s['largest_frac'], ref.stats[:, :, 1] / ref.stats[:, :, 2].astype(np.float64), equal_nan=True)


def _run_experiment(log_root, capsys, **post_args):
    """One epoch of training with its validation, then test() on the checkpoint it saved; returns the printed text and the last eval's results."""
    import argparse
    import train_seg
    from deepatlas_amd import ops
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                            data_root='./data', log_root=str(log_root), shape=[32, 32, 32], **post_args)
    exp = SegmentationExperiment(train_seg.build_config(ns))
    ops.set_deterministic(True)
    exp.train()
    dice_per_class, dice_avg = exp.test(best=False)
    return {'exp': exp, 'out': capsys.readouterr().out, 'dice': (dice_per_class.clone(), float(dice_avg)),
            'extra': dict(getattr(exp, 'eval_extra', None) or {})}


def test_experiment_with_and_without_postprocess(tmp_path, capsys):
    """One epoch of SegmentationExperiment on the smallest synthetic configuration (one 32^3 sample), with and without `postprocess`.
    Without: no `post-processed` text, eval_extra empty, the lines in the parent commit's format.  With: the raw Dice is the same and
    post_dice_* equals the Dice computed here with scipy on the host copy of the same prediction."""
    import re
    from deepatlas_amd.lib import evalMetrics as metrics
    plain = _run_experiment(tmp_path / 'a', capsys)
    post = _run_experiment(tmp_path / 'b', capsys, postprocess='largest-cc', cc_connectivity=18, cc_min_size=None)
    assert 'postprocess' not in plain['exp'].config and post['exp'].config['postprocess'] == {'mode': 'largest_cc', 'connectivity': 18}
    assert 'post-processed' not in plain['out'] and plain['extra'] == {}
    val = [l for l in plain['out'].splitlines() if l.startswith('Validation:')]
    assert len(val) == 1 and re.fullmatch(r'Validation: Dice Avg: (\d\.\d{4}|nan) \(\d+\.\d{3} sec\) \d\d/\d\d/\d\d \d\d:\d\d:\d\d', val[0]), val
    tst = [l for l in plain['out'].splitlines() if l.startswith('Testing Model:')]
    assert len(tst) == 1 and re.fullmatch(r'Testing Model: \S+checkpoint\.pth\.tar \(1 epochs\)  Dice_avg: ([0-9.e-]+|nan)', tst[0]), tst
    # the raw Dice does not depend on the key
    assert torch.equal(torch.nan_to_num(plain['dice'][0]), torch.nan_to_num(post['dice'][0]))
    assert plain['dice'][1] == post['dice'][1] or (np.isnan(plain['dice'][1]) and np.isnan(post['dice'][1]))
    extra = post['extra']
    assert set(extra) == {'post_dice_per_class', 'post_dice_avg', 'components_per_class', 'removed_frac'}
    pval = [l for l in post['out'].splitlines() if l.startswith('Validation:')]
    assert len(pval) == 1 and re.fullmatch(r'Validation: Dice Avg: (\d\.\d{4}|nan) \(\d+\.\d{3} sec\) \d\d/\d\d/\d\d \d\d:\d\d:\d\d'
                                           r', post-processed Dice Avg: (\d\.\d{4}|nan) \(\d+\.\d components / class\)', pval[0]), pval
    assert sum('post-processed Dice Avg' in l for l in post['out'].splitlines() if l.startswith('Testing Model:')) == 1
    # the same numbers from scipy on the host copy of the same prediction (test() evaluated the checkpoint now in exp.model)
    exp = post['exp']
    n_class = exp.config['n_classes']
    dice = np.zeros(n_class - 1)
    comps = np.zeros(n_class - 1)
    removed = total = n_vol = 0
    with torch.no_grad():
        exp.model.eval()
        for images, truths, _ in exp.validation_data_loader:
            _, lab = metrics.eval_dice_counts(exp.model(images.to(exp.device)), truths.to(exp.device))
            pred, truth = lab.cpu().numpy(), truths.numpy()
            for p, t in zip(pred, truth):
                roots, _ = cc.ref_roots(p, 18, n_class)
                clean, stats = cc.ref_keep_largest(p, roots, n_class)
                with np.errstate(invalid='ignore', divide='ignore'):
                    dice += np.array([2.0 * np.sum((clean == c) & (t == c)) / (np.sum(clean == c) + np.sum(t == c)) for c in range(1, n_class)])
                comps += stats[1:, 0]
                removed += int((p > 0).sum()) - int((clean > 0).sum())
                total += int((p > 0).sum())
                n_vol += 1
    want = torch.from_numpy(dice / n_vol).float()
    assert torch.equal(torch.nan_to_num(extra['post_dice_per_class'], nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert np.array_equal(extra['components_per_class'], comps / n_vol)
    assert extra['removed_frac'] == (removed / float(total) if total else 0.0)
    got_avg, want_avg = float(extra['post_dice_avg']), float(want.mean())
    assert got_avg == want_avg or (np.isnan(got_avg) and np.isnan(want_avg))


def test_sample_offsets_past_2_to_31():
    """Two samples of 1025 x 1024 x 1024 voxels: V < 2^31 per sample, but the flat offsets of the second sample's last plane lie past 2^31.
    A few planted voxels there and at the sample boundary; the expected maps are known in closed form (no host reference at this size)."""
    from deepatlas_amd import ops, _native
    td, th, tw = _tile()
    D, H, W = shape = (1025, 1024, 1024)
    V = D * H * W
    assert V < 2 ** 31 <= 2 * V and V + (D - 1) * H * W >= 2 ** 31
    if torch.cuda.mem_get_info()[0] < 48 * 2 ** 30:
        pytest.skip('needs 48 GB of free device memory (label map, two int32 maps, the int32 workspace, the cleaned map)')
    idx = lambda p: (p[0] * H + p[1]) * W + p[2]
    a, b = (D - 1, th - 1, tw - 1), (D - 1, th, tw)                  # across a tile edge: joined under 18 and 26
    c0, c1 = (D - 1, H - 1, W - 2), (D - 1, H - 1, W - 1)            # the last two voxels of the batch, one component
    try:
        lab = torch.zeros((2,) + shape, dtype=torch.uint8, device=DEV)
        lab[0, D - 1, H - 1, W - 1] = 1
        lab[1, 0, 0, 0] = 1                                          # the last voxel of sample 0 and the first of sample 1 stay apart
        lab[1][a] = 2
        lab[1][b] = 2
        lab[1][c0] = 3
        lab[1][c1] = 3
        for conn in cc.CONNECTIVITIES:
            joined = conn != 6
            roots, sizes = ops.connected_components(lab, conn, return_sizes=True)
            assert int(roots.count_nonzero()) == 6 and int(sizes.sum()) == 6
            assert int(roots[0, D - 1, H - 1, W - 1]) == V and int(roots[1, 0, 0, 0]) == 1
            assert int(roots[1][a]) == idx(a) + 1 and int(roots[1][b]) == (idx(a) if joined else idx(b)) + 1
            assert int(roots[1][c0]) == idx(c0) + 1 and int(roots[1][c1]) == idx(c0) + 1
            assert int(sizes[1][a]) == (2 if joined else 1) and int(sizes[1][b]) == (0 if joined else 1) and int(sizes[1][c0]) == 2
            del roots, sizes
            kept, stats = ops.keep_largest_component(lab, N_CLASS, conn, return_stats=True)
            assert int(kept.count_nonzero()) == (6 if joined else 5) and int(kept[1][a]) == 2 and int(kept[1][b]) == (2 if joined else 0)
            assert stats[0].tolist() == [[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0]]
            assert stats[1].tolist() == [[0, 0, 0], [1, 1, 1], [1, 2, 2] if joined else [2, 1, 2], [1, 2, 2]]
            del kept
            small = ops.remove_small_components(lab, N_CLASS, 2, conn)
            assert int(small.count_nonzero()) == (4 if joined else 2) and int(small[1][c1]) == 3 and int(small[0].count_nonzero()) == 0
            del small
    finally:
        lab = None
        _native.workspace.buf.clear()                                # the 8.6 GB scratch of this size is not kept for the rest of the session
        torch.cuda.empty_cache()
