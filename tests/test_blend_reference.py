"""CPU companion of tests/test_gpu_blend.py: the float64 reference of tests/blend_cases.py meets the guard-band condition on its own, the
restated geometry agrees with Partition's, and the host-side pieces of the inference route -- importance_window, parse_tile_blend,
restore_native, predict_seg.py's parser and config lookup.  No GPU."""
import json
import math
import os

import numpy as np
import pytest
import torch

import blend_cases as bc


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape_index,K', bc.CASES)
def test_reference_meets_the_guard_band_condition(shape_index, K):
    for window in bc.WINDOWS:
        for flip in bc.FLIPS:
            c = bc.case_data(shape_index, K, window, flip)
            assert 0.0 < c['d32'] < 1e-6                                            # a float32 evaluation: a few units of 2^-24
            keep = bc.guard(c['acc64'], c['wsum'], c['tol'])
            assert 1.0 - keep.mean() <= bc.MAX_EXCLUDED, (window, flip)
            assert np.allclose(c['acc64'].sum(1), c['wsum'], rtol=1e-12)            # probabilities sum to one under every window
            assert c['wsum'].min() > 0                                              # every voxel is covered


def test_reference_flip_is_the_reference_of_the_unmirrored_logits():
    vol, tile, overlap = bc.SHAPES[0]
    logits = bc.draw_logits(vol, tile, overlap, 5)
    win = bc.tables(tile, 'gaussian')
    for flip in bc.FLIPS:
        a, _ = bc.reference(logits, vol, tile, overlap, win, flip)
        b, _ = bc.reference(np.ascontiguousarray(bc.unmirror(logits, flip)), vol, tile, overlap, win, 0)
        assert np.array_equal(a, b)
    twice, w2 = bc.reference(logits, vol, tile, overlap, win, passes=2)
    once, w1 = bc.reference(logits, vol, tile, overlap, win)
    assert np.array_equal(twice, 2 * once) and np.array_equal(w2, 2 * w1)


@pytest.mark.parametrize('vol,tile,overlap', bc.SHAPES + [bc.BIG[:3], ((9, 11, 13), (8, 8, 8), (2, 2, 2))])
def test_restated_geometry_agrees_with_partition_and_numpy_pad(vol, tile, overlap):
    from deepatlas_amd.lib.transforms import Partition
    part = Partition(tuple(reversed(tile)), tuple(reversed(overlap)))
    part._geom(vol)
    e, g, T = bc.geometry(vol, tile, overlap)
    assert tuple(part.effective_size) == e and tuple(part.tiles_grid_size) == g
    maps = bc.tile_maps(vol, tile, overlap)
    assert len(maps) == T
    # the tiles of a volume of distinct values, by numpy.pad tiling of the VALUES, equal the values gathered through the index maps
    values = np.random.RandomState(0).permutation(int(np.prod(vol))).astype(np.float32).reshape(vol)
    padded = np.pad(values, [(o, gi * ei + o - s) for o, gi, ei, s in zip(overlap, g, e, vol)], 'reflect')
    cover = np.zeros(int(np.prod(vol)), dtype=np.int64)
    t = 0
    for i in range(g[0]):
        for j in range(g[1]):
            for k in range(g[2]):
                idx, inside = maps[t]
                want = padded[i * e[0]:i * e[0] + tile[0], j * e[1]:j * e[1] + tile[1], k * e[2]:k * e[2] + tile[2]]
                assert np.array_equal(values.reshape(-1)[idx], want)
                # inside = the positions whose coordinate i e - o + l lies in the volume
                z = i * e[0] - overlap[0] + np.arange(tile[0])
                y = j * e[1] - overlap[1] + np.arange(tile[1])
                x = k * e[2] - overlap[2] + np.arange(tile[2])
                box = ((z >= 0) & (z < vol[0]))[:, None, None] & ((y >= 0) & (y < vol[1]))[None, :, None] & ((x >= 0) & (x < vol[2]))[None, None, :]
                assert np.array_equal(inside, box)
                lin = (z[:, None, None] * vol[1] + y[None, :, None]) * vol[2] + x[None, None, :]
                assert np.array_equal(idx[inside], lin[box])
                assert len(np.unique(idx[inside])) == inside.sum()
                np.add.at(cover, idx[inside], 1)
                t += 1
    per_axis = [max(sum(1 for a in range(gi) if a * ei - o <= c < a * ei - o + ti) for c in range(s)) for gi, ei, o, ti, s in zip(g, e, overlap, tile, vol)]
    assert cover.min() >= 1 and cover.max() == per_axis[0] * per_axis[1] * per_axis[2]


def test_case_table_is_what_the_issue_names():
    _, g, T = bc.geometry(*bc.SHAPES[0])
    assert T == 45
    cover = np.zeros(int(np.prod(bc.SHAPES[0][0])), dtype=int)
    for idx, inside in bc.tile_maps(*bc.SHAPES[0]):
        np.add.at(cover, idx[inside], 1)
    assert cover.max() == 12
    assert bc.geometry(*bc.SHAPES[1])[2] == 8 and bc.geometry(*bc.SHAPES[2])[2] == 1 and bc.geometry(*bc.SHAPES[3])[2] == 64
    cover = np.zeros(16 ** 3, dtype=int)
    for idx, inside in bc.tile_maps(*bc.SHAPES[3]):
        np.add.at(cover, idx[inside], 1)
    assert cover.max() == 8
    vol, tile, overlap, K = bc.BIG
    items = bc.geometry(vol, tile, overlap)[2] * int(np.prod(tile)) * bc.lanes(K)
    assert bc.geometry(vol, tile, overlap)[2] == 9 and bc.da_grid(items) == bc.GRID_CAP and bc.GRID_CAP * bc.BLOCK < items < 2 * bc.GRID_CAP * bc.BLOCK
    assert [bc.lanes(k) for k in (2, 3, 4, 5, 12, 32, 33, 64, 255, 256)] == [2, 4, 1, 8, 16, 8, 64, 16, 64, 64]


# ---- importance_window ------------------------------------------------------------------------------------------------------------------
def test_importance_window_against_its_formula():
    from deepatlas_amd.lib.transforms import importance_window
    for tile in ((4, 5, 6), (8, 8, 8), (32, 128, 128)):
        for scale in (0.125, 0.25):
            win = importance_window(tile, 'gaussian', scale)
            assert len(win) == 3
            for w, t in zip(win, tile):
                want = np.array([math.exp(-(l - (t - 1) / 2.0) ** 2 / (2.0 * (scale * t) ** 2)) for l in range(t)]).astype(np.float32)
                assert w.dtype == np.float32 and w.shape == (t,) and np.array_equal(w, want)
                assert np.array_equal(w, w[::-1])                                   # symmetric
                assert w.max() <= 1.0 and (w.argmax() in ((t - 1) // 2, t // 2))
        assert all(np.array_equal(w, np.ones(t, dtype=np.float32)) for w, t in zip(importance_window(tile, 'constant'), tile))
    # the float32 products stay normal numbers at t = 128
    wz, wy, wx = importance_window((128, 128, 128))
    corner = np.float32(np.float32(wz[0] * wy[0]) * wx[0])
    assert corner >= np.finfo(np.float32).tiny and corner == ((wz[:, None, None] * wy[None, :, None]) * wx[None, None, :]).min()
    for bad in (dict(kind='hann'), dict(sigma_scale=0.0), dict(sigma_scale=float('nan'))):
        with pytest.raises(ValueError):
            importance_window((8, 8, 8), **bad)
    with pytest.raises(ValueError):
        importance_window((8, 8))
    with pytest.raises(ValueError):
        importance_window((8, 0, 8))


# ---- parse_tile_blend -------------------------------------------------------------------------------------------------------------------
def test_parse_tile_blend_forms():
    from deepatlas_amd.lib.inference import parse_tile_blend, refuse_tile_blend
    patch = {'size': [8, 8, 8]}
    assert parse_tile_blend(None) is None and parse_tile_blend(None, patch) is None
    full = {'window': 'gaussian', 'sigma_scale': 0.125, 'mirror': []}
    assert parse_tile_blend('gaussian', patch) == full
    assert parse_tile_blend('constant', patch) == dict(full, window='constant')
    assert parse_tile_blend({}, patch) == full
    assert parse_tile_blend({'window': 'constant', 'sigma_scale': 0.25, 'mirror': ['x', 'z']}, patch) == {'window': 'constant', 'sigma_scale': 0.25, 'mirror': ['z', 'x']}
    assert parse_tile_blend({'mirror': 'zyx'}, patch)['mirror'] == ['z', 'y', 'x']
    for bad in ('hann', 3, ['gaussian'], {'window': 'hann'}, {'windows': 'gaussian'}, {'sigma_scale': 0}, {'sigma_scale': True}, {'sigma_scale': 'wide'},
                {'mirror': ['w']}, {'mirror': ['x', 'x']}, {'mirror': 'xq'}):
        with pytest.raises(ValueError):
            parse_tile_blend(bad, patch)
    with pytest.raises(ValueError, match=r"needs config\['patch'\]"):
        parse_tile_blend('gaussian')
    refuse_tile_blend({}, 'registration')
    refuse_tile_blend({'tile_blend': None}, 'joint')
    with pytest.raises(ValueError, match='tile_blend'):
        refuse_tile_blend({'tile_blend': 'gaussian'}, 'registration')


def test_tile_blend_key_in_the_experiment_config(tmp_path):
    from deepatlas_amd.models.segmentation import PATCH_DEFAULTS, SegmentationExperiment, parse_patch
    flags = ['--shape', '16', '16', '16', '--patch-size', '8', '8', '8', '--tile-overlap', '2', '2', '2']
    plain = bc.seg_config(tmp_path / 'a', flags)
    blend = bc.seg_config(tmp_path / 'b', flags + ['--tile-blend', 'constant'])
    mirror = bc.seg_config(tmp_path / 'c', flags + ['--tile-mirror', 'xz'])
    assert 'tile_blend' not in plain and 'tile_mirror' not in plain and 'tile_mirror' not in blend
    assert blend['tile_blend'] == {'window': 'constant', 'sigma_scale': 0.125, 'mirror': []}
    assert mirror['tile_blend'] == {'window': 'gaussian', 'sigma_scale': 0.125, 'mirror': ['x', 'z']}
    assert plain['patch'] == blend['patch'] and 'tile_blend' not in PATCH_DEFAULTS      # a top-level key, never one of config['patch']
    with pytest.raises(ValueError):
        parse_patch({'size': [8, 8, 8], 'tile_blend': 'gaussian'})
    names = [SegmentationExperiment.experiment_name(c) for c in (plain, blend, mirror)]
    assert names[0] == names[1] == names[2]                                            # the key takes no part in the name
    a, b = SegmentationExperiment(plain), SegmentationExperiment(mirror)
    assert a.tile_blend is None and b.tile_blend == {'window': 'gaussian', 'sigma_scale': 0.125, 'mirror': ['z', 'x']} and a.exp_name == b.exp_name
    whole = bc.seg_config(tmp_path / 'd', ['--shape', '16', '16', '16'])
    with pytest.raises(ValueError, match=r"needs config\['patch'\]"):
        SegmentationExperiment(dict(whole, tile_blend='gaussian'))
    with pytest.raises(ValueError, match='need --patch-size'):
        bc.seg_config(tmp_path / 'e', ['--shape', '16', '16', '16', '--tile-blend', 'gaussian'])


# ---- restore_native ---------------------------------------------------------------------------------------------------------------------
def numpy_resample(vol, out_size, scale, offset, interpolator='nearest', default=0):
    """ops.resample_volume restated with numpy from ops.resample_axis_table (nearest: a gather; linear: the three axes one after another)."""
    from deepatlas_amd import ops
    a = np.asarray(vol)
    tabs = [ops.resample_axis_table(n, m, s, o, interpolator) for n, m, s, o in zip(a.shape, out_size, scale, offset)]
    inside = tabs[0][3][:, None, None] & tabs[1][3][None, :, None] & tabs[2][3][None, None, :]
    if interpolator == 'nearest':
        out = a[tabs[0][0][:, None, None], tabs[1][0][None, :, None], tabs[2][0][None, None, :]]
        return torch.from_numpy(np.where(inside, out, np.asarray(default, dtype=a.dtype)))
    out = a.astype(np.float64)
    for axis, (lo, hi, frac, _) in enumerate(tabs):
        f = frac.astype(np.float64).reshape([-1 if k == axis else 1 for k in range(3)])
        out = np.take(out, lo, axis) * (1.0 - f) + np.take(out, hi, axis) * f
    return torch.from_numpy(np.where(inside, out, float(default)).astype(np.float32))


def test_restore_native_against_the_numpy_restatement():
    from deepatlas_amd.lib.inference import restore_native
    from deepatlas_amd.lib.transforms import Resample
    rng = np.random.RandomState(1)
    native = (10, 16, 12)
    lab = torch.from_numpy(rng.randint(0, 32, size=native).astype(np.uint8))
    # no geometric step, and a resample at equal spacing: the identity, bit for bit
    assert torch.equal(restore_native(lab, {'native_size': native, 'native_spacing': (1.0, 1.0, 1.0), 'steps': []}, resample=numpy_resample), lab)
    same = {'native_size': native, 'native_spacing': (0.7, 0.7, 0.7), 'steps': [('resample', native, (0.7, 0.7, 0.7), (0.7, 0.7, 0.7))]}
    assert torch.equal(restore_native(lab, same, resample=numpy_resample), lab)
    # flip, then unflip
    flipped = numpy_resample(lab, native, (-1.0, 1.0, 1.0), (float(native[0] - 1), 0.0, 0.0))
    assert torch.equal(flipped, torch.flip(lab, [0]))
    assert torch.equal(restore_native(flipped, {'native_size': native, 'native_spacing': (1.0, 1.0, 1.0), 'steps': [('flip',)]}, resample=numpy_resample), lab)
    # 0.7 mm -> 1.0 mm -> 0.7 mm returns the native size, and every native voxel reads the prepared voxel nearest to it
    sp, vox = (0.7, 0.7, 0.7), (1.0, 1.0, 1.0)
    nx, ny, nz = Resample.new_size(tuple(reversed(native)), sp, vox)
    prepared = numpy_resample(lab, (nz, ny, nx), tuple(vox[k] / sp[k] for k in (2, 1, 0)), (0.0, 0.0, 0.0))
    assert tuple(prepared.shape) == (7, 12, 9)
    record = {'native_size': native, 'native_spacing': sp, 'steps': [('resample', native, sp, vox), ('flip',)]}
    seen = torch.flip(prepared, [0])                                                # what the net saw: resampled, then flipped
    back = restore_native(seen, record, resample=numpy_resample)
    assert tuple(back.shape) == native and back.dtype == torch.uint8
    zi, yi, xi = (np.clip(np.floor(np.arange(n) * 0.7 + 0.5), 0, m - 1).astype(int) for n, m in zip(native, prepared.shape))
    assert np.array_equal(back.numpy(), prepared.numpy()[zi[:, None, None], yi[None, :, None], xi[None, None, :]])
    conf = restore_native(torch.from_numpy(rng.random_sample((7, 12, 9)).astype(np.float32)), record, 'linear', resample=numpy_resample)
    assert tuple(conf.shape) == native and conf.dtype == torch.float32 and float(conf.min()) >= 0.0 and float(conf.max()) <= 1.0
    # a cropped border comes back as zeros
    crop = {'native_size': native, 'native_spacing': vox, 'steps': [('crop', native, (1, 2, 3, 1, 2, 3))]}
    full = restore_native(lab[1:9, 2:14, 3:9], crop, resample=numpy_resample)
    assert torch.equal(full[1:9, 2:14, 3:9], lab[1:9, 2:14, 3:9]) and int(full.sum()) == int(lab[1:9, 2:14, 3:9].sum())
    with pytest.raises(ValueError, match='came back'):
        restore_native(lab, {'native_size': (1, 2, 3), 'native_spacing': vox, 'steps': []}, resample=numpy_resample)
    with pytest.raises(ValueError, match='unknown record step'):
        restore_native(lab, {'native_size': native, 'native_spacing': vox, 'steps': [('shear',)]}, resample=numpy_resample)


# ---- predict_seg.py ---------------------------------------------------------------------------------------------------------------------
def test_predict_seg_parser_and_config_lookup(tmp_path):
    import predict_seg
    p = predict_seg.build_parser()
    a = p.parse_args(['--ckpt', 'c.pth.tar', '--output-dir', 'out', '--input', 'a.nii.gz', 'b.nii'])
    assert a.input == ['a.nii.gz', 'b.nii'] and a.config is None and a.patch_size is None and a.tile_blend is None and not a.save_confidence
    a = p.parse_args(['--ckpt', 'c', '--output-dir', 'o', '--data-dir', 'd', '--list', 'l.txt', '--patch-size', '32', '128', '128', '--tile-overlap', '8', '32', '32',
                      '--tile-batch', '2', '--tile-blend', 'gaussian', '--tile-mirror', 'zyx', '--postprocess', 'min-size', '--cc-connectivity', '26',
                      '--cc-min-size', '10', '--save-confidence', '--label-dir', 'd', '--surface-metrics', '--config', 'x.json'])
    assert (a.patch_size, a.tile_overlap, a.tile_batch, a.tile_blend, a.tile_mirror) == ([32, 128, 128], [8, 32, 32], 2, 'gaussian', 'zyx')
    assert a.list_file == 'l.txt' and a.save_confidence and a.surface_metrics and a.config == 'x.json'
    assert predict_seg.postprocess_setting(a) == {'mode': 'min_size', 'connectivity': 26, 'min_size': 10}
    for bad in ([], ['--ckpt', 'c'], ['--ckpt', 'c', '--output-dir', 'o', '--tile-blend', 'hann']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    # the config beside the checkpoint
    run = tmp_path / 'run' / '230'
    os.makedirs(str(run))
    ckpt = str(run / 'model_best.pth.tar')
    with pytest.raises(ValueError, match='pass --config'):
        predict_seg.find_config(ckpt)
    with open(str(run / 'train_config.json'), 'w') as f:
        json.dump({'model': 'UNet_light', 'n_classes': 32, 'patch': {'size': [8, 8, 8], 'overlap': [2, 2, 2]}, 'tile_blend': 'gaussian'}, f)
    assert predict_seg.find_config(ckpt) == str(run / 'train_config.json')
    other = str(tmp_path / 'other.json')
    with open(other, 'w') as f:
        json.dump({}, f)
    assert predict_seg.find_config(ckpt, other) == other
    with open(predict_seg.find_config(ckpt)) as f:
        cfg = json.load(f)
    # settings: the config's, overridden by the flags; with tile_blend off a constant window
    base = ['--ckpt', ckpt, '--output-dir', 'o', '--input', 'kneeLEFT0_image.nii.gz']
    patch, blend = predict_seg.inference_settings(p.parse_args(base), cfg)
    assert patch['size'] == [8, 8, 8] and patch['overlap'] == [2, 2, 2] and blend == {'window': 'gaussian', 'sigma_scale': 0.125, 'mirror': []}
    patch, blend = predict_seg.inference_settings(p.parse_args(base + ['--tile-overlap', '1', '1', '1', '--tile-mirror', 'x', '--tile-batch', '7']), dict(cfg, tile_blend=None))
    assert patch['overlap'] == [1, 1, 1] and patch['tile_batch'] == 7 and blend == {'window': 'constant', 'sigma_scale': 0.125, 'mirror': ['x']}
    assert predict_seg.inference_settings(p.parse_args(base), {'model': 'UNet_light'}) == (None, None)
    patch, blend = predict_seg.inference_settings(p.parse_args(base + ['--patch-size', '16', '16', '16', '--tile-overlap', '4', '4', '4']), {'model': 'UNet_light'})
    assert patch['size'] == [16, 16, 16] and blend['window'] == 'constant'
    with pytest.raises(ValueError, match='need a patch size'):
        predict_seg.inference_settings(p.parse_args(base + ['--tile-blend', 'gaussian']), {'model': 'UNet_light'})
    # inputs
    scans = predict_seg.resolve_inputs(p.parse_args(base + ['--labels', 'm.nii.gz']), cfg)
    assert scans == [('kneeLEFT0', 'kneeLEFT0_image.nii.gz', 'm.nii.gz')] and predict_seg.scan_name('/x/y/scan7.nii') == 'scan7'
    listing = str(tmp_path / 'l.txt')
    with open(listing, 'w') as f:
        f.write('s0\ns1\n')
    scans = predict_seg.resolve_inputs(p.parse_args(['--ckpt', ckpt, '--output-dir', 'o', '--data-dir', 'D', '--list', listing, '--label-dir', 'L']), dict(cfg, data='OASIS'))
    assert scans == [('s0', os.path.join('D', '', 's0_image.nii.gz'), os.path.join('L', '', 's0_seg.nii.gz')),
                     ('s1', os.path.join('D', '', 's1_image.nii.gz'), os.path.join('L', '', 's1_seg.nii.gz'))]
    for bad in (['--ckpt', ckpt, '--output-dir', 'o'], base + ['--data-dir', 'D', '--list', listing], base + ['--labels', 'a', 'b'],
                ['--ckpt', ckpt, '--output-dir', 'o', '--list', listing]):
        with pytest.raises(ValueError):
            predict_seg.resolve_inputs(p.parse_args(bad), cfg)
    assert predict_seg.format_dice('s0', 0.5) == 's0: Dice Avg: 0.500000'
