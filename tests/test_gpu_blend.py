"""blend.hip on the device (da_blend_accumulate, da_blend_finalize), lib/inference.py's SlidingWindowPredictor, the segmentation experiment's
config['tile_blend'] and predict_seg.py end to end.  Cases, the float64 reference, the tolerance and the guard band: tests/blend_cases.py."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import blend_cases as bc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0) if torch.cuda.is_available() else None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_logits(logits):
    """[T][tz][ty][tx][K] numpy -> the T x K x tz x ty x tx view of the same channels-last memory on the device."""
    return torch.from_numpy(np.array(logits, dtype=np.float32, order='C')).to(DEV).permute(0, 4, 1, 2, 3)


def accumulate(logits, vol, tile, overlap, win, flip=0, calls=None, acc=None):
    from deepatlas_amd import ops
    L = device_logits(logits)
    if acc is None:
        acc = torch.zeros(tuple(vol) + (logits.shape[-1],), dtype=torch.float32, device=DEV)
    for t0, n in (calls or [(0, L.shape[0])]):
        ops.blend_accumulate(acc, L[t0:t0 + n], t0, tile, overlap, win, flip)
    return acc


def host(acc):
    return acc.reshape(-1, acc.shape[-1]).cpu().numpy()


# ---- 1. the accumulator against float64, 2. labels and confidence outside the guard band ------------------------------------------------
@pytest.mark.parametrize('shape_index,K', bc.CASES)
def test_accumulator_labels_and_confidence_against_float64(shape_index, K):
    from deepatlas_amd import ops
    worst = (0.0, 0.0, 0.0)
    for window in bc.WINDOWS:
        for flip in bc.FLIPS:
            c = bc.case_data(shape_index, K, window, flip)
            acc = accumulate(c['logits'], c['vol'], c['tile'], c['overlap'], c['win'], flip)
            d = bc.distance(host(acc), c['acc64'], c['wsum'])
            if d / c['d32'] > worst[0]:
                worst = (d / c['d32'], d, c['d32'])
            print('blend case %d K %d %s flip %d: kernel distance %.3e, float32 torch distance %.3e, tolerance %.3e' % (shape_index, K, window, flip, d, c['d32'], c['tol']))
            assert d <= c['tol'], (window, flip, d, c['d32'])
            labels, conf = ops.blend_finalize(acc, return_conf=True)
            ref_lab, ref_conf, _ = bc.labels_conf(c['acc64'])
            keep = bc.guard(c['acc64'], c['wsum'], c['tol'])
            assert 1.0 - keep.mean() <= bc.MAX_EXCLUDED
            assert labels.dtype == torch.uint8 and tuple(labels.shape) == tuple(c['vol'])
            assert np.array_equal(labels.cpu().numpy().reshape(-1)[keep], ref_lab[keep])
            dc = float(np.abs(conf.cpu().numpy().reshape(-1).astype(np.float64)[keep] - ref_conf[keep]).max())
            print('    confidence distance %.3e' % dc)
            assert dc <= c['tol'], (window, flip, dc)
            assert torch.equal(ops.blend_finalize(acc), labels)
    print('blend case %d K %d: worst kernel / float32 torch ratio %.3f (kernel %.3e, torch %.3e)' % ((shape_index, K) + worst))


def test_one_call_beyond_the_capped_grid():
    """9 tiles of 16 x 32 x 32 at K = 32: more work items than da_grid's 4096 x 256, so the grid-stride loop runs a second trip."""
    vol, tile, overlap, K = bc.BIG
    _, _, T = bc.geometry(vol, tile, overlap)
    items = T * int(np.prod(tile)) * bc.lanes(K)
    assert T == 9 and bc.da_grid(items) * bc.BLOCK < items
    logits = bc.draw_logits(vol, tile, overlap, K)
    win = bc.tables(tile, 'gaussian')
    acc64, wsum = bc.reference(logits, vol, tile, overlap, win)
    tol = bc.FACTOR * bc.distance(bc.evaluate_f32(logits, vol, tile, overlap, win), acc64, wsum)
    acc = accumulate(logits, vol, tile, overlap, win)
    d = bc.distance(host(acc), acc64, wsum)
    print('blend big case: kernel distance %.3e, tolerance %.3e' % (d, tol))
    assert d <= tol
    assert torch.equal(acc, accumulate(logits, vol, tile, overlap, win, calls=bc.chunkings(T)['chunks of 4']))


# ---- 3. exact properties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape_index,K', bc.CASES)
def test_accumulator_is_bit_identical_across_chunkings_runs_and_mirrored_inputs(shape_index, K):
    vol, tile, overlap = bc.SHAPES[shape_index]
    _, _, T = bc.geometry(vol, tile, overlap)
    logits = bc.draw_logits(vol, tile, overlap, K)
    for window in bc.WINDOWS:
        win = bc.tables(tile, window)
        first = accumulate(logits, vol, tile, overlap, win)
        for name, calls in bc.chunkings(T).items():
            assert torch.equal(accumulate(logits, vol, tile, overlap, win, calls=calls), first), name
        assert torch.equal(accumulate(logits, vol, tile, overlap, win), first)
        for flip in bc.FLIPS[1:]:
            mirrored = np.ascontiguousarray(bc.unmirror(logits, flip))            # torch.flip(L, axes)
            for calls in bc.chunkings(T).values():
                assert torch.equal(accumulate(mirrored, vol, tile, overlap, win, flip, calls=calls), first), flip
    # a second pass adds onto the stored sums
    twice = accumulate(logits, vol, tile, overlap, win, acc=accumulate(logits, vol, tile, overlap, win))
    again = accumulate(logits, vol, tile, overlap, win, acc=accumulate(logits, vol, tile, overlap, win), calls=bc.chunkings(T)['one per call'])
    assert torch.equal(twice, again) and not torch.equal(twice, first)


@pytest.mark.parametrize('shape_index', range(len(bc.SHAPES)))
@pytest.mark.parametrize('K', [2, 32, 256])
def test_constant_logits_give_the_running_weight_sums(shape_index, K):
    """exp(0) = 1, the sum K and 1 / K are exact for a power of two: acc = the float32 running sum of the covering tiles' weights / K, bit for bit."""
    vol, tile, overlap = bc.SHAPES[shape_index]
    _, _, T = bc.geometry(vol, tile, overlap)
    logits = np.full((T,) + tuple(tile) + (K,), 0.75, dtype=np.float32)
    for window in bc.WINDOWS:
        win = bc.tables(tile, window)
        want = bc.running_weight_sums(vol, tile, overlap, win) / np.float32(K)
        for flip in (0, 5):
            got = host(accumulate(logits, vol, tile, overlap, win, flip, calls=bc.chunkings(T)['chunks of 4']))
            assert np.array_equal(got, np.repeat(want[:, None], K, 1)), (window, flip)


@pytest.mark.parametrize('K', bc.KS + (256,))
def test_lattice_logits_without_overlap_equal_the_assembled_tile_argmax(K):
    from deepatlas_amd import ops
    from deepatlas_amd.lib.transforms import Partition
    vol, tile, overlap = bc.SHAPES[1]
    logits = bc.lattice_logits(vol, tile, overlap, K)
    acc = accumulate(logits, vol, tile, overlap, bc.tables(tile, 'constant'), calls=bc.chunkings(logits.shape[0])['chunks of 4'])
    L = device_logits(logits)
    per_tile = ops.argmax_dice_counts(L, torch.zeros((L.shape[0],) + tuple(tile), dtype=torch.uint8, device=DEV))[1]
    part = Partition(tuple(reversed(tile)), tuple(reversed(overlap)))
    part._geom(vol)
    want = part.assemble(per_tile)
    assert torch.equal(ops.blend_finalize(acc), want) and int(want.max()) == K - 1


@pytest.mark.parametrize('K', bc.KS + (256,))
def test_single_tile_equals_the_whole_volume_argmax(K):
    from deepatlas_amd import ops
    vol, tile, overlap = bc.SHAPES[2]
    logits = bc.lattice_logits(vol, tile, overlap, K)
    for window in bc.WINDOWS:
        labels = ops.blend_finalize(accumulate(logits, vol, tile, overlap, bc.tables(tile, window)))
        want = logits[0, 1:7, 1:7, 1:7].argmax(-1).astype(np.uint8)
        assert np.array_equal(labels.cpu().numpy(), want)


@pytest.mark.parametrize('K', [5, 32])
def test_nan_logit_marks_exactly_its_tile(K):
    from deepatlas_amd import ops
    vol, tile, overlap = bc.SHAPES[0]
    logits = bc.draw_logits(vol, tile, overlap, K)
    win = bc.tables(tile, 'gaussian')
    clean = accumulate(logits, vol, tile, overlap, win)
    t = 22                                                                         # an interior tile of the 3 x 3 x 5 grid
    idx, inside = bc.tile_maps(vol, tile, overlap)[t]
    bad = logits.copy()
    bad[t, :, :, :, 1] = np.nan                                                    # one class of every voxel of the tile
    acc = accumulate(bad, vol, tile, overlap, win, calls=bc.chunkings(logits.shape[0])['chunks of 4'])
    labels, conf = ops.blend_finalize(acc, return_conf=True)
    hit = np.zeros(int(np.prod(vol)), dtype=bool)
    hit[idx[inside]] = True
    assert 0 < hit.sum() < hit.size
    assert np.array_equal(np.isnan(conf.cpu().numpy().reshape(-1)), hit)
    a, b = host(acc), host(clean)
    assert np.array_equal(a[~hit], b[~hit])
    clean_labels, clean_conf = ops.blend_finalize(clean, return_conf=True)
    assert np.array_equal(labels.cpu().numpy().reshape(-1)[~hit], clean_labels.cpu().numpy().reshape(-1)[~hit])
    assert np.array_equal(conf.cpu().numpy().reshape(-1)[~hit], clean_conf.cpu().numpy().reshape(-1)[~hit])


def test_bad_arguments():
    from deepatlas_amd import _native as nat
    from deepatlas_amd import ops
    vol, tile, overlap = bc.SHAPES[3]
    K = 5
    _, _, T = bc.geometry(vol, tile, overlap)
    L = torch.zeros((T,) + tuple(tile) + (K,), dtype=torch.float32, device=DEV)
    acc = torch.zeros(tuple(vol) + (K,), dtype=torch.float32, device=DEV)
    w = [torch.ones(t, dtype=torch.float32, device=DEV) for t in tile]
    lib = nat.lib()

    def int3(v):
        return ctypes.cast((ctypes.c_int * 3)(*v), ctypes.c_void_p)

    def rc(logits=L, a=acc, dims=vol, k=K, t3=tile, o3=overlap, tile0=0, n=T, ws=w, flip=0):
        return lib.da_blend_accumulate(nat.ptr(logits), nat.ptr(a), dims[0], dims[1], dims[2], k, int3(t3) if t3 else None, int3(o3) if o3 else None,
                                       tile0, n, nat.ptr(ws[0]), nat.ptr(ws[1]), nat.ptr(ws[2]), flip, nat.stream())
    assert rc() == 0
    acc.zero_()
    bad = [rc(logits=None), rc(a=None), rc(t3=None), rc(o3=None), rc(ws=[None, w[1], w[2]]), rc(ws=[w[0], None, w[2]]), rc(ws=[w[0], w[1], None]),
           rc(dims=(0, 16, 16)), rc(o3=(4, 2, 2)), rc(o3=(-1, 2, 2)), rc(t3=(0, 8, 8)),           # what tile_geom refuses
           rc(tile0=-1), rc(n=0), rc(tile0=1, n=T), rc(tile0=T, n=1), rc(k=1), rc(k=257), rc(flip=8), rc(flip=-1)]
    assert bad == [-1] * len(bad)
    lab = torch.zeros(vol, dtype=torch.uint8, device=DEV)
    V = int(np.prod(vol))
    fin = lambda a=acc, v=V, k=K, l=lab: lib.da_blend_finalize(nat.ptr(a), v, k, nat.ptr(l), None, nat.stream())
    assert fin() == 0
    assert [fin(a=None), fin(l=None), fin(v=0), fin(k=1), fin(k=257)] == [-1] * 5
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0                                           # a refused call writes nothing
    with pytest.raises(nat.NativeError, match='DA_ERR_BADARG'):
        ops.blend_accumulate(acc, L.permute(0, 4, 1, 2, 3)[:2], T - 1, tile, overlap, [x.cpu().numpy() for x in w])
    with pytest.raises(ValueError):
        ops.blend_accumulate(acc, L.permute(0, 4, 1, 2, 3), 0, (8, 8, 4), overlap, [x.cpu().numpy() for x in w])
    with pytest.raises(ValueError):
        ops.blend_finalize(acc[..., :1].contiguous())


# ---- 4. the predictor -------------------------------------------------------------------------------------------------------------------
class Pointwise(torch.nn.Module):
    """Stand-in net: K fixed affine maps of the voxel's own intensity, so that tiles agree wherever they overlap."""
    SLOPE = (0.0, 3.0, -2.0, 5.0, 1.5)
    OFFSET = (0.6, -0.9, 1.4, -2.1, 0.1)

    def forward(self, x):
        return torch.cat([x * a + b for a, b in zip(self.SLOPE, self.OFFSET)], 1)


@pytest.mark.parametrize('window', bc.WINDOWS)
@pytest.mark.parametrize('mirror', [(), ('z', 'x'), ('z', 'y', 'x')])
def test_predictor_with_a_pointwise_net_gives_the_whole_volume_labels(window, mirror):
    from deepatlas_amd.lib import evalMetrics as metrics
    from deepatlas_amd.lib.inference import SlidingWindowPredictor
    vol, tile, overlap = (9, 11, 13), (8, 8, 8), (2, 2, 2)
    model = Pointwise().to(DEV)
    image = torch.rand(vol, generator=torch.Generator().manual_seed(3)).to(DEV)
    whole_logits = model(image[None, None])
    whole = metrics.eval_dice_counts(whole_logits, torch.zeros((1,) + vol, dtype=torch.uint8, device=DEV))[1][0]
    predictor = SlidingWindowPredictor(model, 5, tile, overlap, tile_batch=5, window=window, mirror=mirror)
    assert predictor.masks == sorted(predictor.masks) and len(predictor.masks) == 2 ** len(mirror) and predictor.masks[0] == 0
    labels, conf, acc = predictor.predict(image, return_conf=True, return_acc=True)
    # the float64 reference of the same tiles: the whole-volume logits, gathered as Partition gathers the image
    values = whole_logits[0].permute(1, 2, 3, 0).reshape(-1, 5).cpu().numpy()
    logits = bc.tiles_of_volume(values, vol, tile, overlap)
    win = bc.tables(tile, window)
    passes = len(predictor.masks)
    acc64, wsum = bc.reference(logits, vol, tile, overlap, win, passes=passes)
    tol = bc.FACTOR * bc.distance(bc.evaluate_f32(logits, vol, tile, overlap, win, passes=passes), acc64, wsum)
    d = bc.distance(host(acc), acc64, wsum)
    print('predictor %s mirror %s: distance %.3e, tolerance %.3e' % (window, ''.join(mirror), d, tol))
    assert d <= tol
    keep = bc.guard(acc64, wsum, tol)
    assert 1.0 - keep.mean() <= bc.MAX_EXCLUDED
    assert np.array_equal(labels.cpu().numpy().reshape(-1)[keep], whole.cpu().numpy().reshape(-1)[keep])
    assert np.array_equal(labels.cpu().numpy().reshape(-1)[keep], bc.labels_conf(acc64)[0][keep])
    assert torch.equal(predictor.predict_batch(image[None, None].repeat(2, 1, 1, 1, 1)), torch.stack([labels, labels], 0))


def unet_experiment(tmp_path, overlap, extra=()):
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    o = str(overlap)
    exp = SegmentationExperiment(bc.seg_config(tmp_path, ['--shape', '16', '16', '16', '--patch-size', '8', '8', '8', '--tile-overlap', o, o, o,
                                                           '--tile-batch', '5'] + list(extra)))
    exp.setup_model()
    torch.manual_seed(5)
    exp.model.weights_init()
    exp.model.eval()
    return exp


def test_predictor_with_a_unet_does_not_depend_on_the_tile_batch(tmp_path):
    from deepatlas_amd.lib.inference import SlidingWindowPredictor
    exp = unet_experiment(tmp_path, 2)
    image = torch.rand((16, 16, 16), generator=torch.Generator().manual_seed(4)).to(DEV)
    accs = []
    for tb in (1, 5, 64):
        p = SlidingWindowPredictor(exp.model, 32, (8, 8, 8), (2, 2, 2), tile_batch=tb, window='gaussian', mirror=('y',))
        accs.append(p.predict(image, return_acc=True))
    assert torch.equal(accs[0][1], accs[1][1]) and torch.equal(accs[0][1], accs[2][1])
    assert torch.equal(accs[0][0], accs[1][0]) and torch.equal(accs[0][0], accs[2][0])
    assert not exp.model.training and float(accs[0][1].sum()) > 0


def test_predictor_without_overlap_equals_the_core_copy(tmp_path):
    from deepatlas_amd.lib.inference import SlidingWindowPredictor
    exp = unet_experiment(tmp_path, 0)
    images = torch.rand((1, 1, 16, 16, 16), generator=torch.Generator().manual_seed(6)).to(DEV)
    with torch.no_grad():
        core = exp.predict_tiled(images)                                           # tile_blend off: argmax per tile, assemble's core copy
    blended = SlidingWindowPredictor(exp.model, 32, (8, 8, 8), (0, 0, 0), tile_batch=3, window='constant').predict_batch(images)
    assert torch.equal(core, blended)                                              # exactly one tile covers every voxel


# ---- 5. the experiment ------------------------------------------------------------------------------------------------------------------
def _validation_line(text):
    lines = [l for l in text.splitlines() if l.startswith('Validation: Dice Avg')]
    assert len(lines) == 1
    return re.sub(r'\(\d+\.\d+ sec\) \S+ \S+', '', lines[0])


def test_experiment_with_tile_blend_and_without(tmp_path, capsys):
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    flags = ['--shape', '16', '16', '16', '--patch-size', '8', '8', '8', '--tile-overlap', '2', '2', '2']
    cfg = bc.seg_config(tmp_path / 'blend', flags + ['--tile-blend', 'gaussian', '--tile-mirror', 'zx'])
    assert cfg['tile_blend'] == {'window': 'gaussian', 'sigma_scale': 0.125, 'mirror': ['z', 'x']}
    exp = SegmentationExperiment(cfg)
    exp.train()                                                                    # one epoch and its blended, mirrored validation
    dice_per_class, dice_avg = exp.test()
    out = capsys.readouterr().out
    assert math.isfinite(float(dice_avg)) and 'Validation: Dice Avg' in out and exp.predictor is not None and exp.predictor.masks == [0, 1, 4, 5]
    # without the key: the config, the name, the route, the validation line and the Dice are the tile_blend-less run's
    plain_cfg = bc.seg_config(tmp_path / 'plain', flags)
    assert 'tile_blend' not in plain_cfg
    plain = SegmentationExperiment(plain_cfg)
    off = SegmentationExperiment(dict(bc.seg_config(tmp_path / 'off', flags), tile_blend=None))
    assert plain.exp_name == off.exp_name == exp.exp_name
    for e in (plain, off):
        e.setup_train()
        e.model.load_state_dict(exp.model.state_dict())
        e.best_score, e.current_epoch = 0, 1
    a, a_avg, _ = plain.eval(plain.validation_data_loader)
    b, b_avg, _ = off.eval(plain.validation_data_loader)
    assert torch.equal(a, b) and float(a_avg) == float(b_avg) and plain.predictor is None and off.predictor is None
    capsys.readouterr()
    plain.validate()
    first = _validation_line(capsys.readouterr().out)
    off.validate()
    assert _validation_line(capsys.readouterr().out) == first
    from deepatlas_amd.models.registration import RegistrationExperiment
    with pytest.raises(ValueError, match='tile_blend'):
        RegistrationExperiment({'tile_blend': 'gaussian', 'device': 'cuda', 'debug_mode': False})
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    with pytest.raises(ValueError, match='tile_blend'):
        DeepAtlasExperiment({'tile_blend': 'gaussian', 'device': 'cuda', 'debug_mode': False})


# ---- 6. predict_seg.py end to end -------------------------------------------------------------------------------------------------------
SCANS = ['kneeLEFT0', 'kneeLEFT1']
NATIVE = (10, 16, 12)                                 # (z, y, x)
SPACING = (1.5, 0.75, 1.25)                           # (x, y, z): prepared at 1 mm as 13 x 12 x 18


def write_scans(root):
    from deepatlas_amd.lib.datasets import structured_labels
    from deepatlas_amd.lib.nifti import write_nifti
    os.makedirs(str(root), exist_ok=True)
    for k, name in enumerate(SCANS):
        lab = structured_labels(NATIVE, 32, seed=k).numpy()
        img = (lab.astype(np.float64) * 90 + np.random.RandomState(k).uniform(0, 300, size=NATIVE)).astype(np.int16)
        write_nifti(os.path.join(str(root), name + '_image.nii.gz'), img, spacing=SPACING)
        write_nifti(os.path.join(str(root), name + '_masks.nii.gz'), lab, spacing=SPACING)
    path = os.path.join(str(root), 'scans.txt')
    with open(path, 'w') as f:
        f.write(''.join(n + '\n' for n in SCANS))
    return path


def test_predict_seg_end_to_end(tmp_path):
    import predict_seg
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics as metrics
    from deepatlas_amd.lib.inference import restore_native
    from deepatlas_amd.lib.nifti import read_nifti
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    root = tmp_path / 'scans'
    listing = write_scans(root)
    cfg = bc.seg_config(tmp_path, ['--data', 'OAI', '--data-dir', str(root), '--train-list', listing, '--valid-list', listing, '--voxel-size', '1', '1', '1',
                                   '--rescale-percentiles', '0.5', '99.5', '--preload', '--patch-size', '8', '8', '8', '--tile-overlap', '2', '2', '2'])
    cfg['preprocess'].append(['left_to_right', {}])
    exp = SegmentationExperiment(cfg)
    exp.train()
    ckpt = os.path.join(exp.ckpoint_dir, 'checkpoint.pth.tar')
    assert os.path.isfile(ckpt) and os.path.isfile(os.path.join(exp.ckpoint_dir, 'train_config.json'))
    out_dir = tmp_path / 'out'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'predict_seg.py'), '--ckpt', ckpt, '--output-dir', str(out_dir), '--data-dir', str(root),
                          '--list', listing, '--label-dir', str(root), '--tile-blend', 'gaussian', '--tile-mirror', 'y', '--save-confidence'],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=240)
    assert run.returncode == 0, run.stdout
    # the same prediction in this process
    with open(predict_seg.find_config(ckpt)) as f:
        saved = json.load(f)
    args = predict_seg.build_parser().parse_args(['--ckpt', ckpt, '--output-dir', str(out_dir), '--data-dir', str(root), '--list', listing,
                                                  '--tile-blend', 'gaussian', '--tile-mirror', 'y'])
    patch, blend = predict_seg.inference_settings(args, saved)
    assert blend == {'window': 'gaussian', 'sigma_scale': 0.125, 'mirror': ['y']} and patch['size'] == [8, 8, 8]
    model = predict_seg.load_model(saved, ckpt, DEV)
    dices = []
    for name in SCANS:
        src = read_nifti(os.path.join(str(root), name + '_image.nii.gz'))
        got = read_nifti(os.path.join(str(out_dir), name + '_seg.nii.gz'))
        assert got.array.shape == NATIVE and got.array.dtype == np.uint8 and got.spacing == src.spacing and np.array_equal(got.affine, src.affine)
        vol, image, record = predict_seg.prepare(os.path.join(str(root), name + '_image.nii.gz'), name, saved)
        assert tuple(image.shape) == (1, 13, 12, 18) and record['steps'][0][0] == 'resample' and record['steps'][1] == ('flip',)
        labels, conf = predict_seg.predict_volume(model, image, saved, patch, blend, True)
        assert np.array_equal(got.array, restore_native(labels, record).cpu().numpy())
        cf = read_nifti(os.path.join(str(out_dir), name + '_conf.nii.gz'))
        assert cf.array.shape == NATIVE and cf.array.dtype == np.float32 and np.array_equal(cf.array, restore_native(conf, record, 'linear').cpu().numpy())
        truth = read_nifti(os.path.join(str(root), name + '_masks.nii.gz')).array
        counts = ops.label_overlap_counts(torch.from_numpy(got.array)[None].to(DEV), torch.from_numpy(truth)[None].to(DEV), 32)
        dices.append(float(np.nanmean(metrics.dice_from_counts(counts)[0, 1:])))
        assert predict_seg.format_dice(name, dices[-1]) in run.stdout.splitlines()
    assert predict_seg.format_dice('mean over 2 scans', float(np.nanmean(dices))) in run.stdout.splitlines()


def test_predict_seg_whole_volume_route(tmp_path):
    """No `patch` in the config and no patch flag: one forward pass over the prepared volume; a shape the net cannot take is check_shapes' error."""
    import predict_seg
    from deepatlas_amd.lib import evalMetrics as metrics
    from deepatlas_amd.lib.network_factory import get_network
    from deepatlas_amd.lib.nifti import write_nifti
    root = tmp_path / 'scans'
    listing = write_scans(root)
    rng = np.random.RandomState(2)
    write_nifti(os.path.join(str(root), 'fits_image.nii.gz'), rng.uniform(0, 300, size=(8, 16, 32)).astype(np.int16), spacing=(1.0, 1.0, 2.0))
    cfg = bc.seg_config(tmp_path, ['--data', 'OAI', '--data-dir', str(root), '--train-list', listing, '--valid-list', listing, '--voxel-size', '1', '1', '1',
                                   '--rescale-percentiles', '0.5', '99.5'])
    args = predict_seg.build_parser().parse_args(['--ckpt', 'c', '--output-dir', 'o', '--input', 'x.nii.gz'])
    assert predict_seg.inference_settings(args, cfg) == (None, None)
    torch.manual_seed(7)
    model = get_network(cfg['model'])(**cfg['model_settings'])
    model.weights_init()
    model.to(DEV).eval()
    vol, image, record = predict_seg.prepare(os.path.join(str(root), 'fits_image.nii.gz'), 'fits', cfg)
    assert tuple(image.shape) == (1, 16, 16, 32) and [s[0] for s in record['steps']] == ['resample']
    labels, none = predict_seg.predict_volume(model, image, cfg, None, None, False)
    with torch.no_grad():
        want = metrics.eval_dice_counts(model(image[None]), torch.zeros((1, 16, 16, 32), dtype=torch.uint8, device=DEV))[1][0]
    assert none is None and torch.equal(labels, want)
    labels2, conf = predict_seg.predict_volume(model, image, cfg, None, None, True)      # one tile, constant window: the softmax's maximum
    assert tuple(conf.shape) == (16, 16, 32) and bool(((conf > 1.0 / 32) & (conf <= 1.0)).all())
    assert float((labels2 != want).float().mean()) <= 1e-3                               # argmax of the probabilities: ties of rounded softmax values aside
    from deepatlas_amd.lib.inference import restore_native
    assert tuple(restore_native(labels, record).shape) == (8, 16, 32)
    _, bad, _ = predict_seg.prepare(os.path.join(str(root), SCANS[0] + '_image.nii.gz'), SCANS[0], cfg)
    with pytest.raises(ValueError, match='multiples of 8'):
        predict_seg.predict_volume(model, bad, cfg, None, None, False)
