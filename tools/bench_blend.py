#!/usr/bin/env python
"""Timing of the blending kernels (csrc/blend.hip) and of blended tiled inference on one MI355X.
Case 1, K = 32 classes, a 160 x 384 x 384 volume, tiles of 32 x 128 x 128 at overlap 8 (160 tiles) and at overlap t / 4 (a stride of half a
tile, 360 tiles), drawn N(0, 4^2) tile logits resident on the device: one sweep of ops.blend_accumulate over all tiles in chunks of
--tile-batch tiles (what SlidingWindowPredictor issues per flip pass) and ops.blend_finalize (with and without the confidence), HIP events on
warm calls, ROUNDS rounds, median and min - max, each with its share of the achievable HBM rate (6.3 TB/s) over its COMPULSORY bytes: every
in-volume tile logit read once, the accumulator read and written once per covering tile, the labels written (the kernel moves fewer
accumulator bytes than that: it reads and writes a voxel once per CALL, not once per covering tile).  Beside them, alternating in the same run,
the torch composition on the device: per tile softmax, window multiply and a slice add into the accumulator, then argmax.  The error of both
against the float64 evaluation (the same torch composition in float64 on the device), as the largest |acc - acc64| / weight sum.
Case 2, SegmentationExperiment on one synthetic 160 x 384 x 384 volume (UNet_light, 32 classes, untrained), patch 32 x 128 x 128, overlap 8,
tile_batch 4: one whole predict_tiled with tile_blend off (argmax per tile + core copy), 'gaussian', and 'gaussian' with three mirror axes.
Every ratio is a finding, not a gate.  Not measured: hardware counters, other K / sizes / tile shapes, K not a multiple of 4, real scans,
predict_seg.py's file reading and writing.
python tools/bench_blend.py [--rounds 5] [--tile-batch 4] [--out profiles/blend_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
from deepatlas_amd import ops
from deepatlas_amd.lib.transforms import importance_window
from bench_edt import HBM_ACHIEVABLE, alternate

NOT_MEASURED = ['hardware counters', 'other class counts, volume sizes and tile shapes', 'K that is no multiple of 4', 'real scans',
                "predict_seg.py's file reading and writing"]


def stats(ts):
    ts = np.asarray(ts)
    return {'ms': round(float(np.median(ts)), 4), 'ms_min': round(float(ts.min()), 4), 'ms_max': round(float(ts.max()), 4)}


def share(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 4)


def tile_boxes(vol, tile, overlap):
    """Per tile, raster order: (volume slices, local slices) of its in-volume part."""
    e = [t - 2 * o for t, o in zip(tile, overlap)]
    g = [-(-s // a) for s, a in zip(vol, e)]
    out = []
    for i in range(g[0]):
        for j in range(g[1]):
            for k in range(g[2]):
                vs, ls = [], []
                for a, ea, o, t, s in zip((i, j, k), e, overlap, tile, vol):
                    lo, hi = max(a * ea - o, 0), min(a * ea - o + t, s)
                    vs.append(slice(lo, hi))
                    ls.append(slice(lo - (a * ea - o), hi - (a * ea - o)))
                out.append((tuple(vs), tuple(ls)))
    return out


def torch_accumulate(acc, logits, boxes, w3):
    """logits T x tz x ty x tx x K (channels-last memory): softmax, window multiply, slice adds."""
    for t, (vs, ls) in enumerate(boxes):
        p = torch.softmax(logits[t].to(acc.dtype), -1) * w3[..., None]
        acc[vs] += p[ls]
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--tile-batch', type=int, default=4)
    ap.add_argument('--shape', type=str, default='160x384x384')
    ap.add_argument('--tile', type=str, default='32x128x128')
    ap.add_argument('--classes', type=int, default=32)
    ap.add_argument('--skip-experiment', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_blend.py measures on the GPU'
    dev = torch.device('cuda:0')
    vol = tuple(int(v) for v in a.shape.split('x'))
    tile = tuple(int(v) for v in a.tile.split('x'))
    K, V = a.classes, int(np.prod(vol))
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps({'bench_blend': rows, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE, 'not_measured': NOT_MEASURED}) + '\n')

    win = importance_window(tile, 'gaussian')
    w3 = ((torch.from_numpy(win[0])[:, None, None] * torch.from_numpy(win[1])[None, :, None]) * torch.from_numpy(win[2])[None, None, :]).to(dev)
    for overlap in ((8, 8, 8), tuple(t // 4 for t in tile)):
        boxes = tile_boxes(vol, tile, overlap)
        T = len(boxes)
        covered = sum(int(np.prod([s.stop - s.start for s in vs])) for vs, _ in boxes)          # in-volume tile voxels = sum over voxels of covering tiles
        base = {'shape': list(vol), 'tile': list(tile), 'overlap': list(overlap), 'K': K, 'tiles': T, 'tile_batch': a.tile_batch,
                'mean_covering_tiles_per_voxel': round(covered / V, 3)}
        logits = torch.empty((T,) + tile + (K,), dtype=torch.float32, device=dev).normal_(0.0, 4.0, generator=torch.Generator(device=dev).manual_seed(7))
        view = logits.permute(0, 4, 1, 2, 3)
        acc = torch.zeros(vol + (K,), dtype=torch.float32, device=dev)
        acc_t = torch.zeros_like(acc)

        def kernel_sweep():
            for k in range(0, T, a.tile_batch):
                ops.blend_accumulate(acc, view[k:k + a.tile_batch], k, tile, overlap, win)

        def torch_sweep():
            torch_accumulate(acc_t, logits, boxes, w3)
        times = alternate([('kernel', kernel_sweep), ('torch', torch_sweep)], a.rounds, 1)
        comp = covered * K * 4 * 3
        s = stats(times['kernel'])
        emit(dict(base, variant='blend_accumulate, one sweep over all tiles (%d calls)' % -(-T // a.tile_batch), **s, compulsory_bytes=comp,
                  share_of_achievable_hbm_over_compulsory=share(comp, s['ms'])))
        s = stats(times['torch'])
        emit(dict(base, variant='torch composition: per tile softmax, window multiply, slice add', **s, compulsory_bytes=comp,
                  share_of_achievable_hbm_over_compulsory=share(comp, s['ms'])))
        # the error of one sweep from zero against float64 on the device (both accumulators restarted)
        acc.zero_(); acc_t.zero_()
        kernel_sweep(); torch_sweep()
        acc64 = torch_accumulate(torch.zeros(vol + (K,), dtype=torch.float64, device=dev), logits, boxes, w3.double())
        wsum = acc64.sum(-1, keepdim=True)
        err = {'kernel': float(((acc.double() - acc64).abs() / wsum).max()), 'torch float32': float(((acc_t.double() - acc64).abs() / wsum).max())}
        lab64 = acc64.argmax(-1)
        del acc64, wsum
        fin = alternate([('labels', lambda: ops.blend_finalize(acc)), ('labels + confidence', lambda: ops.blend_finalize(acc, return_conf=True)),
                         ('torch argmax', lambda: acc.argmax(-1).to(torch.uint8))], a.rounds, 3)
        differ = int((ops.blend_finalize(acc).long() != lab64).sum())
        emit(dict(base, variant='error of one sweep against the float64 evaluation: largest |acc - acc64| / weight sum', error=err,
                  labels_differing_from_float64_argmax=differ, voxels=V))
        for name, extra in (('labels', 1), ('labels + confidence', 5)):
            s = stats(fin[name])
            comp = V * (K * 4 + extra)
            emit(dict(base, variant='blend_finalize, ' + name, **s, compulsory_bytes=comp, share_of_achievable_hbm_over_compulsory=share(comp, s['ms'])))
        s = stats(fin['torch argmax'])
        emit(dict(base, variant='torch composition: argmax over the classes, cast to uint8', **s, compulsory_bytes=V * (K * 4 + 1),
                  share_of_achievable_hbm_over_compulsory=share(V * (K * 4 + 1), s['ms'])))
        del logits, view, acc, acc_t, lab64
        torch.cuda.empty_cache()
    if not a.skip_experiment:
        experiment_case(emit, vol, tile)


def experiment_case(emit, vol, tile):
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    seen = []

    class Capture(object):
        def __init__(self, config):
            seen.append(config)

        def train(self):
            pass

        def test(self):
            pass
    train_seg.SegmentationExperiment = Capture
    common = (['--num-samples', '1', '--num-epochs', '1', '--shape'] + [str(v) for v in vol] + ['--log-root', tempfile.mkdtemp(), '--patch-size']
              + [str(v) for v in tile])
    for extra in ([], ['--tile-blend', 'gaussian'], ['--tile-blend', 'gaussian', '--tile-mirror', 'zyx']):
        train_seg.main(common + extra)
    images = torch.rand((1, 1) + tuple(vol), generator=torch.Generator().manual_seed(3)).to('cuda:0')
    state = None
    for cfg, name in zip(seen, ('tile_blend off: argmax per tile, core copy', "tile_blend 'gaussian'", "tile_blend 'gaussian', mirror z y x (8 passes)")):
        exp = SegmentationExperiment(cfg)
        exp.setup_model()
        if state is None:
            torch.manual_seed(0)
            exp.model.weights_init()
            state = exp.model.state_dict()
        exp.model.load_state_dict(state)
        exp.model.eval()
        ops.set_matrix_precision(ops.DEFAULT_MATRIX_PRECISION)
        ts = []
        with torch.no_grad():
            exp.predict_tiled(images)
            torch.cuda.synchronize()
            for _ in range(3):
                t0 = time.perf_counter()
                exp.predict_tiled(images)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
        emit({'shape': list(vol), 'tile': list(tile), 'overlap': [8, 8, 8], 'tile_batch': 4, 'model': 'UNet_light, 32 classes, untrained',
              'variant': 'predict_tiled of one volume, ' + name, **stats(ts)})
        del exp
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
