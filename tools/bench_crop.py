#!/usr/bin/env python
"""Timing of the crop kernels (csrc/crop.hip) and of patch training on one MI355X.
Case 1, a uint8 label map of 160 x 384 x 384 (the OAI size) with a float32 image, patch 32 x 128 x 128, N = 1 and 2, two kinds of labels
(blocky coordinate-function labels; the argmax of an untrained UNet_light): ops.window_label_counts, ops.sample_crop_starts for 1 and for 8
draws (BalancedRandomCrop's tag cycle 2, 3, 0, 1, ... at threshold 0.01: classes 2 and 1 and unconditioned draws) and ops.crop_gather, HIP
events on warm back-to-back calls, ROUNDS rounds, median and min - max, each with its share of the achievable HBM rate (6.3 TB/s) over its
COMPULSORY bytes (the labels once per class the draws name, every output byte once; the gather: every patch byte read once and written once).
Beside them, in the same run, for one draw of class 1:
  torch   F.avg_pool3d(mask.float(), window, stride=1) * volume, threshold, nonzero, index, slice.  The pooling visits every window voxel
          per output, so it is first timed at half the size per axis; the full size runs only if 64 x that time stays below --torch-budget s
  host    D -> H of labels and image, the reference's rejection loop (lib/transforms.py:445-457) restated in numpy, slice, H -> D; with
          its number of tries
Case 2, SegmentationExperiment on synthetic 160 x 192 x 160 volumes (UNet_light, 32 classes): the whole-volume training step, a patch step
(crop + step) of 1 and of 4 patches of 32 x 128 x 128, the whole-volume evaluation of one volume and its tiled evaluation (overlap 8).
Every ratio is a finding, not a gate.  Not measured: hardware counters, other sizes, dtypes and thresholds, int32 / int64 labels, real scans.
python tools/bench_crop.py [--iters 10] [--rounds 5] [--out profiles/crop_bench.json]"""
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
import torch.nn.functional as F
from deepatlas_amd import ops
from deepatlas_amd.lib import transforms as T
from bench_edt import HBM_ACHIEVABLE, alternate, untrained_argmax


def stats(ts):
    ts = np.asarray(ts)
    return {'ms': round(float(np.median(ts)), 4), 'ms_min': round(float(ts.min()), 4), 'ms_max': round(float(ts.max()), 4)}


def share(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 4)


def rejection_loop(lab, window, cls, threshold, rng, max_tries=500):
    """The reference's loop; gives up after max_tries (the reference would not) with the last start."""
    wd, wh, ww = window
    D, H, W = lab.shape
    tries = 0
    while True:
        tries += 1
        if tries > max_tries:
            return (z, y, x), -1
        z, y, x = (int(rng.randint(0, r)) if r > 0 else 0 for r in (D - wd, H - wh, W - ww))
        crop = lab[z:z + wd, y:y + wh, x:x + ww]
        if np.sum(crop == cls) / crop.size > threshold:
            return (z, y, x), tries


def torch_route(lab, img, window, cls, min_count, k_bits):
    """One conditioned draw by library calls: pooled mask, threshold over the domain, nonzero, index, slice."""
    wd, wh, ww = window
    vol = wd * wh * ww
    cnt = F.avg_pool3d((lab == cls).float()[None], window, stride=1)[0] * vol
    D, H, W = lab.shape[-3:]
    cnt = cnt[0, :max(D - wd, 1), :max(H - wh, 1), :max(W - ww, 1)]
    adm = torch.nonzero(torch.round(cnt) >= min_count)
    z, y, x = adm[(k_bits * adm.shape[0]) >> 32].tolist() if adm.shape[0] else (0, 0, 0)
    return img[:, :, z:z + wd, y:y + wh, x:x + ww].contiguous(), lab[:, z:z + wd, y:y + wh, x:x + ww].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shape', type=str, default='160x384x384')
    ap.add_argument('--patch', type=str, default='32x128x128')
    ap.add_argument('--torch-budget', type=float, default=60.0)
    ap.add_argument('--skip-experiment', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_crop.py measures on the GPU'
    dev = torch.device('cuda:0')
    shape = tuple(int(v) for v in a.shape.split('x'))
    window = tuple(int(v) for v in a.patch.split('x'))
    D, H, W = shape
    V, PV = D * H * W, window[0] * window[1] * window[2]
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps({'bench_crop': rows, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE,
                                    'not_measured': ['hardware counters', 'other sizes, dtypes and thresholds', 'int32 / int64 labels', 'real scans']}) + '\n')

    blocky = ((np.arange(D)[:, None, None] // 20 + np.arange(H)[None, :, None] // 48 + np.arange(W)[None, None, :] // 48) % 6).astype(np.uint8)
    kinds = {'blocky': torch.from_numpy(blocky).to(dev), 'untrained argmax': untrained_argmax(shape, dev)[0]}
    img1 = torch.rand((1, 1) + shape, generator=torch.Generator().manual_seed(3)).to(dev)
    m = T.crop_min_count(0.01, PV)
    tags = [2, 3, 0, 1, 2, 3, 0, 1]
    cyc = {0: None, 1: 1, 2: 2, 3: 2}
    for kind, lab1 in kinds.items():
        for N in (1, 2):
            lab = torch.stack([lab1, torch.roll(lab1, 7, 2)][:N], 0).contiguous()
            img = img1.expand(N, 1, D, H, W).contiguous()
            base = {'labels': kind, 'N': N, 'shape': list(shape), 'patch': list(window)}
            Vo = (D - window[0] + 1) * (H - window[1] + 1) * (W - window[2] + 1)
            k = lambda: ops.window_label_counts(lab, window, 1)
            s = stats(alternate([('k', k)], a.rounds, a.iters)['k'])
            comp = N * (V + 4 * Vo)
            emit(dict(base, variant='window_label_counts (class 1)', **s, compulsory_bytes=comp, share_of_achievable_hbm_over_compulsory=share(comp, s['ms'])))
            for P in (1, 8):
                classes = [cyc[t] for t in tags[:P]]
                n_cls = len(set(c for c in classes if c is not None))
                k = lambda: ops.sample_crop_starts(lab, window, classes, [m] * P, 17)
                s = stats(alternate([('k', k)], a.rounds, a.iters)['k'])
                _, info = k()
                comp = N * V * n_cls
                emit(dict(base, variant='sample_crop_starts, %d draw%s (classes %s)' % (P, '' if P == 1 else 's', classes), **s, compulsory_bytes=comp,
                          share_of_achievable_hbm_over_compulsory=share(comp, s['ms']), admissible=info[:, :, 0].tolist()))
                starts, _ = k()
                g = lambda: ops.crop_gather(img, lab, starts, window)
                s = stats(alternate([('k', g)], a.rounds, a.iters)['k'])
                comp = N * P * PV * (4 + 1) * 2
                emit(dict(base, variant='crop_gather, %d patch%s per sample, image + uint8 labels' % (P, '' if P == 1 else 'es'), **s, compulsory_bytes=comp,
                          share_of_achievable_hbm_over_compulsory=share(comp, s['ms'])))
            if N == 1:
                # the host route: everything the reference's transform needs on the host, and the patch back on the device
                rng = np.random.RandomState(5)
                tries = []

                def host():
                    l, i = lab[0].cpu().numpy(), img[0].cpu().numpy()
                    (z, y, x), t = rejection_loop(l, window, 1, 0.01, rng)
                    tries.append(t)
                    pi = torch.from_numpy(np.ascontiguousarray(i[:, z:z + window[0], y:y + window[1], x:x + window[2]])).to(dev)
                    pl = torch.from_numpy(np.ascontiguousarray(l[z:z + window[0], y:y + window[1], x:x + window[2]])).to(dev)
                    torch.cuda.synchronize()
                    return pi, pl
                host()
                ts = []
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    host()
                    ts.append((time.perf_counter() - t0) * 1e3)
                emit(dict(base, variant='host route: D -> H, rejection loop in numpy, slice, H -> D (class 1, threshold 0.01)', **stats(ts), tries=tries[1:], tries_note='-1: gave up after 500 tries'))
    # the torch composition, N = 1, blocky labels
    lab = kinds['blocky'][None]
    half = tuple(v // 2 for v in shape)
    hwin = tuple(v // 2 for v in window)
    lab_h, img_h = lab[:, :half[0], :half[1], :half[2]].contiguous(), img1[:, :, :half[0], :half[1], :half[2]].contiguous()
    mh = T.crop_min_count(0.01, hwin[0] * hwin[1] * hwin[2])
    torch_route(lab_h, img_h, hwin, 1, mh, 12345)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch_route(lab_h, img_h, hwin, 1, mh, 12345)
    torch.cuda.synchronize()
    half_ms = (time.perf_counter() - t0) * 1e3
    emit({'labels': 'blocky', 'N': 1, 'shape': list(half), 'patch': list(hwin), 'variant': 'torch composition at half the size per axis (one call)', 'ms': round(half_ms, 3)})
    if 64 * half_ms * 1e-3 < a.torch_budget:
        t0 = time.perf_counter()
        torch_route(lab, img1, window, 1, m, 12345)
        torch.cuda.synchronize()
        emit({'labels': 'blocky', 'N': 1, 'shape': list(shape), 'patch': list(window), 'variant': 'torch composition (one call, after the half-size warm-up)',
              'ms': round((time.perf_counter() - t0) * 1e3, 3)})
    else:
        emit({'labels': 'blocky', 'N': 1, 'shape': list(shape), 'patch': list(window), 'variant': 'torch composition', 'ms': None,
              'not_measured': 'projected %.0f s (64 x the half-size call) exceeds the budget of %.0f s' % (64 * half_ms * 1e-3, a.torch_budget)})
    if not a.skip_experiment:
        experiment_case(emit, a, window)


def experiment_case(emit, a, window):
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
    shape = (160, 192, 160)
    common = ['--num-samples', '1', '--num-epochs', '1', '--shape'] + [str(v) for v in shape] + ['--log-root', tempfile.mkdtemp()]
    train_seg.main(common)
    train_seg.main(common + ['--patch-size'] + [str(v) for v in window])
    whole, patch = SegmentationExperiment(seen[0]), SegmentationExperiment(seen[1])
    whole.setup_train()
    images, truths, _ = next(iter(whole.training_data_loader))
    images, truths = images.to(whole.device), truths.to(whole.device)
    base = {'shape': list(shape), 'patch': list(window), 'model': 'UNet_light, 32 classes'}

    def host_timed(fn, warm=2, n=5):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return stats(ts)
    emit(dict(base, variant='whole-volume training step', **host_timed(lambda: whole.train_step(images, truths))))
    with torch.no_grad():
        whole.model.eval()
        emit(dict(base, variant='whole-volume evaluation of one volume (forward + argmax + counts)',
                  **host_timed(lambda: ops.argmax_dice_counts(whole.model(images), truths))))
    del whole
    torch.cuda.empty_cache()
    patch.setup_train()
    for B in (1, 4):
        patch.config['batch_size'] = B
        patch.patch['per_volume'] = patch.crop.patches = B

        def step():
            out = patch.crop({'image': images, 'segmentation': truths})
            patch.train_step(out['image'], out['segmentation'])
        emit(dict(base, variant='patch step: balanced crop of %d patch%s from one volume + training step' % (B, '' if B == 1 else 'es'), **host_timed(step)))
    with torch.no_grad():
        patch.model.eval()
        emit(dict(base, variant='tiled evaluation of one volume (overlap 8, %d tiles, tile_batch 4: tiles, forward, argmax, assemble, counts)'
                  % int(np.prod(np.ceil(np.asarray(shape) / (np.asarray(window) - 16)))),
                  **host_timed(lambda: ops.label_overlap_counts(patch.predict_tiled(images), truths, 32), warm=1, n=3)))


if __name__ == '__main__':
    main()
