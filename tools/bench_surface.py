#!/usr/bin/env python
"""Timing of the surface-distance metrics (ops.surface_distance_stats, csrc/edt.hip) at 80x96x80 and 160x192x160, N = 1, n_class = 32.
Truth: the blocky maps of synthetic_batch_on_device(structured=True).  Predictions: the truth shifted by (1, 2, 3) voxels, the truth with a
tenth of its voxels relabelled at random, and the argmax of an untrained UNet_light (noise: every voxel a surface voxel).
Per input: the op and ops.signed_distance_maps of the same truth (both run two transforms per class: the difference is what the counting,
gather and select passes and the surface predicate cost) with HIP events on warm back-to-back calls, ROUNDS rounds, median and min - max; the
passes of one call from a torch.profiler trace where the profiler is available, each with the bytes it moves by the model below and the share
of the achievable HBM rate (6.3 TB/s) that makes.  Model, K' classes, V voxels, S pooled surface voxels: counting 2 K' V (both maps, a byte a
voxel and class), row pass 2 K' V (1 + 4), line passes 2 K' V 8 each, gather 2 K' V + 8 S, select 3 x 4 S.
Baseline, what users do today: D->H copy, scipy binary_erosion and distance_transform_edt twice per class, numpy percentile, on 16 threads
and serially; its results must equal the device's (counts and hd exactly, the rest within 1e-12).  The ratio is a finding, not a gate.
Last: a validation pass of SegmentationExperiment (2 volumes) without the key (the parent commit's pass: the same route) and with
config['surface_metrics'].
Not measured here: N > 1, hardware counters, other connectivities and spacings.
python tools/bench_surface.py [--iters 10] [--rounds 5] [--shapes 80x96x80 160x192x160] [--out profiles/surface_bench.json]"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
from deepatlas_amd import ops
from bench_edt import HBM_ACHIEVABLE, N_CLASS, CLASSES, alternate, untrained_argmax

KERNELS = {'sd_count_kernel': 'counting', 'sd_scan_kernel': 'segment offsets', 'edt_surface_row_kernel': 'row pass (W)',
           'edt_line_kernel<false>': 'line pass (H)', 'edt_line_kernel<true>': 'line pass (D)', 'sd_gather_kernel': 'gather',
           'sd_finish_kernel': 'sums + select'}
STAT_RTOL = 1e-12


def kernel_breakdown(fn):
    """{pass: ms summed over the launches of one call of fn} from a torch.profiler trace, or why it is missing."""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for k, label in KERNELS.items():
                if k in ev.key:
                    t = getattr(ev, 'device_time_total', None)
                    if t is None:
                        t = getattr(ev, 'cuda_time_total', 0.0)
                    out[label] = out.get(label, 0.0) + float(t) / 1e3
        return {k: round(v, 4) for k, v in out.items()} or {'unavailable': 'no device events'}
    except Exception as e:
        return {'unavailable': repr(e)}


def host_stats(pred_dev, truth_dev, workers):
    """The route without the kernels: copy to the host, per class two erosions, two scipy transforms and numpy's percentile."""
    from scipy import ndimage
    p, t = pred_dev[0].cpu().numpy(), truth_dev[0].cpu().numpy()
    st = ndimage.generate_binary_structure(3, 1)
    out = np.full((1, len(CLASSES), 7), np.nan)

    def one(j):
        a, b = p == CLASSES[j], t == CLASSES[j]
        sa, sb = a & ~ndimage.binary_erosion(a, st), b & ~ndimage.binary_erosion(b, st)
        out[0, j, 0], out[0, j, 1] = sa.sum(), sb.sum()
        if not sa.any() or not sb.any():
            return
        d_pt, d_tp = ndimage.distance_transform_edt(~sb)[sa], ndimage.distance_transform_edt(~sa)[sb]
        out[0, j, 2:] = (max(d_pt.max(), d_tp.max()), np.percentile(np.concatenate([d_pt, d_tp]), 95.0), (d_pt.mean() + d_tp.mean()) / 2,
                         d_pt.mean(), d_tp.mean())
    if workers > 1:
        with concurrent.futures.ThreadPoolExecutor(workers) as pool:
            list(pool.map(one, range(len(CLASSES))))
    else:
        for j in range(len(CLASSES)):
            one(j)
    return out


def assert_equal(dev_stats, host, what):
    g = dev_stats.cpu().numpy()
    ok = ~np.isnan(host)
    assert np.array_equal(np.isnan(g), ~ok) and np.array_equal(g[..., :3], host[..., :3], equal_nan=True), 'counts or hd differ on %s' % what
    assert np.all(np.abs(g[ok] - host[ok]) <= STAT_RTOL * np.abs(host[ok])), 'the host route and the device disagree on %s' % what


def bench_shape(a, shape, rows):
    from deepatlas_amd.lib.datasets import synthetic_batch_on_device
    dev = torch.device('cuda:0')
    D, H, W = shape
    V, Kp = D * H * W, len(CLASSES)
    truth = synthetic_batch_on_device(1, shape, N_CLASS, structured=True, device=dev)[1].contiguous()
    shifted = torch.zeros_like(truth)
    shifted[:, 1:, 2:, 3:] = truth[:, :-1, :-2, :-3]
    g = torch.Generator().manual_seed(7)
    hit = (torch.rand(truth.shape, generator=g) < 0.1).to(dev)
    noisy = torch.where(hit, torch.randint(0, N_CLASS, truth.shape, generator=g).to(dev).to(truth.dtype), truth)
    inputs = [('shifted (1,2,3)', shifted), ('noisy 0.1', noisy), ('untrained argmax', untrained_argmax(shape, dev))]
    for i, (iname, pred) in enumerate(inputs):
        pred = pred.contiguous()
        op = lambda: ops.surface_distance_stats(pred, truth, N_CLASS)
        maps = lambda: ops.signed_distance_maps(truth, N_CLASS)
        times = alternate([('surface_distance_stats', op), ('signed_distance_maps', maps)], a.rounds, a.iters)
        s = op()
        S = int(s[..., :2].sum())
        defined = int((~torch.isnan(s[..., 2])).sum())
        passes = kernel_breakdown(op)
        model = {'counting': 2 * Kp * V, 'row pass (W)': 2 * Kp * V * 5, 'line pass (H)': 2 * Kp * V * 8, 'line pass (D)': 2 * Kp * V * 8,
                 'gather': 2 * Kp * V + 8 * S, 'sums + select': 12 * S}
        shares = {k: round(model[k] / (passes[k] * 1e-3) / HBM_ACHIEVABLE, 4) for k in model if passes.get(k)}
        t_op, t_maps = np.array(times['surface_distance_stats']), np.array(times['signed_distance_maps'])
        row = {'variant': 'surface_distance_stats', 'input': iname, 'shape': list(shape), 'N': 1, 'n_class': N_CLASS, 'classes': Kp,
               'classes_defined': defined, 'pooled_surface_voxels': S, 'ms': round(float(np.median(t_op)), 4),
               'ms_min': round(float(t_op.min()), 4), 'ms_max': round(float(t_op.max()), 4),
               'signed_distance_maps_ms': round(float(np.median(t_maps)), 4),
               'over_signed_distance_maps_ms': round(float(np.median(t_op) - np.median(t_maps)), 4),
               'hd95_mean': round(float(np.nanmean(s[..., 3].cpu().numpy())), 3), 'assd_mean': round(float(np.nanmean(s[..., 4].cpu().numpy())), 3),
               'passes_ms': passes, 'passes_share_of_achievable_hbm': shares}
        rows.append(row)
        print(json.dumps(row), flush=True)
        host = {}
        for workers in ([a.host_threads, 1] if i == 0 or a.serial_everywhere else [a.host_threads]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = host_stats(pred, truth, workers)
            host['%d threads' % workers if workers > 1 else 'serial'] = round((time.perf_counter() - t0) * 1e3, 1)
            assert_equal(s, ref, '%s %s' % (iname, shape))
        best = min(host.values())
        row = {'variant': 'host baseline (D->H, scipy erosion + transform per class, numpy percentile)', 'input': iname, 'shape': list(shape),
               'ms': host, 'equal_to_device': True, 'baseline_over_device': round(best / float(np.median(t_op)), 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)


def bench_eval(a, shape, rows):
    import contextlib
    import io
    import tempfile
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                            data_root='./data', log_root=tempfile.mkdtemp(), shape=list(shape))
    with contextlib.redirect_stdout(io.StringIO()):
        exp = SegmentationExperiment(train_seg.build_config(ns))
        exp.setup_model(); exp.setup_train_data()
    res = {'without': [], 'surface_metrics': []}
    for key in res:
        exp.config.pop('surface_metrics', None)
        if key == 'surface_metrics':
            exp.config['surface_metrics'] = True
        exp.eval(exp.validation_data_loader)
    for _ in range(a.rounds):
        for key in res:
            exp.config.pop('surface_metrics', None)
            if key == 'surface_metrics':
                exp.config['surface_metrics'] = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            exp.eval(exp.validation_data_loader)
            torch.cuda.synchronize()
            res[key].append((time.perf_counter() - t0) * 1e3)
    med = {k: round(float(np.median(v)), 2) for k, v in res.items()}
    row = {'variant': 'SegmentationExperiment.eval (UNet_light, 2 volumes)', 'shape': list(shape), 'ms': med,
           'ms_min_max': {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()},
           'surface_metrics_cost_ms': round(med['surface_metrics'] - med['without'], 2),
           'note': 'without the key the pass takes the route of the parent commit'}
    rows.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-threads', type=int, default=16)
    ap.add_argument('--serial-everywhere', action='store_true', help='time the serial host route on every input, not only the first of a shape')
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_surface.py measures on the GPU'
    assert 1 <= a.host_threads <= 16
    rows = []
    for s in a.shapes:
        shape = tuple(int(v) for v in s.split('x'))
        bench_shape(a, shape, rows)
        bench_eval(a, shape, rows)
    out = json.dumps({'bench_surface': rows, 'not_measured': ['N > 1', 'hardware counters', 'connectivity 18 / 26', 'anisotropic spacing']})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
