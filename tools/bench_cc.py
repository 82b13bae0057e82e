#!/usr/bin/env python
"""Timing of the connected-component clean-up (csrc/cc.hip) at 80x96x80 and 160x192x160, N = 1, n_class = 32, on four label maps:
the blocky maps of synthetic_batch_on_device(structured=True); the argmax of an untrained UNet_light (noise: the most components); one
label everywhere (the worst case of the size atomics and of the root's chains); a one-voxel-wide serpentine through the whole volume.
Per input and connectivity: ops.keep_largest_component in total and its three C entries (da_cc_label, da_cc_select, da_cc_filter) with HIP
events on warm back-to-back calls, ROUNDS rounds, median and min - max; the kernels inside da_cc_label (local, seam, flatten) from one
torch.profiler trace where the profiler is available.  Nominal bytes per kernel (uint8 labels): local 9 V (labels, parent, zeroed sizes),
flatten 8 V (parent, roots), select 4 V (sizes), filter 6 V (labels, roots, output); the compulsory total is the label map + four int32
passes = 17 V; rates are shares of the achievable HBM rate (6.3 TB/s).  The seam pass is a pointer chase and has no nominal byte count.
Baseline, what users do today: D->H copy, scipy.ndimage.label per present class, the selection in numpy, H->D copy, classes spread over
16 threads (and serially; the faster is the baseline).  The ratio is a finding, not a gate.
Last: one validation pass of SegmentationExperiment (2 volumes) with and without config['postprocess'].
python tools/bench_cc.py [--iters 10] [--rounds 5] [--shapes 80x96x80 160x192x160] [--out profiles/cc_bench.json]"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from deepatlas_amd import _native as nat
from deepatlas_amd import ops

HBM_ACHIEVABLE = 6.3e12      # bytes / s
N_CLASS = 32
NOMINAL_BYTES = {'da_cc_label': None, 'da_cc_select': 4, 'da_cc_filter': 6, 'cc_local_kernel': 9, 'cc_seam_kernel': None, 'cc_flatten_kernel': 8}


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, rounds, iters):
    for _, fn in variants:
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(timed(fn, iters))
    return times


def host_keep_largest(lab_dev, connectivity, workers):
    """The route without the kernels: copy to the host, scipy.ndimage.label per present class, keep the largest, copy back."""
    from scipy import ndimage
    import cc_cases
    structure = cc_cases.structure(connectivity)
    vol = lab_dev[0].cpu().numpy()
    out = np.zeros_like(vol)

    def one(c):
        comp, k = ndimage.label(vol == c, structure)
        if k:
            out[comp == int(np.argmax(np.bincount(comp.ravel())[1:])) + 1] = c      # the first maximum: scipy numbers by first voxel
    classes = [int(c) for c in np.unique(vol) if 0 < c < N_CLASS]
    if workers > 1:
        with concurrent.futures.ThreadPoolExecutor(workers) as pool:
            list(pool.map(one, classes))
    else:
        for c in classes:
            one(c)
    return torch.from_numpy(out)[None].to(lab_dev.device)


def untrained_argmax(shape, dev):
    from deepatlas_amd.lib.network_factory import get_network
    ops.set_matrix_precision(ops.DEFAULT_MATRIX_PRECISION)
    torch.manual_seed(0)
    net = get_network('UNet_light')(in_channel=1, n_classes=N_CLASS, bias=True, BN=True)
    net.weights_init()
    net.to(dev).eval()
    g = torch.Generator().manual_seed(11)
    x = torch.rand((1, 1) + tuple(shape), generator=g).to(dev)
    with torch.no_grad():
        _, pred = ops.argmax_dice_counts(net(x), torch.zeros((1,) + tuple(shape), dtype=torch.uint8, device=dev))
    del net
    torch.cuda.empty_cache()
    return pred


def kernel_breakdown(fn):
    """{kernel name: ms} of one call of fn from a torch.profiler trace, or None where the profiler yields no device events."""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for k in ('cc_local_kernel', 'cc_seam_kernel', 'cc_flatten_kernel', 'cc_select_kernel', 'cc_filter_kernel'):
                if k in ev.key:
                    t = getattr(ev, 'device_time_total', None)
                    if t is None:
                        t = getattr(ev, 'cuda_time_total', 0.0)
                    out[k] = out.get(k, 0.0) + float(t) / 1e3 / max(ev.count, 1)
        return out or None
    except Exception as e:          # the tool still reports the per-entry times; it says why the per-kernel ones are missing
        return {'unavailable': repr(e)}


def bench_shape(a, shape, rows):
    import cc_cases
    from deepatlas_amd.lib.datasets import synthetic_batch_on_device
    dev = torch.device('cuda:0')
    D, H, W = shape
    V = D * H * W
    inputs = [('structured', synthetic_batch_on_device(1, shape, N_CLASS, structured=True, device=dev)[1]),
              ('untrained argmax', untrained_argmax(shape, dev)),
              ('one label', torch.ones((1,) + tuple(shape), dtype=torch.uint8, device=dev)),
              ('serpentine', torch.from_numpy(cc_cases.serpentine(shape)).to(dev))]
    L = nat.lib()
    st = nat.stream()
    for iname, lab in inputs:
        for conn in a.connectivities:
            roots = torch.empty((1, D, H, W), dtype=torch.int32, device=dev)
            sizes = torch.empty_like(roots)
            out = torch.empty_like(lab)
            ws = torch.empty(L.da_cc_ws_bytes(1, D, H, W) + 256, dtype=torch.uint8, device=dev)
            best = torch.zeros((1, N_CLASS), dtype=torch.int64, device=dev)
            stats = torch.zeros((1, N_CLASS, 3), dtype=torch.int64, device=dev)

            def label():
                nat.call('da_cc_label', nat.ptr(lab), 1, 1, D, H, W, N_CLASS, conn, nat.ptr(roots), nat.ptr(sizes), nat.ptr(ws), ws.numel(), st)

            def select():
                best.zero_(); stats.zero_()
                nat.call('da_cc_select', nat.ptr(lab), 1, nat.ptr(sizes), 1, V, N_CLASS, nat.ptr(best), nat.ptr(stats), st)

            def filt():
                nat.call('da_cc_filter', nat.ptr(lab), 1, nat.ptr(roots), nat.ptr(sizes), nat.ptr(best), 1, V, N_CLASS, 0, 1, nat.ptr(out), st)

            total = lambda: ops.keep_largest_component(lab, N_CLASS, conn, return_stats=True)
            variants = [('keep_largest_component', total), ('da_cc_label', label), ('da_cc_select', select), ('da_cc_filter', filt)]
            times = alternate(variants, a.rounds, a.iters)
            kept, s = total()
            n_comp, largest = int(s[0, :, 0].sum()), int(s[0, :, 1].max())
            per_kernel = kernel_breakdown(total)
            for name, _ in variants:
                t = np.array(times[name])
                row = {'variant': name, 'input': iname, 'connectivity': conn, 'shape': [D, H, W], 'N': 1, 'n_class': N_CLASS, 'components': n_comp,
                       'largest': largest, 'ms': round(float(np.median(t)), 4), 'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4)}
                nb = 17 if name == 'keep_largest_component' else NOMINAL_BYTES[name]
                line = '%-24s %-17s conn %2d %-12s %9.4f ms (%.4f - %.4f)' % (name, iname, conn, 'x'.join(map(str, shape)), row['ms'], row['ms_min'], row['ms_max'])
                if nb:
                    rate = nb * V / (row['ms'] * 1e-3)
                    row.update(nominal_bytes=nb * V, GBps=round(rate / 1e9, 1), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 4))
                    line += '  %7.1f GB/s  %.3f of 6.3 TB/s' % (row['GBps'], row['share_of_achievable_hbm'])
                rows.append(row)
                print(line, flush=True)
            if per_kernel and 'unavailable' not in per_kernel:
                row = {'variant': 'kernels of one keep_largest_component call', 'input': iname, 'connectivity': conn, 'shape': [D, H, W],
                       'ms': {k: round(v, 4) for k, v in per_kernel.items()},
                       'share_of_achievable_hbm': {k: round(NOMINAL_BYTES[k] * V / (v * 1e-3) / HBM_ACHIEVABLE, 4)
                                                   for k, v in per_kernel.items() if NOMINAL_BYTES.get(k) and v > 0}}
            else:
                row = {'variant': 'kernels of one keep_largest_component call', 'input': iname, 'connectivity': conn, 'shape': [D, H, W], 'ms': per_kernel}
            rows.append(row)
            print(json.dumps(row), flush=True)
            if conn == a.connectivities[0]:
                host = {}
                for workers in (16, 1):
                    t0 = time.perf_counter()
                    ref = host_keep_largest(lab, conn, workers)
                    torch.cuda.synchronize()
                    host[workers] = (time.perf_counter() - t0) * 1e3
                dev_ms = float(np.median(times['keep_largest_component']))
                row = {'variant': 'host baseline (scipy.ndimage.label per class)', 'input': iname, 'connectivity': conn, 'shape': [D, H, W],
                       'ms_16_threads': round(host[16], 1), 'ms_serial': round(host[1], 1), 'equal_to_device': bool(torch.equal(ref, kept)),
                       'baseline_over_device': round(min(host.values()) / dev_ms, 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)


def bench_validation(a, shape, rows):
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    import contextlib
    import io
    import tempfile
    ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                            data_root='./data', log_root=tempfile.mkdtemp(), shape=list(shape))
    with contextlib.redirect_stdout(io.StringIO()):
        exp = SegmentationExperiment(train_seg.build_config(ns))
        exp.setup_model(); exp.setup_loss(); exp.setup_train_data(); exp.setup_optimizer()
        exp.initialize_model(exp.model, exp.optimizer, '')
    res = {}
    for key, post in (('without', None), ('largest_cc', 'largest_cc'), ('without (again)', None)):
        exp.config['postprocess'] = post
        exp.eval(exp.validation_data_loader)
        ts = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            exp.eval(exp.validation_data_loader)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[key] = round(float(np.median(ts)), 2)
    row = {'variant': 'validation pass, 2 volumes (untrained net)', 'shape': list(shape), 'ms': res,
           'postprocess_cost_ms': round(res['largest_cc'] - min(res['without'], res['without (again)']), 2)}
    rows.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--connectivities', type=int, nargs='+', default=[6, 26])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_cc.py measures on the GPU'
    rows = []
    for s in a.shapes:
        shape = tuple(int(v) for v in s.split('x'))
        bench_shape(a, shape, rows)
        bench_validation(a, shape, rows)
    out = json.dumps({'bench_cc': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
