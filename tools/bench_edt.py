#!/usr/bin/env python
"""Timing of the distance transform, the signed distance maps and the boundary loss (csrc/edt.hip) at 80x96x80 and 160x192x160, N = 1,
n_class = 32, on two label maps: the blocky maps of synthetic_batch_on_device(structured=True) and the argmax of an untrained UNet_light
(noise: short distances everywhere).
Per input: ops.distance_transform_edt of the mask `label != the most frequent label` and ops.signed_distance_maps of the 31 foreground classes with HIP
events on warm back-to-back calls, ROUNDS rounds, median and min - max; the three passes of each (row pass along W, line pass along H, line
pass along D) from one torch.profiler trace where the profiler is available; da_boundary_loss_fwd / _bwd on random logits and those maps.
Compulsory bytes: the transform reads the mask (1 byte) and writes a float per voxel, 5 V; the signed maps read the labels and write K' floats
per voxel, (1 + 4 K') V; the loss forward reads logits and maps, 4 (K + K') V, the backward also writes the gradient, 4 (2 K + K') V.  What the
passes really move is more: every pass reads and writes a float per voxel and site set, and the signed maps run two transforms per class.
Rates are shares of the achievable HBM rate (6.3 TB/s) over the COMPULSORY bytes.
Baseline, what users do today: D->H copy, scipy.ndimage.distance_transform_edt twice per class (inside and outside) on at most 16 threads,
H->D copy; the result must equal the device's bit for bit.  The ratio is a finding, not a gate.
Last: training steps of SegmentationExperiment without the key (the parent commit's step: the same route, bit for bit) and with
lambda_boundary = 1.
python tools/bench_edt.py [--iters 10] [--rounds 5] [--shapes 80x96x80 160x192x160] [--out profiles/edt_bench.json]"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from deepatlas_amd import _native as nat
from deepatlas_amd import ops

HBM_ACHIEVABLE = 6.3e12      # bytes / s
N_CLASS = 32
CLASSES = list(range(1, N_CLASS))
KERNELS = {'edt_row_kernel': 'row pass (W)', 'edt_line_kernel<false>': 'line pass (H)', 'edt_line_kernel<true>': 'line pass (D)'}


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


def host_signed_maps(lab_dev, workers):
    """The route without the kernels: copy to the host, two scipy transforms per class, copy back."""
    from scipy import ndimage
    vol = lab_dev[0].cpu().numpy()
    out = np.zeros((len(CLASSES),) + vol.shape, dtype=np.float32)

    def one(j):
        inside = vol == CLASSES[j]
        if inside.any() and not inside.all():
            out[j] = ndimage.distance_transform_edt(~inside) - ndimage.distance_transform_edt(inside)
    with concurrent.futures.ThreadPoolExecutor(workers) as pool:
        list(pool.map(one, range(len(CLASSES))))
    return torch.from_numpy(out)[None].to(lab_dev.device)


def finite_max(t):
    """Largest finite entry, rounded; None where there is none (a mask without a zero voxel is +inf everywhere)."""
    f = t[torch.isfinite(t)]
    return round(float(f.max()), 2) if f.numel() else None


def stats_row(name, iname, shape, t, nbytes, extra=None):
    t = np.array(t)
    ms = float(np.median(t))
    rate = nbytes / (ms * 1e-3)
    row = {'variant': name, 'input': iname, 'shape': list(shape), 'N': 1, 'n_class': N_CLASS, 'ms': round(ms, 4), 'ms_min': round(float(t.min()), 4),
           'ms_max': round(float(t.max()), 4), 'compulsory_bytes': int(nbytes), 'GBps': round(rate / 1e9, 1),
           'share_of_achievable_hbm': round(rate / HBM_ACHIEVABLE, 4)}
    row.update(extra or {})
    print('%-28s %-17s %-12s %9.4f ms (%.4f - %.4f)  %7.1f GB/s  %.4f of 6.3 TB/s' % (name, iname, 'x'.join(map(str, shape)), row['ms'], row['ms_min'],
                                                                                      row['ms_max'], row['GBps'], row['share_of_achievable_hbm']), flush=True)
    return row


def bench_shape(a, shape, rows):
    from deepatlas_amd.lib.datasets import synthetic_batch_on_device
    dev = torch.device('cuda:0')
    D, H, W = shape
    V = D * H * W
    K, Kp = N_CLASS, len(CLASSES)
    inputs = [('structured', synthetic_batch_on_device(1, shape, N_CLASS, structured=True, device=dev)[1]),
              ('untrained argmax', untrained_argmax(shape, dev))]
    L = nat.lib()
    st = nat.stream()
    g = torch.Generator().manual_seed(5)
    logits = torch.randn((1, D, H, W, K), generator=g).to(dev)               # channels-last, as the network delivers them
    slots = torch.tensor([-1] + list(range(Kp)), dtype=torch.int32, device=dev)
    for iname, lab in inputs:
        lab = lab.contiguous()
        frequent = int(torch.bincount(lab.flatten().long(), minlength=N_CLASS).argmax())
        mask = (lab != frequent).to(torch.uint8)             # the zero set = the voxels of the most frequent label
        edt = lambda: ops.distance_transform_edt(mask, squared=True)
        maps = lambda: ops.signed_distance_maps(lab, N_CLASS)
        phi = maps()
        loss = torch.empty(1, device=dev)
        dz = torch.empty_like(logits)
        gl = torch.ones(1, device=dev)
        ws = torch.empty(L.da_boundary_loss_ws_bytes(1) + 256, dtype=torch.uint8, device=dev)

        def fwd():
            nat.call('da_boundary_loss_fwd', nat.ptr(logits), nat.ptr(phi), nat.ptr(slots), 1, V, K, Kp, nat.ptr(loss), nat.ptr(ws), ws.numel(), st)

        def bwd():
            nat.call('da_boundary_loss_bwd', nat.ptr(logits), nat.ptr(phi), nat.ptr(slots), nat.ptr(gl), 1, V, K, Kp, nat.ptr(dz), st)
        times = alternate([('distance_transform_edt', edt), ('signed_distance_maps', maps), ('da_boundary_loss_fwd', fwd), ('da_boundary_loss_bwd', bwd)],
                          a.rounds, a.iters)
        present = int(sum(bool((lab == c).any()) for c in CLASSES))
        rows.append(stats_row('distance_transform_edt', iname, shape, times['distance_transform_edt'], 5 * V,
                              {'zero_label': frequent, 'max_distance': finite_max(edt().sqrt()), 'passes_ms': kernel_breakdown(edt)}))
        rows.append(stats_row('signed_distance_maps', iname, shape, times['signed_distance_maps'], (1 + 4 * Kp) * V,
                              {'classes': Kp, 'classes_present': present, 'max_abs_distance': finite_max(phi.abs()),
                               'passes_ms': kernel_breakdown(maps)}))
        print(json.dumps({k: rows[-1 - i]['passes_ms'] for i, k in ((1, 'edt passes'), (0, 'signed maps passes'))}), flush=True)
        rows.append(stats_row('da_boundary_loss_fwd', iname, shape, times['da_boundary_loss_fwd'], 4 * (K + Kp) * V))
        rows.append(stats_row('da_boundary_loss_bwd', iname, shape, times['da_boundary_loss_bwd'], 4 * (2 * K + Kp) * V))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = host_signed_maps(lab, a.host_threads)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        equal = bool(torch.equal(ref, phi))
        assert equal, 'the host route and the device disagree on %s %s' % (iname, shape)
        dev_ms = float(np.median(times['signed_distance_maps']))
        row = {'variant': 'host baseline (D->H, scipy per class on %d threads, H->D)' % a.host_threads, 'input': iname, 'shape': list(shape),
               'ms': round(host_ms, 1), 'equal_to_device': equal, 'baseline_over_device': round(host_ms / dev_ms, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del phi, dz, ref


def bench_step(a, shape, rows):
    import contextlib
    import io
    import tempfile
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    res = {}
    exps = {}
    for key, lam in (('without', None), ('lambda_boundary=1', 1.0)):
        ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                                data_root='./data', log_root=tempfile.mkdtemp(), shape=list(shape), lambda_boundary=lam)
        with contextlib.redirect_stdout(io.StringIO()):
            exp = SegmentationExperiment(train_seg.build_config(ns))
            exp.setup_model(); exp.setup_loss(); exp.setup_train_data(); exp.setup_optimizer()
            exp.initialize_model(exp.model, exp.optimizer, '')
        images, truths, _ = next(iter(exp.training_data_loader))
        exps[key] = (exp, images.to(exp.device), truths.to(exp.device))
        res[key] = []
    for key, (exp, im, tr) in exps.items():
        for _ in range(3):
            exp.train_step(im, tr)
    for _ in range(a.rounds):
        for key, (exp, im, tr) in exps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.step_iters):
                exp.train_step(im, tr)
            torch.cuda.synchronize()
            res[key].append((time.perf_counter() - t0) * 1e3 / a.step_iters)
    med = {k: round(float(np.median(v)), 3) for k, v in res.items()}
    row = {'variant': 'SegmentationExperiment.train_step (UNet_light, batch 1)', 'shape': list(shape), 'ms': med,
           'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in res.items()},
           'boundary_term_cost_ms': round(med['lambda_boundary=1'] - med['without'], 3),
           'note': 'without the key the step takes the route of the parent commit (fused head + Dice), bit for bit'}
    rows.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--step-iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-threads', type=int, default=16)
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_edt.py measures on the GPU'
    assert 1 <= a.host_threads <= 16
    rows = []
    for s in a.shapes:
        shape = tuple(int(v) for v in s.split('x'))
        bench_shape(a, shape, rows)
        bench_step(a, shape, rows)
    out = json.dumps({'bench_edt': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
