#!/usr/bin/env python
"""Timing of the instance refinement (csrc/refine.hip, lib/refine.py refine_field) at 80x96x80 and 160x192x160, N = 1, on a smooth pair, starting
from a smooth 2-voxel field and from the field an untrained voxel_morph_cvpr predicts.  HIP-event timing of warm calls; every variant is timed in
ROUNDS rounds that alternate with the others, and the median with the min - max spread of the rounds is reported.
  * the two new kernels alone, ms per call and the share of the achievable HBM rate (6.3 TB/s) over their compulsory bytes per voxel: moments 20
    (disp 12, fixed 4, moving 4, each once), step 92 (those 20, g_extra 12, disp written 12, m and v read and written 48);
  * time per iteration of refine_field, fused eager / fused graphed / fused=False (the composition through autograd), as
    (time of 60 iterations - time of 10 iterations) / 50, so that what a call pays once (allocations, the table of per-iteration scalars, the
    capture of the graph) drops out;
  * the wall time of one refine_field(iters=50) per route, between two device synchronisations (that includes what a call pays once);
  * 1 - NCC and the folding fraction before and after 50 iterations on the untrained net's field.
python tools/bench_refine.py [--rounds 5] [--shapes 80x96x80 160x192x160] [--out profiles/refine_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from deepatlas_amd import ops
from deepatlas_amd.lib import evalMetrics as metrics
from deepatlas_amd.lib.network_factory import get_network
from deepatlas_amd.lib.refine import refine_field, one_minus_ncc

HBM_RATE = 6.3e12            # bytes / s achievable (float4 copy)
MOMENTS_BYTES, STEP_BYTES = 20, 92


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


def grid(shape):
    D, H, W = shape
    return torch.meshgrid(torch.linspace(-1, 1, D), torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing='ij')


def smooth_volume(shape, dev, shift=0.0):
    D, H, W = shape
    z, y, x = grid(shape)
    x, y = x + shift * torch.sin(2.0 * y), y + shift * torch.cos(1.5 * z)
    v = 0.5 + 0.25 * torch.sin(3.1 * x + 0.4) * torch.cos(2.3 * y) + 0.2 * torch.cos(2.7 * z - 0.3) * torch.sin(1.9 * x * y + 0.2) \
        + 0.3 * torch.exp(-((x - 0.2) ** 2 + (y + 0.3) ** 2 + (z - 0.1) ** 2) / 0.08)
    return v.clamp(0, 1).view(1, 1, D, H, W).contiguous().to(dev)


def smooth_field(shape, dev, amp_vox=2.0):
    D, H, W = shape
    z, y, x = grid(shape)
    u = torch.stack([torch.sin(2.1 * y) * torch.cos(1.3 * z) * 2 / (W - 1), torch.cos(1.7 * x) * torch.sin(0.9 * z + 0.4) * 2 / (H - 1),
                     torch.sin(1.1 * x + 0.8) * torch.cos(2.3 * y) * 2 / (D - 1)], 0) * amp_vox
    return u.unsqueeze(0).contiguous(memory_format=torch.channels_last_3d).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kernel-iters', type=int, default=50)
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_refine.py measures on the GPU'
    dev = torch.device('cuda:0')
    rows = []
    for shape in a.shapes:
        D, H, W = (int(s) for s in shape.split('x'))
        V = D * H * W
        fixed, moving = smooth_volume((D, H, W), dev), smooth_volume((D, H, W), dev, shift=0.04)
        torch.manual_seed(3)
        net = get_network('voxel_morph_cvpr')()
        net.weights_init()
        net.to(dev).eval()
        with torch.no_grad():
            net_field = net(moving, fixed)[0].detach().clone()
        del net
        torch.cuda.empty_cache()
        starts = {'smooth 2-voxel field': smooth_field((D, H, W), dev), "untrained net's field": net_field}
        # ---- the kernels alone
        mv, fx, _, _, _, _ = ops.refine_args(moving, fixed, starts['smooth 2-voxel field'])
        u = ops.ndhwc(starts['smooth 2-voxel field']).clone()
        m, v, gx = torch.zeros_like(u), torch.zeros_like(u), torch.zeros_like(u)
        stats = ops.refine_moments(mv, fx, u)
        state = ops.refine_host_state((0.0, 0.0, 0.0), (0.9, 0.999), 1e-8, 1, float(V), 1.0, 0).to(dev)          # a step of 0: the field stays where it is
        variants = [('da_refine_moments', MOMENTS_BYTES * V, lambda: ops.refine_moments(mv, fx, u, stats), a.kernel_iters),
                    ('da_refine_step (update, g_extra)', STEP_BYTES * V, lambda: ops.refine_step(mv, fx, u, stats, state, g_extra=gx, m=m, v=v, update=True), a.kernel_iters)]
        # ---- refine_field per route and start
        routes = {'fused eager': dict(), 'fused graphed': dict(graph=True), 'composed (fused=False)': dict(fused=False)}
        for sname, d0 in starts.items():
            for rname, kw in routes.items():
                for n in (10, 60):
                    variants.append(('refine_field %d iterations, %s, from the %s' % (n, rname, sname), None,
                                     (lambda d0=d0, kw=kw, n=n: refine_field(moving, fixed, d0, iters=n, **kw)), 1))
        for vv in variants:
            vv[2](); vv[2]()
        torch.cuda.synchronize()
        times = {vv[0]: [] for vv in variants}
        for _ in range(a.rounds):
            for name, _, fn, iters in variants:
                times[name].append(timed(fn, iters))
        for name, nbytes, _, _ in variants[:2]:
            t = np.array(times[name])
            row = {'variant': name, 'shape': [D, H, W], 'N': 1, 'ms': round(float(np.median(t)), 4), 'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4),
                   'bytes': nbytes, 'share_of_hbm_rate': round(nbytes / (float(np.median(t)) * 1e-3) / HBM_RATE, 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        per_iter = {}
        for sname in starts:
            for rname in routes:
                t10 = np.array(times['refine_field 10 iterations, %s, from the %s' % (rname, sname)])
                t60 = np.array(times['refine_field 60 iterations, %s, from the %s' % (rname, sname)])
                t = (t60 - t10) / 50.0
                row = {'variant': 'per iteration, %s, from the %s' % (rname, sname), 'shape': [D, H, W], 'N': 1, 'ms': round(float(np.median(t)), 4),
                       'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4), 'call_of_10_ms': round(float(np.median(t10)), 3),
                       'call_of_60_ms': round(float(np.median(t60)), 3)}
                per_iter[(sname, rname)] = row['ms']
                rows.append(row)
                print(json.dumps(row), flush=True)
        # ---- one call of 50 iterations: wall time, and what it buys on the untrained net's field
        walls = {}
        for rname, kw in routes.items():
            walls[rname] = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = refine_field(moving, fixed, net_field, iters=50, **kw)
                torch.cuda.synchronize()
                walls[rname].append(round((time.perf_counter() - t0) * 1e3, 2))
        out = refine_field(moving, fixed, net_field, iters=50)
        fold = lambda d: float(metrics.jacobian_stats(d)['nonpos_frac'][0])
        sname = "untrained net's field"
        summary = {'variant': 'summary', 'shape': [D, H, W], 'wall_ms_refine_field_50_iterations': walls,
                   'per_iteration_ms': {s + ' / ' + r: per_iter[(s, r)] for s in starts for r in routes},
                   'composed_over_fused_eager': round(per_iter[(sname, 'composed (fused=False)')] / per_iter[(sname, 'fused eager')], 2),
                   'composed_over_fused_graphed': round(per_iter[(sname, 'composed (fused=False)')] / per_iter[(sname, 'fused graphed')], 2),
                   'one_minus_ncc_before': round(float(one_minus_ncc(moving, fixed, net_field)), 5), 'one_minus_ncc_after': round(float(one_minus_ncc(moving, fixed, out)), 5),
                   'folding_fraction_before': fold(net_field), 'folding_fraction_after': fold(out),
                   'settings': 'iters=50, lr_vox=0.1, lambda_sim=1, lambda_reg=1, grad_scale=V'}
        rows.append(summary)
        print(json.dumps(summary), flush=True)
        del starts, net_field, u, m, v, gx
        torch.cuda.empty_cache()
    out = json.dumps({'bench_refine': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
