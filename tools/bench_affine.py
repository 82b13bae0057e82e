#!/usr/bin/env python
"""Timing of the affine pre-alignment kernels (csrc/affine.hip da_affine_warp_fwd / da_affine_warp_bwd_theta) at 80x96x80 and 160x192x160,
N = 1, C = 1, under a rigid theta of 5 degrees / 3 voxels on a smooth volume.  HIP-event timing of warm back-to-back calls; every variant is
timed in ROUNDS rounds that alternate with the others, and the median with the min - max spread of the rounds is reported.  Per kernel: ms
per call and the share of the achievable HBM rate (6.3 TB/s) over the compulsory bytes -- forward 8 per voxel (src read once, out written),
d_theta 8 per voxel (g and src read once; the twelve sums are negligible).  Beside them the only route without the kernels, the torch
composition on the device: F.affine_grid + F.grid_sample forward, and forward + backward to theta through autograd (which materialises the
V x 3 grid and its gradient).  Last, the wall time of one default affine_register (rigid, NCC, levels 4 / 2 / 1, 60 / 40 / 20 iterations)
on a pair misaligned by that theta, between two device synchronisations, and the corner error it leaves.
python tools/bench_affine.py [--iters 50] [--rounds 5] [--shapes 80x96x80 160x192x160] [--out profiles/affine_bench.json]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
from deepatlas_amd import ops
from deepatlas_amd import _native as nat
from deepatlas_amd.lib import affine as A

HBM_RATE = 6.3e12            # bytes / s achievable (float4 copy)


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


def smooth_volume(shape, dev):
    D, H, W = shape
    z, y, x = torch.meshgrid(torch.linspace(-1, 1, D), torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing='ij')
    v = 0.5 + 0.25 * torch.sin(3.1 * x + 0.4) * torch.cos(2.3 * y) + 0.2 * torch.cos(2.7 * z - 0.3) * torch.sin(1.9 * x * y + 0.2) \
        + 0.3 * torch.exp(-((x - 0.2) ** 2 + (y + 0.3) ** 2 + (z - 0.1) ** 2) / 0.08)
    return v.clamp(0, 1).view(1, 1, D, H, W).contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_affine.py measures on the GPU'
    dev = torch.device('cuda:0')
    rows = []
    for shape in a.shapes:
        D, H, W = (int(s) for s in shape.split('x'))
        V = D * H * W
        src = smooth_volume((D, H, W), dev)
        theta = A.rigid_theta(torch.tensor([[5.0, -3.0, 4.0]], dtype=torch.float64) * math.pi / 180, torch.tensor([[3.0, -2.0, 1.5]], dtype=torch.float64),
                              (D, H, W)).float().to(dev).contiguous()
        g = torch.randn((1, 1, D, H, W), generator=torch.Generator().manual_seed(3)).to(dev)
        s_, g_ = ops.ndhwc(src), ops.ndhwc(g)
        out = torch.empty_like(s_)
        d_theta = torch.empty_like(theta)
        wp, wn = nat.workspace.get(nat.lib().da_affine_warp_ws_bytes(1, D, H, W), dev)

        def k_fwd():
            nat.call('da_affine_warp_fwd', nat.ptr(s_), nat.ptr(theta), nat.ptr(out), 1, D, H, W, 1, nat.stream())

        def k_bwd():
            nat.call('da_affine_warp_bwd_theta', nat.ptr(g_), nat.ptr(s_), nat.ptr(theta), nat.ptr(d_theta), 1, D, H, W, 1, wp, wn, nat.stream())

        thg = theta.clone().requires_grad_(True)

        def t_fwd():
            with torch.no_grad():
                return F.grid_sample(src, F.affine_grid(theta, list(src.shape), align_corners=True), mode='bilinear', padding_mode='zeros', align_corners=True)

        def t_fwd_bwd():
            o = F.grid_sample(src, F.affine_grid(thg, list(src.shape), align_corners=True), mode='bilinear', padding_mode='zeros', align_corners=True)
            return torch.autograd.grad(o, thg, g)

        def a_fwd_bwd():
            return torch.autograd.grad(ops.AffineWarpFn.apply(src, thg), thg, g)

        # the routes compute the same thing: each against torch float64 on the device
        th64 = theta.double().requires_grad_(True)
        o64 = F.grid_sample(src.double(), F.affine_grid(th64, list(src.shape), align_corners=True), mode='bilinear', padding_mode='zeros', align_corners=True)
        g64 = torch.autograd.grad(o64, th64, g.double())[0]
        k_fwd(); k_bwd()
        rel = lambda got, want: float((got.double() - want).abs().max() / want.abs().max())
        agree = dict(kernels=dict(out=rel(ops.ncdhw(out), o64.detach()), d_theta=rel(d_theta, g64)),
                     torch_float32=dict(out=rel(t_fwd(), o64.detach()), d_theta=rel(t_fwd_bwd()[0], g64)))
        del o64, th64
        torch.cuda.empty_cache()
        variants = [
            ('affine warp forward (da_affine_warp_fwd)', 8 * V, k_fwd, a.iters),
            ('affine warp d_theta (da_affine_warp_bwd_theta)', 8 * V, k_bwd, a.iters),
            ('fused forward + d_theta through autograd', None, a_fwd_bwd, a.iters),
            ('torch affine_grid + grid_sample forward', None, t_fwd, max(a.iters // 2, 3)),
            ('torch affine_grid + grid_sample forward + backward to theta', None, t_fwd_bwd, max(a.iters // 2, 3)),
        ]
        for v in variants:
            v[2](); v[2]()
        torch.cuda.synchronize()
        times = {v[0]: [] for v in variants}
        for _ in range(a.rounds):
            for name, _, fn, iters in variants:
                times[name].append(timed(fn, iters))
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name, nbytes, _, _ in variants:
            t = np.array(times[name])
            row = {'variant': name, 'shape': [D, H, W], 'N': 1, 'ms': round(med[name], 4), 'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4)}
            line = '%-62s %-12s %9.4f ms (%.4f - %.4f)' % (name, shape, row['ms'], row['ms_min'], row['ms_max'])
            if nbytes is not None:
                row.update(bytes=nbytes, share_of_hbm_rate=round(nbytes / (med[name] * 1e-3) / HBM_RATE, 4))
                line += '  %.1f MB, %.3f of the achievable HBM rate' % (nbytes / 1e6, row['share_of_hbm_rate'])
            rows.append(row)
            print(line, flush=True)
        # one default registration: the moving image is the volume under theta, the aligning map its inverse
        with torch.no_grad():
            moving = ops.AffineWarpFn.apply(src, theta).contiguous()
        A.affine_register(moving, src, iters=(2, 2, 2))                  # warm: code objects, the workspace, the optimiser's kernels
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            est = A.affine_register(moving, src)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        want = A.invert_theta(theta)
        k_pair = med[variants[0][0]] + med[variants[1][0]]
        t_pair = med[variants[4][0]]
        summary = {'variant': 'summary', 'shape': [D, H, W], 'kernel_forward_plus_d_theta_ms': round(k_pair, 4),
                   'torch_forward_plus_backward_ms': round(t_pair, 4), 'torch_over_kernels': round(t_pair / k_pair, 2),
                   'torch_forward_over_kernel_forward': round(med[variants[3][0]] / med[variants[0][0]], 2),
                   'distance_from_float64': agree,
                   'default_affine_register_wall_ms': [round(w, 1) for w in walls], 'iterations': list(A.pyramid_levels((D, H, W), A.DEFAULT_LEVELS, A.DEFAULT_ITERS)),
                   'corner_error_vox_before': round(float(A.corner_error_vox(A.identity_theta(1).to(dev), want, (D, H, W))), 3),
                   'corner_error_vox_after': round(float(A.corner_error_vox(est, want, (D, H, W))), 3)}
        rows.append(summary)
        print(json.dumps(summary), flush=True)
    out = json.dumps({'bench_affine': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
