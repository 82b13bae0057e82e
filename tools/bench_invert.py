#!/usr/bin/env python
"""Timing of the field inversion (csrc/fieldinv.hip da_field_invert) at 80x96x80 and 160x192x160, N = 1, on a smooth field
(tests/regeval_cases.py's generator) scaled to a Lipschitz bound of 0.25 / 0.5 / 0.8 (tests/invert_cases.py lipschitz_bound) and on the field
an untrained VoxelMorph predicts for a random image pair.  HIP-event timing of warm back-to-back calls of the C entry on preallocated buffers
(_native.call, no statistics); every variant is timed in ROUNDS rounds that alternate with the others, and the median with the min - max
spread of the rounds is reported.  Per field: the kernel with tol_vox = 1e-3 (the interface default: voxels stop on their own) and with
tol_vox = 0, max_iters = 32 (every update runs), the mean number of updates per voxel of each (from the entry's statistics, a call of its
own), the rate over the COMPULSORY bytes -- 12 per voxel read of the field, 12 written = 24 V -- as a share of the achievable HBM rate
(6.3 TB/s), and the only route without the kernel: 32 iterations of (grid add + F.grid_sample(border) + negate) in float32 torch on the device,
with its distance from the kernel's result in voxels.
python tools/bench_invert.py [--iters 20] [--rounds 5] [--shapes 80x96x80 160x192x160] [--out profiles/invert_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from deepatlas_amd import _native as nat
from deepatlas_amd import ops

HBM_ACHIEVABLE = 6.3e12      # bytes / s
MAX_ITERS = 32


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


def alternate(variants, rounds):
    """{name: [ms per round]} with the variants (name, fn, iters) alternating."""
    for _, fn, _ in variants:               # warm every shape (code objects, allocator)
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, fn, iters in variants:
            times[name].append(timed(fn, iters))
    return times


def lipschitz_bound(u):
    """tests/invert_cases.py lipschitz_bound, on the tensor's device"""
    D, H, W = u.shape[2:]
    s = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], dtype=torch.float64, device=u.device).view(1, 3, 1, 1, 1)
    g = u.double() * s
    steps = [g[:, :, 1:] - g[:, :, :-1], g[:, :, :, 1:] - g[:, :, :, :-1], g[..., 1:] - g[..., :-1]]
    return max(float(t.pow(2).sum(1).sqrt().max()) for t in steps) * 3.0 ** 0.5


def identity(shape, dev):
    D, H, W = shape
    ax = [torch.arange(n, dtype=torch.float32, device=dev) / (n - 1) * 2.0 - 1 for n in (D, H, W)]
    return torch.stack(torch.meshgrid(*ax, indexing='ij')[::-1]).unsqueeze(0)


def composed(u, ident, iters=MAX_ITERS):
    """The definition from existing torch ops: what a user without the kernel would run on the device."""
    v = torch.zeros_like(u)
    for _ in range(iters):
        v = -torch.nn.functional.grid_sample(u, (ident + v).permute(0, 2, 3, 4, 1), mode='bilinear', padding_mode='border', align_corners=True)
    return v


def untrained_field(shape, dev):
    from deepatlas_amd.lib.network_factory import get_network
    ops.set_matrix_precision(ops.DEFAULT_MATRIX_PRECISION)
    torch.manual_seed(0)
    reg = get_network('voxel_morph_cvpr')().to(dev).eval()
    g = torch.Generator().manual_seed(11)
    im_m = torch.rand((1, 1) + tuple(shape), generator=g).to(dev)
    im_t = torch.rand((1, 1) + tuple(shape), generator=g).to(dev)
    with torch.no_grad():
        u = reg(im_m, im_t)[0].clone()
    del reg
    torch.cuda.empty_cache()
    return u


def bench_shape(a, shape, rows):
    import regeval_cases as rc
    dev = torch.device('cuda:0')
    D, H, W = shape
    V = D * H * W
    L = nat.lib()
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last_3d)      # the layout the registration net hands out (no copy in ndhwc)
    smooth = rc.smooth_field(shape, 1, 1.0, seed=3).to(dev)
    fields = [('smooth, Lipschitz %g' % lip, cl((smooth.double() * (lip / lipschitz_bound(smooth))).float())) for lip in (0.25, 0.5, 0.8)]
    fields.append(('untrained net', cl(untrained_field(shape, dev))))
    ident = identity(shape, dev)
    sc = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], device=dev).view(1, 3, 1, 1, 1)
    for fname, du in fields:
        u = ops.ndhwc(du)
        out = torch.empty_like(u)
        ws = torch.empty(L.da_field_invert_ws_bytes(1, D, H, W) + 256, dtype=torch.uint8, device=dev)
        st = nat.stream()

        def kernel(tol):
            nat.call('da_field_invert', nat.ptr(u), nat.ptr(out), None, 1, D, H, W, MAX_ITERS, tol, None, None, 0, st)

        info = {}
        for key, tol in (('tol 1e-3', 1e-3), ('tol 0', 0.0)):
            _, stats = ops.invert_field(du, max_iters=MAX_ITERS, tol_vox=tol, return_stats=True)
            s = stats[0].cpu().numpy()
            info[key] = {'mean_iters': round(float(s[2]) / V, 3), 'max_update_vox': float(s[0]), 'unconverged_frac': float(s[1]) / V, 'outside_frac': float(s[3]) / V}
        with torch.no_grad():
            dist = float(((ops.invert_field(du, max_iters=MAX_ITERS, tol_vox=0.0) - composed(du, ident)) * sc).abs().max())
        variants = [('kernel, tol_vox 1e-3', lambda: kernel(1e-3), a.iters), ('kernel, tol_vox 0, 32 updates', lambda: kernel(0.0), a.iters),
                    ('torch composition, 32 iterations', lambda: composed(du, ident), max(a.iters // 4, 3))]
        with torch.no_grad():
            times = alternate(variants, a.rounds)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for (name, _, _), key in zip(variants, ('tol 1e-3', 'tol 0', None)):
            t = np.array(times[name])
            row = {'variant': name, 'field': fname, 'lipschitz_bound': round(lipschitz_bound(du), 4), 'shape': [D, H, W], 'N': 1, 'ms': round(med[name], 4),
                   'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4)}
            line = '%-34s %-22s %-12s %9.4f ms (%.4f - %.4f)' % (name, fname, 'x'.join(map(str, shape)), row['ms'], row['ms_min'], row['ms_max'])
            if key:
                rate = 24.0 * V / (med[name] * 1e-3)
                row.update(info[key], compulsory_bytes=24 * V, GBps_compulsory=round(rate / 1e9, 1), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 4))
                line += '  %5.2f updates / voxel  %7.1f GB/s  %.3f of 6.3 TB/s' % (row['mean_iters'], row['GBps_compulsory'], row['share_of_achievable_hbm'])
            rows.append(row)
            print(line, flush=True)
        summary = {'variant': 'summary', 'field': fname, 'shape': [D, H, W],
                   'composition_over_kernel_tol_1e-3': round(med[variants[2][0]] / med[variants[0][0]], 1),
                   'composition_over_kernel_32_updates': round(med[variants[2][0]] / med[variants[1][0]], 1),
                   'kernel_32_updates_vs_composition_max_vox': dist}
        rows.append(summary)
        print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_invert.py measures on the GPU'
    rows = []
    for s in a.shapes:
        bench_shape(a, tuple(int(v) for v in s.split('x')), rows)
    out = json.dumps({'bench_invert': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
