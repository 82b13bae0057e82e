#!/usr/bin/env python
"""Timing of the native-grid registration route (csrc/regapply.hip) on one GPU, N = 1: moving 160x384x384 int16 -> fixed 160x384x384 through a
160x192x192 prepared grid (frames a = (1, 2, 2), b = 0), on a smooth 2-voxel field and on the field an untrained VoxelMorph predicts.
HIP-event timing of warm back-to-back calls on preallocated inputs; every variant is timed in ROUNDS rounds of ITERS calls that alternate
with the others; the median round with the min - max spread is reported.
  prefilter   the W pass from int16 (mask 1), the H and D passes (masks 2, 4: each call also runs the converting copy, timed alone as mask 0
              and subtracted in `ms_pass`), and the full prefilter
  warp        orders 0, 1 and 3 (order 3 on coefficients prefiltered beforehand; `order 3 + prefilter` is the whole call)
  (a)         the three-interpolation composition of existing ops, linear only: resample_volume onto the prepared grid, WarpFn, resample_volume
              onto the fixed grid
  (b)         the host route, once per field: device -> host of the moving volume and the sample positions, scipy spline_filter +
              map_coordinates(order 3, mirror) over 16 threads, host -> device of the result (wall clock)
Rates: compulsory bytes (stated per row: every input read once, every output written once) over the time, as a share of the achievable HBM
rate (6.3 TB/s).  Accuracy, on tests/regapply_cases.py's band-limited analytic image and known field: the largest distance of each route from
the analytic values and from the float64 reference, over the voxels at least 4 voxels inside the moving grid.
python tools/bench_regapply.py [--iters 50] [--rounds 5] [--out profiles/regapply_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from deepatlas_amd import ops

HBM_ACHIEVABLE = 6.3e12      # bytes / s
MOVING = FIXED = (160, 384, 384)
PREPARED = (160, 192, 192)
FRAME = ((1.0, 0.0), (2.0, 0.0), (2.0, 0.0))
HOST_THREADS = 16


def timed(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, rounds):
    for _, fn, _, _ in variants:               # warm every shape (code objects, allocator)
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in variants}
    for _ in range(rounds):
        for name, fn, iters, _ in variants:
            times[name].append(timed(fn, iters))
    return times


def smooth_field(size, amp_vox, dev):
    z, y, x = torch.meshgrid(*[torch.linspace(0, 1, n, device=dev) for n in size], indexing='ij')
    vox = [amp_vox * torch.sin(2 * np.pi * z + 0.3) * torch.cos(2 * np.pi * y), amp_vox * torch.cos(np.pi * x + 0.2) * torch.sin(2 * np.pi * y),
           amp_vox * torch.sin(2 * np.pi * x) * torch.cos(np.pi * z)]
    return torch.stack([vox[ch] / ((size[2 - ch] - 1) / 2.0) for ch in range(3)])[None].contiguous()


def untrained_field(shape, dev):
    from deepatlas_amd.lib.network_factory import get_network
    ops.set_matrix_precision(ops.DEFAULT_MATRIX_PRECISION)
    torch.manual_seed(0)
    reg = get_network('voxel_morph_cvpr')().to(dev).eval()
    g = torch.Generator().manual_seed(11)
    im_m, im_t = (torch.rand((1, 1) + tuple(shape), generator=g).to(dev) for _ in range(2))
    with torch.no_grad():
        u = reg(im_m, im_t)[0].clone()
    del reg
    torch.cuda.empty_cache()
    return u


def composition(moving, disp, inv_scale):
    """(a): three interpolations, all linear."""
    prepared = ops.resample_volume(moving, PREPARED, FRAME_SCALE, (0.0, 0.0, 0.0), 'linear', 0)
    warped = ops.WarpFn.apply(prepared[None, None], disp)[0][0, 0]
    return ops.resample_volume(warped, FIXED, inv_scale, (0.0, 0.0, 0.0), 'linear', 0)


FRAME_SCALE = tuple(f[0] for f in FRAME)


def positions(disp, out_size, ff, mf):
    """y (3, Do, Ho, Wo) float32 on the device, torch ops: the host route's coordinates."""
    dev = disp.device
    x = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=dev) for n in out_size], indexing='ij')
    p = [(x[a] - ff[a][1]) / ff[a][0] for a in range(3)]
    size = disp.shape[2:]
    g = torch.stack([p[2] / (size[2] - 1) * 2 - 1, p[1] / (size[1] - 1) * 2 - 1, p[0] / (size[0] - 1) * 2 - 1], -1)[None]
    u = torch.nn.functional.grid_sample(disp, g, mode='bilinear', padding_mode='border', align_corners=True)[0]
    return torch.stack([mf[a][0] * (p[a] + u[2 - a] * ((size[a] - 1) / 2.0)) + mf[a][1] for a in range(3)])


def host_route(moving, y):
    """(b): (result on the device, seconds)."""
    from concurrent.futures import ThreadPoolExecutor
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    src = moving.cpu().numpy().astype(np.float32)
    coords = y.cpu().numpy()
    coef = ndimage.spline_filter(src, 3, output=np.float32, mode='mirror')
    out = np.empty(coords.shape[1:], dtype=np.float32)
    slabs = np.array_split(np.arange(coords.shape[1]), HOST_THREADS)

    def work(rows):
        if len(rows):
            out[rows[0]:rows[-1] + 1] = ndimage.map_coordinates(coef, coords[:, rows[0]:rows[-1] + 1], order=3, mode='mirror', prefilter=False)
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        list(pool.map(work, slabs))
    res = torch.from_numpy(out).to(moving.device)
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def row_of(name, times, nbytes, note, extra=None):
    t = np.array(times)
    med = float(np.median(t))
    row = {'variant': name, 'ms': round(med, 4), 'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4), 'compulsory_bytes': int(nbytes),
           'compulsory': note, 'GBps_compulsory': round(nbytes / (med * 1e-3) / 1e9, 1), 'share_of_achievable_hbm': round(nbytes / (med * 1e-3) / HBM_ACHIEVABLE, 4)}
    row.update(extra or {})
    print('%-44s %9.4f ms (%.4f - %.4f)  %7.1f GB/s  %.3f of 6.3 TB/s' % (name, row['ms'], row['ms_min'], row['ms_max'], row['GBps_compulsory'],
                                                                          row['share_of_achievable_hbm']), flush=True)
    return row


def bench_speed(a, rows):
    dev = torch.device('cuda:0')
    V, Vp = int(np.prod(FIXED)), int(np.prod(PREPARED))
    g = torch.Generator().manual_seed(5)
    moving = (torch.rand(MOVING, generator=g) * 3000).to(torch.int16).to(dev)
    as_f32 = moving.float()
    coef = ops.bspline_prefilter(moving)
    inv_scale = tuple(1.0 / s for s in FRAME_SCALE)
    # prefilter, once: it does not depend on the field
    pre = [('prefilter W pass (int16 in)', lambda: ops.bspline_prefilter(moving, axes=(2,)), a.iters, (6 * V, 'int16 read + float32 written')),
           ('prefilter copy alone (float32 in, mask 0)', lambda: ops.bspline_prefilter(as_f32, axes=()), a.iters, (8 * V, 'float32 read + written')),
           ('prefilter copy + H pass (float32 in)', lambda: ops.bspline_prefilter(as_f32, axes=(1,)), a.iters, (16 * V, 'copy 8 V + the pass 8 V')),
           ('prefilter copy + D pass (float32 in)', lambda: ops.bspline_prefilter(as_f32, axes=(0,)), a.iters, (16 * V, 'copy 8 V + the pass 8 V')),
           ('prefilter, all three passes (int16 in)', lambda: ops.bspline_prefilter(moving), a.iters, (22 * V, '6 V + 8 V + 8 V: each pass reads and writes once'))]
    times = alternate(pre, a.rounds)
    copy_ms = float(np.median(times[pre[1][0]]))
    for name, _, _, (nbytes, note) in pre:
        extra = {'ms_pass': round(float(np.median(times[name])) - copy_ms, 4)} if 'copy +' in name else None
        rows.append(row_of(name, times[name], nbytes, note, extra))
    for fname, disp in (('smooth, 2 voxels', smooth_field(PREPARED, 2.0, dev)), ('untrained net', untrained_field(PREPARED, dev))):
        warp = lambda order, src, **kw: ops.warp_to_grid(src, disp, FIXED, FRAME, FRAME, order=order, **kw)
        variants = [('warp order 0 (int16)', lambda: warp(0, moving), a.iters, (4 * V + 12 * Vp, 'int16 read + written, the field read')),
                    ('warp order 1 (int16 -> float32)', lambda: warp(1, moving), a.iters, (6 * V + 12 * Vp, 'int16 read, float32 written, the field read')),
                    ('warp order 3 (prefiltered)', lambda: warp(3, coef, prefiltered=True), a.iters, (8 * V + 12 * Vp, 'coefficients read, float32 written, the field read')),
                    ('warp order 3 + prefilter (int16 in)', lambda: warp(3, moving), a.iters, (30 * V + 12 * Vp, 'the prefilter 22 V + the warp 8 V + the field')),
                    ('(a) composition: resample, WarpFn, resample', lambda: composition(moving, disp, inv_scale), a.iters,
                     (2 * V + 4 * Vp + 8 * Vp + 12 * Vp + 4 * Vp + 4 * V, 'each of the three ops reads its inputs and writes its output once'))]
        with torch.no_grad():
            times = alternate(variants, a.rounds)
            y = positions(disp, FIXED, FRAME, FRAME)
            host, seconds = host_route(moving, y)
            got = warp(3, coef, prefiltered=True)
        for name, _, _, (nbytes, note) in variants:
            rows.append(dict(row_of(name, times[name], nbytes, note), field=fname))
        # compared where the position is inside by more than the tests' guard band (1e-3 voxel): at the edge the two routes' float32 positions decide differently
        inside = torch.stack([(y[k] >= -0.5 + 1e-3) & (y[k] < MOVING[k] - 0.5 - 1e-3) for k in range(3)]).all(0)
        rows.append({'variant': '(b) host route: D->H, scipy order 3 on %d threads, H->D' % HOST_THREADS, 'field': fname, 'ms': round(seconds * 1e3, 1), 'calls': 1,
                     'kernel_vs_host_max_abs_inside': float((got - host)[inside].abs().max()), 'inside_frac': float(inside.float().mean()),
                     'largest_displacement_vox': float((disp.abs() * torch.tensor([(PREPARED[2 - c] - 1) / 2.0 for c in range(3)], device=dev).view(1, 3, 1, 1, 1)).max()),
                     'source_max': 3000})
        print(json.dumps(rows[-1]), flush=True)
        del y, host, got
        torch.cuda.empty_cache()


def bench_accuracy(rows):
    import regapply_cases as rc
    dev = torch.device('cuda:0')
    c = rc.ANALYTIC
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in c['moving']], indexing='ij'))
    src = rc.analytic_image(grid)[None].astype(np.float32)
    disp = rc.analytic_field()
    d_src, d_disp = torch.from_numpy(src[0]).to(dev), torch.from_numpy(disp)[None].to(dev)
    ref = {}
    for order in (1, 3):
        s = rc.prefilter_ref64(src) if order == 3 else src
        ref[order], y, inside, _ = rc.warp_reference(s, disp, c['fixed'], c['fixed_frame'], c['moving_frame'], order, default=0)
    core = inside & np.all([(y[k] >= 4) & (y[k] <= c['moving'][k] - 5) for k in range(3)], axis=0)
    truth = rc.analytic_image(y)
    routes = {'kernel order 1': ops.warp_to_grid(d_src, d_disp, c['fixed'], c['fixed_frame'], c['moving_frame'], order=1).cpu().numpy(),
              'kernel order 3': ops.warp_to_grid(d_src, d_disp, c['fixed'], c['fixed_frame'], c['moving_frame'], order=3).cpu().numpy(),
              'float64 reference order 1': ref[1][0], 'float64 reference order 3': ref[3][0]}
    # (a) on these frames: onto the prepared grid (prepared index p reads native a_m p + b_m), WarpFn, onto the fixed grid (x reads p = (x - b_f) / a_f)
    with torch.no_grad():
        prepared = ops.resample_volume(d_src, c['prepared'], tuple(f[0] for f in c['moving_frame']), tuple(f[1] for f in c['moving_frame']), 'linear', 0)
        warped = ops.WarpFn.apply(prepared[None, None], d_disp)[0][0, 0]
        routes['(a) composition, linear x 3'] = ops.resample_volume(warped, c['fixed'], tuple(1.0 / f[0] for f in c['fixed_frame']),
                                                                   tuple(-f[1] / f[0] for f in c['fixed_frame']), 'linear', 0).cpu().numpy()
        routes['(b) host route, order 3'] = host_route(d_src, positions(d_disp, c['fixed'], c['fixed_frame'], c['moving_frame']))[0].cpu().numpy()
    for name, out in routes.items():
        order = 1 if ('order 1' in name or 'linear' in name) else 3
        row = {'variant': 'accuracy: ' + name, 'image': 'sum of 4 sinusoids, amplitude 400, <= 0.15 cycles / voxel', 'moving': list(c['moving']), 'fixed': list(c['fixed']),
               'max_abs_from_analytic': float(np.max(np.abs(out - truth)[core])), 'max_abs_from_float64_reference_order_%d' % order: float(np.max(np.abs(out - ref[order][0])[core]))}
        rows.append(row)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_regapply.py measures on the GPU'
    rows = []
    bench_accuracy(rows)
    bench_speed(a, rows)
    out = json.dumps({'bench_regapply': rows, 'moving': list(MOVING), 'prepared': list(PREPARED), 'fixed': list(FIXED), 'iters': a.iters, 'rounds': a.rounds})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
