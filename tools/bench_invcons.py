#!/usr/bin/env python
"""Timing of the inverse-consistency penalty (csrc/invcons.hip da_invcons_fwd / da_invcons_bwd) at 80x96x80 and 160x192x160, N = 1, one
direction, on a smooth pair (tests/regeval_cases.py's generator, 2 voxels of standard deviation) and on the pair of fields an untrained
VoxelMorph predicts for the two directions of one image pair.  HIP-event timing of warm back-to-back calls; every variant is timed in ROUNDS
rounds that alternate with the others, and the median with the min - max spread of the rounds is reported.  The kernel rows time the C entries
themselves on preallocated buffers (_native.call; the backward rows include the zero-fill of d_disp_b the entry asks of its caller); the
'through autograd' row adds the host cost of torch.autograd.  Per row: ms per call and the rate over the COMPULSORY bytes as a share of the
achievable HBM rate (6.3 TB/s) -- forward 12 per voxel read of u_a + 12 of u_b (every voxel of u_b is sampled by a smooth map about once) +
12 for the saved residual = 36; backward 12 + 12 + 12 read and 12 written by the gather of d_disp_a = 48, and for d_disp_b (a kernel of its own, one lane per
element, reading u_a and the residual again) the 12 of the zero-fill beside the 8 x 12 bytes of atomic adds = 60 + 96 atomic.  The scatter's own rate is stated as added bytes per second: 8 taps x 12 bytes per voxel whose
sample point is inside, over the time the backward with d_disp_b takes beyond the backward without it.  Beside them the deterministic route
(the fixed-point accumulation of da_warp_bwd_dsrc_det on the stored g) and the only route without the kernels: the composition from existing
ops (ops.WarpFn on the 3-channel field + torch elementwise + autograd).  Then the whole RegistrationStep (VoxelMorph, NCC + bending energy,
FlatAdam) with lam_ic = 1 (the doubled batch and the penalty) against lam_ic = 0 (the step without it bit for bit,
tests/test_gpu_invcons.py) and against the step on a doubled batch without the penalty: what of the difference is the loss itself.
python tools/bench_invcons.py [--iters 20] [--rounds 5] [--shapes 80x96x80 160x192x160] [--no-step] [--out profiles/invcons_bench.json]"""
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


def composed(u_a, u_b):
    """L(u_a, u_b) from existing ops: what a user without the kernels would run on the device."""
    D, H, W = u_a.shape[2:]
    s = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], device=u_a.device).view(1, 3, 1, 1, 1)
    sr = (u_a + ops.WarpFn.apply(u_b, u_a)[0]) * s
    return (sr * sr).sum(1).mean()


def untrained_pair(shape, dev):
    """The two directions' fields of an untrained VoxelMorph on one random image pair."""
    from deepatlas_amd.lib.network_factory import get_network
    ops.set_matrix_precision(ops.DEFAULT_MATRIX_PRECISION)
    torch.manual_seed(0)
    reg = get_network('voxel_morph_cvpr')().to(dev).eval()
    g = torch.Generator().manual_seed(11)
    im_m = torch.rand((1, 1) + tuple(shape), generator=g).to(dev)
    im_t = torch.rand((1, 1) + tuple(shape), generator=g).to(dev)
    with torch.no_grad():
        pair = reg(im_m, im_t)[0].clone(), reg(im_t, im_m)[0].clone()
    del reg
    torch.cuda.empty_cache()
    return pair


def bench_kernels(a, shape, rows):
    import regeval_cases as rc
    dev = torch.device('cuda:0')
    D, H, W = shape
    V = D * H * W
    L = nat.lib()
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last_3d)      # the layout the registration net hands out (no copy in ndhwc)
    pairs = [('smooth 2 voxels', cl(rc.smooth_field(shape, 1, 2.0, seed=3)), cl(rc.smooth_field(shape, 1, 2.0, seed=4)))]
    pairs.append(('untrained net',) + tuple(cl(t) for t in untrained_pair(shape, dev)))
    for fname, da, db in pairs:
        s = {k: float(v[0]) for k, v in ops.inverse_consistency_stats(da, db).items()}
        inside = 1.0 - s['outside_frac']
        ua, ub = ops.ndhwc(da), ops.ndhwc(db)
        loss, gl, resid = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty_like(ua)
        d_a, d_b = torch.empty_like(ua), torch.empty_like(ub)
        ws = torch.empty(max(L.da_invcons_ws_bytes(1, D, H, W), L.da_warp_bwd_dsrc_det_ws_bytes(1, D, H, W, 3)) + 256, dtype=torch.uint8, device=dev)
        st = nat.stream()

        def k_fwd():
            nat.call('da_invcons_fwd', nat.ptr(ua), nat.ptr(ub), 1, D, H, W, nat.ptr(loss), None, nat.ptr(resid), nat.ptr(ws), ws.numel(), st)

        def k_bwd(want_a=True, want_b=True, det=0):
            if want_b and not det:
                d_b.zero_()
            nat.call('da_invcons_bwd', nat.ptr(ua), nat.ptr(ub), nat.ptr(resid), nat.ptr(gl), nat.ptr(d_a) if want_a else None,
                     nat.ptr(d_b) if want_b else None, 1, D, H, W, det, nat.ptr(ws), ws.numel(), st)

        def through_autograd():
            x, y = da.detach().requires_grad_(True), db.detach().requires_grad_(True)
            ops.InverseConsistencyFn.apply(x, y).backward()
            return x.grad, y.grad

        def t_fwd():
            with torch.no_grad():
                return composed(da, db)

        def t_both():
            x, y = da.detach().requires_grad_(True), db.detach().requires_grad_(True)
            composed(x, y).backward()
            return x.grad, y.grad

        k_fwd()
        variants = [
            ('forward (da_invcons_fwd)', k_fwd, a.iters),
            ('backward, both gradients (da_invcons_bwd, atomics)', k_bwd, a.iters),
            ('backward, d_disp_a only (the gather)', lambda: k_bwd(True, False), a.iters),
            ('backward, d_disp_b only (the scatter)', lambda: k_bwd(False, True), a.iters),
            ('backward, both gradients, deterministic', lambda: k_bwd(True, True, 1), max(a.iters // 2, 3)),
            ('composition from existing ops, forward', t_fwd, max(a.iters // 4, 3)),
            ('composition from existing ops, forward + backward', t_both, max(a.iters // 4, 3)),
            ('forward + backward through autograd', through_autograd, a.iters),
        ]
        nbytes = {variants[0][0]: 36 * V, variants[1][0]: 60 * V, variants[2][0]: 48 * V, variants[3][0]: 48 * V}
        # the two routes compute the same thing: each against the float64 evaluation of the formula on the device
        x64, y64 = da.double().requires_grad_(True), db.double().requires_grad_(True)
        p = x64 + torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64, device=dev) / (n - 1) * 2 - 1 for n in (D, H, W)], indexing='ij')[::-1]).unsqueeze(0)
        sc = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], dtype=torch.float64, device=dev).view(1, 3, 1, 1, 1)
        sr = (x64 + torch.nn.functional.grid_sample(y64, p.permute(0, 2, 3, 4, 1), mode='bilinear', padding_mode='zeros', align_corners=True)) * sc
        l64 = (sr * sr).sum(1).mean()
        ga64, gb64 = torch.autograd.grad(l64, (x64, y64))
        l64 = float(l64.detach())

        def distance(route):
            x, y = da.detach().requires_grad_(True), db.detach().requires_grad_(True)
            l = route(x, y)
            l.backward()
            return {'loss_rel': abs(float(l.detach()) - l64) / abs(l64), 'd_a_rel': float((x.grad.double() - ga64).abs().max() / ga64.abs().max()),
                    'd_b_rel': float((y.grad.double() - gb64).abs().max() / gb64.abs().max())}
        agree = dict(kernels=distance(ops.InverseConsistencyFn.apply), composition_float32=distance(composed))
        del x64, y64, p, sr, ga64, gb64
        torch.cuda.empty_cache()
        times = alternate(variants, a.rounds)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name, _, _ in variants:
            t = np.array(times[name])
            row = {'variant': name, 'field': fname, 'mean_residual_vox': round(s['mean_vox'], 4), 'outside_frac': round(s['outside_frac'], 6), 'shape': [D, H, W],
                   'N': 1, 'ms': round(med[name], 4), 'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4)}
            line = '%-52s %-16s %-12s %9.4f ms (%.4f - %.4f)' % (name, fname, 'x'.join(map(str, shape)), row['ms'], row['ms_min'], row['ms_max'])
            if name in nbytes:
                rate = nbytes[name] / (med[name] * 1e-3)
                row.update(compulsory_bytes=nbytes[name], GBps_compulsory=round(rate / 1e9, 1), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 4))
                line += '  %7.1f GB/s  %.3f of 6.3 TB/s' % (row['GBps_compulsory'], row['share_of_achievable_hbm'])
            rows.append(row)
            print(line, flush=True)
        pair = med[variants[0][0]] + med[variants[1][0]]
        atomic_bytes = 8 * 12 * V * inside              # (an upper count: a sample point inside still has taps outside next to the faces)
        scatter_ms = med[variants[1][0]] - med[variants[2][0]]
        summary = {'variant': 'summary', 'field': fname, 'shape': [D, H, W], 'stats': s,
                   'fused_forward_plus_backward_ms': round(pair, 4), 'composition_forward_plus_backward_ms': round(med[variants[6][0]], 4),
                   'composition_over_fused': round(med[variants[6][0]] / pair, 2), 'through_autograd_ms': round(med[variants[7][0]], 4),
                   'composition_over_through_autograd': round(med[variants[6][0]] / med[variants[7][0]], 2),
                   'atomic_bytes': int(atomic_bytes), 'scatter_ms_beyond_the_gather': round(scatter_ms, 4),
                   'atomic_GBps_beyond_the_gather': round(atomic_bytes / (scatter_ms * 1e-3) / 1e9, 1) if scatter_ms > 0 else None,
                   'atomic_GBps_scatter_only_kernel': round(atomic_bytes / (med[variants[3][0]] * 1e-3) / 1e9, 1),
                   'deterministic_over_atomic': round(med[variants[4][0]] / med[variants[1][0]], 2), 'distance_from_float64': agree}
        rows.append(summary)
        print(json.dumps(summary), flush=True)


def bench_step(a, shape, rows):
    from deepatlas_amd.lib.network_factory import get_network
    from deepatlas_amd.models.joint import RegistrationStep
    from deepatlas_amd.optim import FlatAdam
    dev = torch.device('cuda:0')
    ops.set_matrix_precision(ops.DEFAULT_MATRIX_PRECISION)
    g = torch.Generator().manual_seed(11)
    im_m = torch.rand((1, 1) + tuple(shape), generator=g).to(dev)
    im_t = torch.rand((1, 1) + tuple(shape), generator=g).to(dev)
    both_m, both_t = torch.cat((im_m, im_t)), torch.cat((im_t, im_m))
    steps, info = {}, {}
    for key, lam in (('plain', 0.0), ('doubled', 0.0), ('ic', 1.0)):
        torch.manual_seed(0)
        reg = get_network('voxel_morph_cvpr')().to(dev)
        steps[key] = RegistrationStep(reg, FlatAdam(reg.parameters(), lr=1e-4), lam_ic=lam)
    r = steps['ic'].gradients(im_m, im_t)
    info = {'penalty': float(r['ic'])}
    iters = max(a.iters // 2, 3)
    variants = [('registration step, lam_ic = 0 (the step without the penalty)', lambda: steps['plain'](im_m, im_t), iters),
                ('registration step, lam_ic = 0, on the doubled batch', lambda: steps['doubled'](both_m, both_t), iters),
                ('registration step, lam_ic = 1', lambda: steps['ic'](im_m, im_t), iters)]
    times = alternate(variants, a.rounds)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for name, _, _ in variants:
        t = np.array(times[name])
        row = {'variant': name, 'shape': list(shape), 'N': 1, 'ms': round(med[name], 4), 'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4)}
        rows.append(row)
        print('%-64s %-12s %9.4f ms (%.4f - %.4f)' % (name, 'x'.join(map(str, shape)), row['ms'], row['ms_min'], row['ms_max']), flush=True)
    plain, doubled, with_ic = (med[v[0]] for v in variants)
    rows.append(dict({'variant': 'step summary', 'shape': list(shape), 'step_with_ic_over_plain': round(with_ic / plain, 3),
                      'doubled_batch_over_plain': round(doubled / plain, 3), 'loss_itself_ms': round(with_ic - doubled, 4),
                      'loss_itself_share_of_the_step_with_ic': round((with_ic - doubled) / with_ic, 4)}, **info))
    print(json.dumps(rows[-1]), flush=True)
    del steps
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--no-step', action='store_true', help='kernel timings only')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_invcons.py measures on the GPU'
    rows = []
    for s in a.shapes:
        shape = tuple(int(v) for v in s.split('x'))
        bench_kernels(a, shape, rows)
        if not a.no_step:
            bench_step(a, shape, rows)
    out = json.dumps({'bench_invcons': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
