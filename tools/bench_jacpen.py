#!/usr/bin/env python
"""Timing of the Jacobian folding penalty (csrc/jacpen.hip da_jacdet_penalty_fwd / da_jacdet_penalty_bwd) at 80x96x80 and 160x192x160, N = 1,
eps = 0, p = 1, on a fold-free smooth field (tests/regeval_cases.py's generator, 1.5 voxels of standard deviation) and on smooth + noise fields
whose folding share (measured with ops.jacobian_det) is stated in every row.  HIP-event timing of warm back-to-back calls; every variant is
timed in ROUNDS rounds that alternate with the others, and the median with the min - max spread of the rounds is reported.  The kernel rows
time the C entries themselves on preallocated buffers (_native.call): through torch.autograd a call costs 30 - 90 us of host time, more than
the kernels take, and the 'through autograd' row shows that cost.  Per direction:
ms per call and the rate over the COMPULSORY bytes -- forward 12 per voxel read + 4 for the saved determinant map; backward 4 for the map +
12 written (the displacements are read again only around active voxels and are not counted) -- as a share of the achievable HBM rate
(6.3 TB/s).  Beside them ops.jacobian_det with its map (the evaluation kernel with the same stencil) and the only route without the
kernels: the torch composition of the same formula on the device (torch.gradient + autograd), which materialises nine V-sized derivative
tensors and keeps them for the backward pass.  Then the whole RegistrationStep (VoxelMorph, NCC + bending energy, FlatAdam) with
lam_jac = 1 against lam_jac = 0, which is the step without the penalty bit for bit (tests/test_gpu_jacpen.py), on the field an untrained net
predicts.
python tools/bench_jacpen.py [--iters 20] [--rounds 5] [--shapes 80x96x80 160x192x160] [--no-step] [--out profiles/jacpen_bench.json]"""
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
# (name, standard deviation of the smooth field, of the added iid noise; voxels)
FIELDS = [('smooth', 1.5, 0.0), ('smooth + noise 0.25', 1.5, 0.25), ('smooth + noise 0.5', 1.5, 0.5)]


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


def torch_penalty(disp, eps=0.0, p=1):
    """The definition in torch on the device, in the dtype of disp: what a user without the kernels would run."""
    _, _, D, H, W = disp.shape
    size, dim_of = (W, H, D), (3, 2, 1)
    J = [[None] * 3 for _ in range(3)]
    for c in range(3):
        u = disp[:, c] * ((size[c] - 1) / 2.0)
        for k in range(3):
            g = torch.gradient(u, dim=dim_of[k])[0]
            J[c][k] = g + 1.0 if c == k else g
    det = (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
           + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))
    return (eps - det).clamp(min=0).pow(p).mean()


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


def bench_kernels(a, shape, rows):
    import regeval_cases as rc
    dev = torch.device('cuda:0')
    D, H, W = shape
    V = D * H * W
    one = torch.ones((), device=dev)
    for fname, sd, noise in FIELDS:
        disp = rc.smooth_field(shape, 1, sd, seed=3)
        if noise:
            disp = disp + rc.noise_field(shape, 1, noise, seed=4)
        disp = disp.to(dev).contiguous(memory_format=torch.channels_last_3d)      # the layout the registration net hands out (no copy in ndhwc)
        folds = float(ops.jacobian_det(disp)[:, 4].sum()) / V
        xg = disp.clone().requires_grad_(True)
        loss_k = ops.JacobianPenaltyFn.apply(xg, 0.0, 1)
        # the C entries on buffers of their own
        u = ops.ndhwc(disp)
        loss, gl, det, det2, du = (torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty((1, D, H, W), device=dev),
                                   torch.empty((1, D, H, W), device=dev), torch.empty_like(u))
        stats = torch.empty((1, 8), dtype=torch.float64, device=dev)
        ws = torch.empty(max(nat.lib().da_jacdet_penalty_ws_bytes(1, D, H, W), nat.lib().da_jacobian_det_ws_bytes(1, D, H, W)) + 256, dtype=torch.uint8, device=dev)
        st = nat.stream()

        def k_fwd():
            nat.call('da_jacdet_penalty_fwd', nat.ptr(u), 1, D, H, W, 0.0, 1, nat.ptr(loss), None, nat.ptr(det), nat.ptr(ws), ws.numel(), st)

        def k_bwd():
            nat.call('da_jacdet_penalty_bwd', nat.ptr(u), nat.ptr(det), nat.ptr(gl), nat.ptr(du), 1, D, H, W, 0.0, 1, st)

        def k_det():
            nat.call('da_jacobian_det', nat.ptr(u), 1, D, H, W, nat.ptr(stats), nat.ptr(det2), nat.ptr(ws), ws.numel(), st)

        def through_autograd():
            x = disp.detach().requires_grad_(True)
            ops.JacobianPenaltyFn.apply(x, 0.0, 1).backward()
            return x.grad

        def t_fwd():
            with torch.no_grad():
                return torch_penalty(disp)

        variants = [
            ('penalty forward (da_jacdet_penalty_fwd)', k_fwd, a.iters),
            ('penalty backward (da_jacdet_penalty_bwd)', k_bwd, a.iters),
            ('jacobian_det statistics + map (da_jacobian_det)', k_det, a.iters),
            ('torch composition forward', t_fwd, max(a.iters // 4, 3)),
            ('torch composition forward + backward', lambda: torch.autograd.grad(torch_penalty(xg), xg), max(a.iters // 4, 3)),
            ('penalty forward + backward through autograd', through_autograd, a.iters),
        ]
        nbytes = {variants[0][0]: 16 * V, variants[1][0]: 16 * V, variants[2][0]: 16 * V}
        # the two routes compute the same thing: each against the float64 evaluation of the formula on the device
        x64 = disp.double().requires_grad_(True)
        l64 = torch_penalty(x64)
        g64 = torch.autograd.grad(l64, x64)[0] if folds > 0 else torch.zeros_like(x64)
        l64 = float(l64.detach())

        def distance(loss, grad):
            d = {'loss_abs': abs(float(loss.detach()) - l64)}
            if folds > 0:
                d.update(loss_rel=d['loss_abs'] / abs(l64), grad_rel=float((grad.double() - g64).abs().max() / g64.abs().max()))
            else:
                d.update(grad_max_abs=float(grad.abs().max()))
            return d
        lt = torch_penalty(xg)
        agree = dict(kernels=distance(loss_k, torch.autograd.grad(loss_k, xg, one, retain_graph=True)[0]),
                     torch_float32=distance(lt, torch.autograd.grad(lt, xg)[0]))
        del lt, g64, x64
        torch.cuda.empty_cache()
        times = alternate(variants, a.rounds)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name, _, _ in variants:
            t = np.array(times[name])
            row = {'variant': name, 'field': fname, 'folding_share': round(folds, 6), 'shape': [D, H, W], 'N': 1, 'ms': round(med[name], 4),
                   'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4)}
            line = '%-48s %-20s %-12s %9.4f ms (%.4f - %.4f)' % (name, fname, 'x'.join(map(str, shape)), row['ms'], row['ms_min'], row['ms_max'])
            if name in nbytes:
                rate = nbytes[name] / (med[name] * 1e-3)
                row.update(compulsory_bytes=nbytes[name], GBps_compulsory=round(rate / 1e9, 1), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 4))
                line += '  %7.1f GB/s  %.3f of 6.3 TB/s' % (row['GBps_compulsory'], row['share_of_achievable_hbm'])
            rows.append(row)
            print(line, flush=True)
        pair = med[variants[0][0]] + med[variants[1][0]]
        summary = {'variant': 'summary', 'field': fname, 'folding_share': round(folds, 6), 'shape': [D, H, W],
                   'fused_forward_plus_backward_ms': round(pair, 4), 'torch_forward_plus_backward_ms': round(med[variants[4][0]], 4),
                   'torch_over_fused': round(med[variants[4][0]] / pair, 2), 'through_autograd_ms': round(med[variants[5][0]], 4),
                   'torch_over_through_autograd': round(med[variants[4][0]] / med[variants[5][0]], 2), 'distance_from_float64': agree}
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
    steps, info = {}, {}
    for lam in (0.0, 1.0):
        torch.manual_seed(0)
        reg = get_network('voxel_morph_cvpr')().to(dev)
        step = RegistrationStep(reg, FlatAdam(reg.parameters(), lr=1e-4), lam_jac=lam)
        r = step.gradients(im_m, im_t)
        info[lam] = {'folding_share_of_the_predicted_field': float(ops.jacobian_det(r['disp'])[:, 4].sum()) / r['disp'][:, 0].numel()}
        if 'jac' in r:
            info[lam]['penalty'] = float(r['jac'])
        steps[lam] = step
    variants = [('registration step, lam_jac = 0 (the step without the penalty)', lambda: steps[0.0](im_m, im_t), max(a.iters // 2, 3)),
                ('registration step, lam_jac = 1', lambda: steps[1.0](im_m, im_t), max(a.iters // 2, 3))]
    times = alternate(variants, a.rounds)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for (name, _, _), lam in zip(variants, (0.0, 1.0)):
        t = np.array(times[name])
        row = dict({'variant': name, 'shape': list(shape), 'N': 1, 'ms': round(med[name], 4), 'ms_min': round(float(t.min()), 4),
                    'ms_max': round(float(t.max()), 4)}, **info[lam])
        rows.append(row)
        print('%-64s %-12s %9.4f ms (%.4f - %.4f) %s' % (name, 'x'.join(map(str, shape)), row['ms'], row['ms_min'], row['ms_max'], json.dumps(info[lam])), flush=True)
    rows.append({'variant': 'step summary', 'shape': list(shape), 'penalty_cost_ms': round(med[variants[1][0]] - med[variants[0][0]], 4),
                 'penalty_cost_share_of_step': round(med[variants[1][0]] / med[variants[0][0]] - 1.0, 4)})
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
    assert torch.cuda.is_available(), 'bench_jacpen.py measures on the GPU'
    rows = []
    for s in a.shapes:
        shape = tuple(int(v) for v in s.split('x'))
        bench_kernels(a, shape, rows)
        if not a.no_step:
            bench_step(a, shape, rows)
    out = json.dumps({'bench_jacpen': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
