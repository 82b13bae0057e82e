#!/usr/bin/env python
"""Timing of the mutual-information similarity (csrc/mi.hip da_mi_fwd / da_mi_bwd) at 80x96x80 and 160x192x160, N = 1, 32 bins, on a
non-linearly related pair (y = a fold of x plus noise).  HIP-event timing of warm back-to-back calls; every variant is timed in ROUNDS
rounds that alternate with the others, and the median with the min - max spread of the rounds is reported.  Per direction: ms per call,
the share of the fp32 matrix-instruction rate (155 TFLOP/s measured) over the 2 V B^2 FLOP of the outer-product sum (forward) and of the
two B x B by B x V products (backward: 4 V B^2), and the compulsory bytes (forward 8 per voxel read; backward 8 read + 8 written).  Beside
them the only route without the kernels -- the torch composition of the same formula on the device, which materialises the two V x B
weight matrices and keeps them for autograd -- and da_ncc_fwd / da_ncc_bwd on the same pair as context (the similarity MI replaces; a
streaming kernel).
python tools/bench_mi.py [--iters 20] [--rounds 5] [--shapes 80x96x80 160x192x160] [--bins 32] [--out profiles/mi_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from deepatlas_amd import ops

MFMA_F32_RATE = 155e12       # FLOP / s, v_mfma_f32_32x32x2_f32 back to back on every SIMD


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


def torch_mi(x, y, bins, sigma_ratio=1.0, vmin=0.0, vmax=1.0):
    """The definition in torch on the device (float32): what a user without the kernels would run."""
    N = x.shape[0]
    x, y = x.reshape(N, -1), y.reshape(N, -1)
    V = x.shape[1]
    c = torch.linspace(vmin, vmax, bins, dtype=x.dtype, device=x.device)
    p = 1.0 / (2.0 * ((vmax - vmin) / (bins - 1) * sigma_ratio) ** 2)

    def weights(t):
        e = torch.exp(-p * (t.clamp(vmin, vmax).unsqueeze(-1) - c) ** 2)
        return e / e.sum(-1, keepdim=True)
    wx, wy = weights(x), weights(y)
    P = torch.bmm(wx.transpose(1, 2), wy) / V
    a, b = wx.mean(1), wy.mean(1)
    R = P / (a.unsqueeze(2) * b.unsqueeze(1) + 1e-6) + 1e-6
    return -(P * torch.log(R)).sum((1, 2)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--bins', type=int, default=32)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mi.py measures on the GPU'
    dev = torch.device('cuda:0')
    B = a.bins
    rows = []
    for shape in a.shapes:
        D, H, W = (int(s) for s in shape.split('x'))
        V = D * H * W
        g = torch.Generator().manual_seed(7)
        u = torch.rand((1, 1, D, H, W), generator=g)
        x = u.to(dev)
        y = (0.1 + 0.8 * (2 * u - 1).abs() ** 1.5 + 0.04 * torch.randn(u.shape, generator=g)).to(dev)      # (a few values beyond [0, 1]: clamped by the loss)
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        one = torch.ones((), device=dev)

        def mi_fwd():
            return ops.MIFn.apply(x, y, B)

        loss_k = ops.MIFn.apply(xg, yg, B)

        def mi_bwd():
            return torch.autograd.grad(loss_k, (xg, yg), one, retain_graph=True)

        def ncc_fwd():
            return ops.NCCFn.apply(x, y)

        loss_n = ops.NCCFn.apply(xg, yg)

        def ncc_bwd():
            return torch.autograd.grad(loss_n, (xg, yg), one, retain_graph=True)

        def t_fwd():
            with torch.no_grad():
                return torch_mi(x, y, B)

        def t_fwd_bwd():
            return torch.autograd.grad(torch_mi(xg, yg, B), (xg, yg))

        # the two routes compute the same thing: each against the float64 evaluation of the formula on the device
        x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
        l64 = torch_mi(x64, y64, B)
        g64 = torch.autograd.grad(l64, (x64, y64))
        l64 = float(l64.detach())

        def distance(loss, grads):
            return dict(loss_abs=abs(float(loss.detach()) - l64), dx_rel=float((grads[0].double() - g64[0]).abs().max() / g64[0].abs().max()),
                        dy_rel=float((grads[1].double() - g64[1]).abs().max() / g64[1].abs().max()))
        lt = torch_mi(xg, yg, B)
        agree = dict(kernels=distance(loss_k, mi_bwd()), torch_float32=distance(lt, torch.autograd.grad(lt, (xg, yg))))
        del lt, g64, x64, y64
        torch.cuda.empty_cache()
        variants = [
            ('mi forward (da_mi_fwd)', 2 * V * B * B, 8 * V, mi_fwd, a.iters),
            ('mi backward (da_mi_bwd, dx and dy)', 4 * V * B * B, 16 * V, mi_bwd, a.iters),
            ('torch composition forward', None, 2 * 4 * V * B + 8 * V, t_fwd, max(a.iters // 4, 3)),
            ('torch composition forward + backward', None, None, t_fwd_bwd, max(a.iters // 4, 3)),
            ('ncc forward (da_ncc_fwd)', None, 8 * V, ncc_fwd, a.iters),
            ('ncc backward (da_ncc_bwd)', None, 16 * V, ncc_bwd, a.iters),
        ]
        for v in variants:
            v[3](); v[3]()
        torch.cuda.synchronize()
        times = {v[0]: [] for v in variants}
        for _ in range(a.rounds):
            for name, _, _, fn, iters in variants:
                times[name].append(timed(fn, iters))
        med = {k: float(np.median(v)) for k, v in times.items()}
        fused_pair = med[variants[0][0]] + med[variants[1][0]]
        for name, flop, nbytes, _, _ in variants:
            t = np.array(times[name])
            row = {'variant': name, 'shape': [D, H, W], 'N': 1, 'bins': B, 'ms': round(med[name], 4), 'ms_min': round(float(t.min()), 4),
                   'ms_max': round(float(t.max()), 4)}
            line = '%-40s %-12s %9.4f ms (%.4f - %.4f)' % (name, shape, row['ms'], row['ms_min'], row['ms_max'])
            if flop is not None:
                row.update(flop=flop, share_of_fp32_mfma_rate=round(flop / (med[name] * 1e-3) / MFMA_F32_RATE, 4))
                line += '  %.3f of the fp32 MFMA rate' % row['share_of_fp32_mfma_rate']
            if nbytes is not None:
                row.update(bytes=nbytes)
                line += '  %.1f MB' % (nbytes / 1e6)
            rows.append(row)
            print(line, flush=True)
        summary = {'variant': 'summary', 'shape': [D, H, W], 'fused_forward_plus_backward_ms': round(fused_pair, 4),
                   'torch_forward_plus_backward_ms': round(med[variants[3][0]], 4),
                   'torch_over_fused': round(med[variants[3][0]] / fused_pair, 2), 'distance_from_float64': agree}
        rows.append(summary)
        print(json.dumps(summary), flush=True)
    out = json.dumps({'bench_mi': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
