#!/usr/bin/env python
"""Timing of the registration-evaluation kernels (csrc/regeval.hip) at 160x192x160, N = 1 and 4, on a smooth field (4 voxels of standard
deviation, tests/regeval_cases.py's generator) and on a noise field (iid normal displacements of 8 voxels: what bench.py's untrained
registration net produces).  HIP-event timing of warm back-to-back calls; every variant is timed in ROUNDS rounds that alternate with the
others, and the median with the min - max spread of the rounds is reported.  Per kernel: ms per volume, GB/s over the COMPULSORY bytes
(fused counts 12 disp + 1 target label + 1 gathered moving label = 14 bytes per voxel, + 1 with the warped map; Jacobian statistics 12,
+ 4 with the map) and that rate as a share of the achievable HBM rate (6.3 TB/s).  Beside them the compositions a user would otherwise
write: ops.WarpLabelsFn + ops.argmax_dice_counts (the only device route to hard warped labels without this kernel), torch-ROCm
grid_sample(mode='nearest') + ops.label_overlap_counts, and torch.gradient + the determinant by elementwise ops.
python tools/bench_regeval.py [--iters 20] [--rounds 5] [--shape D H W] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import torch.nn.functional as F
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


def main():
    import regeval_cases as rc
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shape', type=int, nargs=3, default=[160, 192, 160])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_regeval.py measures on the GPU'
    D, H, W = a.shape
    V, C = D * H * W, 32
    dev = torch.device('cuda:0')
    rows = []
    for N in (1, 4):
        lab_m = rc.random_labels((D, H, W), N, torch.uint8, seed=1).to(dev)
        lab_t = rc.random_labels((D, H, W), N, torch.uint8, seed=2).to(dev)
        ident = rc.identity_grid64((D, H, W)).float().to(dev)[None]
        scale = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], device=dev).view(1, 3, 1, 1, 1)
        for field in ('smooth', 'noise'):
            disp = (rc.smooth_field((D, H, W), N, 4.0, seed=3) if field == 'smooth' else rc.noise_field((D, H, W), N, 8.0, seed=4)).to(dev)
            disp = disp.contiguous(memory_format=torch.channels_last_3d)            # the layout the registration net hands out (no copy in ndhwc)

            def torch_nearest_counts():
                w = F.grid_sample(lab_m.float()[:, None], ident + disp.permute(0, 2, 3, 4, 1), mode='nearest', padding_mode='zeros', align_corners=True)
                return ops.label_overlap_counts(w[:, 0].to(torch.uint8), lab_t, C)

            def torch_jacobian():
                u = disp * scale
                g = [torch.gradient(u[:, c], dim=(3, 2, 1)) for c in range(3)]        # d / dx, d / dy, d / dz of component c
                j = [[g[c][k] + (1.0 if c == k else 0.0) for k in range(3)] for c in range(3)]
                det = (j[0][0] * (j[1][1] * j[2][2] - j[1][2] * j[2][1]) - j[0][1] * (j[1][0] * j[2][2] - j[1][2] * j[2][0])
                       + j[0][2] * (j[1][0] * j[2][1] - j[1][1] * j[2][0]))
                return det.mean(), det.std(), det.min(), det.max(), (det <= 0).sum()

            variants = [
                ('reg_label_counts', 14, lambda: ops.reg_label_counts(lab_m, lab_t, disp, C)),
                ('reg_label_counts + warped map', 15, lambda: ops.reg_label_counts(lab_m, lab_t, disp, C, return_warped=True)),
                ('warp_labels_nearest', 14, lambda: ops.warp_labels_nearest(lab_m, disp)),
                ('composition: WarpLabelsFn + argmax_dice_counts', None, lambda: ops.argmax_dice_counts(ops.WarpLabelsFn.apply(lab_m, disp, C), lab_t)),
                ('composition: torch grid_sample nearest + label_overlap_counts', None, torch_nearest_counts),
                ('jacobian_det statistics', 12, lambda: ops.jacobian_det(disp)),
                ('jacobian_det statistics + map', 16, lambda: ops.jacobian_det(disp, return_map=True)),
                ('composition: torch.gradient + elementwise determinant', None, torch_jacobian),
            ]
            for _, _, fn in variants:           # warm every shape (code objects, allocator)
                fn(); fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _, _ in variants}
            for _ in range(a.rounds):           # alternate the variants
                for name, _, fn in variants:
                    times[name].append(timed(fn, a.iters if not name.startswith('composition') else max(a.iters // 4, 3)))
            for name, bpv, _ in variants:
                t = np.array(times[name])
                med = float(np.median(t))
                row = {'variant': name, 'field': field, 'N': N, 'shape': [D, H, W], 'ms_per_volume': round(med / N, 4),
                       'ms_per_volume_min': round(float(t.min()) / N, 4), 'ms_per_volume_max': round(float(t.max()) / N, 4)}
                line = '%-64s %-6s N=%d  %8.4f ms/volume (%.4f - %.4f)' % (name, field, N, row['ms_per_volume'], row['ms_per_volume_min'], row['ms_per_volume_max'])
                if bpv is not None:
                    rate = bpv * V * N / (med * 1e-3)
                    row.update(compulsory_bytes_per_voxel=bpv, GBps_compulsory=round(rate / 1e9, 1), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 4))
                    line += '  %7.1f GB/s  %.3f of 6.3 TB/s' % (row['GBps_compulsory'], row['share_of_achievable_hbm'])
                rows.append(row)
                print(line, flush=True)
    out = json.dumps({'bench_regeval': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
