#!/usr/bin/env python
"""Timing of the device augmentation resample (da_spatial_resample, lib/transforms.py:161-290) at 160x192x160, 1-channel fp32 image + uint8
labels, batches of 1 and 4: rigid, B-spline order 2, B-spline order 3 (mesh 3x3x3).  HIP-event timing of warm back-to-back calls of the C
ABI (parameters uploaded once), ms per volume and bytes/s over the compulsory traffic (image and labels read once, written once).  Next to
it, the nearest torch-ROCm composition on the same GPU, as a speed yardstick only (its boundary rules differ): affine_grid + two grid_sample
for the rigid case, a trilinearly up-sampled dense field + two grid_sample for the B-spline.
python tools/bench_augment.py [--iters 50] [--shape D H W]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from deepatlas_amd._native import call, ptr, stream
from deepatlas_amd.lib import transforms as T


def timed(fn, iters):
    for _ in range(5):
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
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--shape', type=int, nargs=3, default=[160, 192, 160])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_augment.py measures on the GPU'
    D, H, W = a.shape
    V = D * H * W
    dev = torch.device('cuda:0')
    rows = []
    for N in (1, 4):
        g = torch.Generator().manual_seed(N)
        img = torch.rand((N, 1, D, H, W), generator=g).to(dev)
        lab = torch.randint(0, 32, (N, D, H, W), generator=g).to(torch.uint8).to(dev)
        img_o, lab_o = torch.empty_like(img), torch.empty_like(lab)
        nbytes = N * V * (4 * 2 + 1 * 2)
        np.random.seed(0)
        o = np.array([W // 2, H // 2, D // 2], dtype=np.float64)
        draws = [(np.random.normal(0, 5, 3) * np.pi / 180, np.random.normal(0, 2, 3)) for _ in range(N)]
        rigid = np.stack([T.rigid_index_affine(r, t, (1, 1, 1), o) for r, t in draws])
        # torch's affine_grid: the same rotation about the volume centre, the translation in normalised units
        theta = torch.from_numpy(np.stack([np.concatenate([T._rotation_zxy(r), (2 * t / [W, H, D])[:, None]], 1) for r, t in draws])
                                 .astype(np.float32)).to(dev)
        for case, order in (('rigid', 0), ('bspline2', 2), ('bspline3', 3)):
            if order:
                A = np.broadcast_to(np.eye(3, 4), (N, 3, 4))
                grid = T.bspline_grid((W, H, D), (3, 3, 3), order)
                coef = np.stack([T.bspline_coefficients(T.draw_bspline(1.0, 3 * int(np.prod(grid)), 4.0, 'Normal'), grid) for _ in range(N)])
                cft = torch.from_numpy(coef.astype(np.float32)).to(dev)
            else:
                A, grid, cft = rigid, (0, 0, 0), None
            kern = np.concatenate([A[:, :, :3], (A[:, :, :3] @ o + A[:, :, 3])[:, :, None]], axis=2)       # ops.spatial_resample's centring
            aff = torch.from_numpy(kern.astype(np.float32)).to(dev)

            def ours():
                call('da_spatial_resample', ptr(img), ptr(img_o), 1, 0, ptr(lab), ptr(lab_o), 1, ptr(aff), ptr(cft), order,
                     grid[0], grid[1], grid[2], N, D, H, W, stream())
            ms = timed(ours, a.iters)
            # torch composition (normalised coordinates, align_corners=False: a voxel-centre grid like ours)
            if order == 0:
                def ref():
                    gr = F.affine_grid(theta, (N, 1, D, H, W), align_corners=False)
                    F.grid_sample(img, gr, mode='bilinear', padding_mode='zeros', align_corners=False)
                    F.grid_sample(lab.float()[:, None], gr, mode='nearest', padding_mode='zeros', align_corners=False).to(torch.uint8)
            else:
                ident = F.affine_grid(torch.eye(3, 4, device=dev)[None].expand(N, 3, 4), (N, 1, D, H, W), align_corners=True)
                scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)], device=dev)

                def ref():
                    field = F.interpolate(cft, size=(D, H, W), mode='trilinear', align_corners=True)        # N x 3 x D x H x W, (x, y, z)
                    gr = ident + field.permute(0, 2, 3, 4, 1) * scale
                    F.grid_sample(img, gr, mode='bilinear', padding_mode='zeros', align_corners=True)
                    F.grid_sample(lab.float()[:, None], gr, mode='nearest', padding_mode='zeros', align_corners=True).to(torch.uint8)
            ms_ref = timed(ref, max(a.iters // 5, 5))
            row = {'case': case, 'N': N, 'shape': [D, H, W], 'ms_per_call': round(ms, 4), 'ms_per_volume': round(ms / N, 4),
                   'GBps_compulsory': round(nbytes / (ms * 1e-3) / 1e9, 1), 'compulsory_MB': round(nbytes / 1e6, 1),
                   'torch_ms_per_volume': round(ms_ref / N, 4), 'speedup_vs_torch': round(ms_ref / ms, 1)}
            rows.append(row)
            print('%-9s N=%d  %.4f ms/volume  %7.1f GB/s  (torch composition %.4f ms/volume, %.1fx)'
                  % (case, N, row['ms_per_volume'], row['GBps_compulsory'], row['torch_ms_per_volume'], row['speedup_vs_torch']))
    print(json.dumps({'bench_augment': rows}))


if __name__ == '__main__':
    main()
