#!/usr/bin/env python
"""Timing of multi-atlas label fusion (csrc/regeval.hip da_label_fusion_vote, da_local_msd_weights) at 160x192x160, N = 1, K = 5 and 16
atlases, on smooth fields (4 voxels of standard deviation, tests/regeval_cases.py's generator) and noise fields (iid normal
displacements of 8 voxels), with blocky atlas labels (lib/datasets.py structured_labels) and iid labels, 32 classes.  HIP-event timing of
warm back-to-back calls; every variant is timed in ROUNDS rounds that alternate with the others, and the median with the min - max spread
of the rounds is reported.  Per kernel: ms per call, GB/s over the COMPULSORY bytes (vote: per atlas 12 displacement + 1 gathered label,
+ 1 fused label = 13 K + 1 bytes per voxel, + 4 K with per-voxel weights, + 4 with the confidence; weights: per atlas 4 read + 4
written, + 4 for the target) and that rate as a share of the achievable HBM rate (6.3 TB/s).  Beside them the only route without the
kernel: K x ops.warp_labels_nearest, then torch one_hot - sum - argmax.
python tools/bench_label_fusion.py [--iters 20] [--rounds 5] [--shape D H W] [--out FILE]"""
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
from deepatlas_amd.lib.datasets import structured_labels

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
    ap.add_argument('--atlases', type=int, nargs='+', default=[5, 16])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_label_fusion.py measures on the GPU'
    D, H, W = a.shape
    V, C = D * H * W, 32
    dev = torch.device('cuda:0')
    rows = []
    for K in a.atlases:
        for field in ('smooth', 'noise'):
            disp = (rc.smooth_field((D, H, W), K, 4.0, seed=3) if field == 'smooth' else rc.noise_field((D, H, W), K, 8.0, seed=4)).to(dev)
            disp = disp.contiguous(memory_format=torch.channels_last_3d)            # the layout the registration net hands out (no copy in ndhwc)
            g = torch.Generator().manual_seed(5)
            w_voxel = torch.rand((1, K, D, H, W), generator=g).to(dev)
            w_atlas = torch.rand((1, K), generator=g).to(dev)
            images = torch.rand((1, K, D, H, W), generator=g).to(dev)
            target = torch.rand((1, D, H, W), generator=g).to(dev)
            for labels_kind in ('blocky', 'iid'):
                if labels_kind == 'blocky':
                    lab = torch.stack([structured_labels((D, H, W), C, seed=i) for i in range(K)]).to(dev)
                else:
                    lab = rc.random_labels((D, H, W), K, torch.uint8, seed=1).to(dev)

                def composition():
                    score = None
                    for k in range(K):
                        w = ops.warp_labels_nearest(lab[k:k + 1], disp[k:k + 1])
                        oh = F.one_hot(w.long(), C)
                        score = oh if score is None else score + oh
                    return score.argmax(-1).to(torch.uint8)

                variants = [
                    ('label_fusion majority', 13 * K + 1, lambda: ops.label_fusion(lab, disp)),
                    ('label_fusion majority + confidence', 13 * K + 5, lambda: ops.label_fusion(lab, disp, return_confidence=True)),
                    ('label_fusion per-atlas weights', 13 * K + 1, lambda: ops.label_fusion(lab, disp, w_atlas)),
                    ('label_fusion per-voxel weights', 17 * K + 1, lambda: ops.label_fusion(lab, disp, w_voxel)),
                    ('composition: K x warp_labels_nearest + one_hot-sum-argmax', None, composition),
                ]
                if labels_kind == 'blocky':             # (the weights do not depend on the labels: timed once per field)
                    variants.append(('local_msd_weights r=2', 8 * K + 4, lambda: ops.local_msd_weights(images, target, radius=2, sigma=0.1)))
                for _, _, fn in variants:           # warm every shape (code objects, allocator)
                    fn(); fn()
                torch.cuda.synchronize()
                assert torch.equal(ops.label_fusion(lab, disp), composition())          # the two routes compute the same map
                times = {name: [] for name, _, _ in variants}
                for _ in range(a.rounds):           # alternate the variants
                    for name, _, fn in variants:
                        times[name].append(timed(fn, a.iters if not name.startswith('composition') else max(a.iters // 4, 3)))
                comp = float(np.median(times[variants[4][0]]))
                for name, bpv, _ in variants:
                    t = np.array(times[name])
                    med = float(np.median(t))
                    row = {'variant': name, 'field': field, 'labels': labels_kind, 'K': K, 'N': 1, 'shape': [D, H, W], 'ms': round(med, 4),
                           'ms_min': round(float(t.min()), 4), 'ms_max': round(float(t.max()), 4)}
                    line = '%-62s K=%-2d %-6s %-6s %9.4f ms (%.4f - %.4f)' % (name, K, field, labels_kind, row['ms'], row['ms_min'], row['ms_max'])
                    if bpv is not None:
                        rate = bpv * V / (med * 1e-3)
                        row.update(compulsory_bytes_per_voxel=bpv, GBps_compulsory=round(rate / 1e9, 1), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 4))
                        line += '  %7.1f GB/s  %.3f of 6.3 TB/s' % (row['GBps_compulsory'], row['share_of_achievable_hbm'])
                        if name.startswith('label_fusion'):
                            row['composition_over_kernel'] = round(comp / med, 2)
                            line += '  composition / kernel %.1f' % row['composition_over_kernel']
                    rows.append(row)
                    print(line, flush=True)
    out = json.dumps({'bench_label_fusion': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
