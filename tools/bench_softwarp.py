#!/usr/bin/env python
"""Timing of the Dice between a warped label map and a dense tensor (csrc/warp.hip da_softwarp_dice_*) at 1 x 160 x 192 x 160, C = 32, on a smooth field
(4 voxels of standard deviation, tests/regeval_cases.py's generator) and on a noise field (iid normal displacements of 8 voxels).  HIP-event timing of
warm back-to-back calls, forward + backward; the variants are timed in ROUNDS rounds that alternate, and the median with the min - max spread of the
rounds is reported.  Each fused pair stands beside the composition of the ops that existed before it:
  registration-phase term   ops.LabelWarpSoftDiceFn      against  ops.WarpLabelsFn + ops.DiceFn(soft target)
  segmentation-phase term   ops.SoftmaxLabelWarpDiceFn   against  ops.WarpLabelsFn + ops.DiceFn(softmax=True, soft target)
GB/s over the COMPULSORY bytes of the fused pair -- registration term: the dense tensor once forward and the rows the backward reads (4 C each), the
field twice, d_disp and the gathered labels: 8 C + 38 bytes per voxel; segmentation term: the logits forward, logits in and dlogits out backward, the
field and the gathered labels twice: 12 C + 26 -- as a share of the achievable HBM rate (6.3 TB/s).  Then the whole DeepAtlasJointStep on a
(labelled moving, unlabelled fixed) pair, fused on and off.
python tools/bench_softwarp.py [--iters 20] [--rounds 5] [--shape D H W] [--no-step] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
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


def alternate(variants, rounds, iters):
    for _, _, fn in variants:           # warm every shape (code objects, allocator)
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, _, fn in variants:
            times[name].append(timed(fn, iters))
    return times


def main():
    import regeval_cases as rc
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shape', type=int, nargs=3, default=[160, 192, 160])
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_softwarp.py measures on the GPU'
    D, H, W = a.shape
    V, C, N = D * H * W, 32, 1
    dev = torch.device('cuda:0')
    rows = []
    lab_m = rc.random_labels((D, H, W), N, torch.uint8, seed=1).to(dev)
    g = torch.Generator().manual_seed(5)
    logits = (torch.rand((N, C, D, H, W), generator=g) * 6 - 3).to(dev).contiguous(memory_format=torch.channels_last_3d)
    prob = torch.softmax(logits, 1).contiguous(memory_format=torch.channels_last_3d)
    for field in ('smooth', 'noise'):
        disp = (rc.smooth_field((D, H, W), N, 4.0, seed=3) if field == 'smooth' else rc.noise_field((D, H, W), N, 8.0, seed=4)).to(dev)
        disp = disp.contiguous(memory_format=torch.channels_last_3d)

        def reg_fused():
            u = disp.detach().requires_grad_(True)
            ops.LabelWarpSoftDiceFn.apply(lab_m, u, prob, C, 'Uniform', False, 1e-6).backward()
            return u.grad

        def reg_composed():
            u = disp.detach().requires_grad_(True)
            ops.DiceFn.apply(ops.WarpLabelsFn.apply(lab_m, u, C), None, prob, 'Uniform', False, False, 1e-6).backward()
            return u.grad

        def seg_fused():
            z = logits.detach().requires_grad_(True)
            ops.SoftmaxLabelWarpDiceFn.apply(z, lab_m, disp, 'Uniform', False, 1e-6).backward()
            return z.grad

        def seg_composed():
            z = logits.detach().requires_grad_(True)
            with torch.no_grad():
                target = ops.WarpLabelsFn.apply(lab_m, disp, C)
            ops.DiceFn.apply(z, None, target, 'Uniform', False, True, 1e-6).backward()
            return z.grad

        variants = [('registration term, fused (LabelWarpSoftDiceFn)', 8 * C + 38, reg_fused),
                    ('registration term, composition (WarpLabelsFn + DiceFn)', None, reg_composed),
                    ('segmentation term, fused (SoftmaxLabelWarpDiceFn)', 12 * C + 26, seg_fused),
                    ('segmentation term, composition (WarpLabelsFn + DiceFn softmax)', None, seg_composed)]
        times = alternate(variants, a.rounds, a.iters)
        for name, bpv, _ in variants:
            t = np.array(times[name])
            med = float(np.median(t))
            row = {'variant': name, 'field': field, 'N': N, 'C': C, 'shape': [D, H, W], 'ms_fwd_bwd': round(med, 4), 'ms_min': round(float(t.min()), 4),
                   'ms_max': round(float(t.max()), 4)}
            line = '%-66s %-6s %8.4f ms fwd+bwd (%.4f - %.4f)' % (name, field, med, t.min(), t.max())
            if bpv is not None:
                rate = bpv * V * N / (med * 1e-3)
                row.update(compulsory_bytes_per_voxel=bpv, GBps_compulsory=round(rate / 1e9, 1), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 4))
                line += '  %7.1f GB/s  %.3f of 6.3 TB/s' % (row['GBps_compulsory'], row['share_of_achievable_hbm'])
            rows.append(row)
            print(line, flush=True)
        del disp
    del logits, prob
    if not a.no_step:
        # the whole step on a (labelled moving, unlabelled fixed) pair: the experiment's configuration (UNet_light, voxel_morph_cvpr, split matrix mode)
        from deepatlas_amd.lib.network_factory import get_network
        from deepatlas_amd.models.joint import DeepAtlasJointStep
        from deepatlas_amd.optim import FlatAdam
        ops.set_matrix_precision(ops.DEFAULT_MATRIX_PRECISION)
        ops.enable_async_wgrad(True)
        torch.manual_seed(0)
        seg = get_network('UNet_light')(in_channel=1, n_classes=C, bias=True, BN=True).to(dev)
        reg = get_network('voxel_morph_cvpr')().to(dev)
        seg_opt, reg_opt = FlatAdam(seg.parameters(), lr=1e-3), FlatAdam(reg.parameters(), lr=1e-3)
        im_m, im_t = torch.rand((1, 1, D, H, W), generator=g).to(dev), torch.rand((1, 1, D, H, W), generator=g).to(dev)
        steps = {f: DeepAtlasJointStep(seg, seg_opt, reg, reg_opt, C, fused=f) for f in (True, False)}
        variants = [('joint step, seg_t=None, fused anatomy terms', None, lambda: steps[True](im_m, im_t, lab_m, None)),
                    ('joint step, seg_t=None, composed anatomy terms', None, lambda: steps[False](im_m, im_t, lab_m, None))]
        times = alternate(variants, a.rounds, max(a.iters // 4, 3))
        for name, _, _ in variants:
            t = np.array(times[name])
            rows.append({'variant': name, 'N': N, 'C': C, 'shape': [D, H, W], 'ms_per_step': round(float(np.median(t)), 3), 'ms_min': round(float(t.min()), 3),
                         'ms_max': round(float(t.max()), 3)})
            print('%-66s        %8.3f ms per step (%.3f - %.3f)' % (name, np.median(t), t.min(), t.max()), flush=True)
    out = json.dumps({'bench_softwarp': rows})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
