#!/usr/bin/env python
"""Timing of the volume preprocessing kernels (csrc/preprocess.hip) and of the NIfTI reader (lib/nifti.py) on one MI355X.
Case 1, an int16 volume of 160 x 384 x 384 (an OAI knee scan): every kernel as its wrapper is called (HIP events on warm back-to-back calls,
ROUNDS rounds, median and min - max), beside the host route for the same result on the same array:
  resample   0.7 -> 1.0 mm on every axis, nearest and linear; host: numpy indexing through the same tables (linear: the float32 formula)
  moments    host: numpy mean / var(ddof=1) in float64
  percentiles (0.5, 99.5); host: numpy.percentile on the float32 values
  rescale    (x - a) / b to float32 with the clamp; host: the numpy expression
  label LUT  on a uint8 volume of the same size; host: numpy take
and the share of the achievable HBM rate (6.3 TB/s) over each kernel's COMPULSORY bytes (every input byte once per pass the algorithm needs,
every output byte once).  moments and percentiles return Python floats, so their times include the device-to-host copy of the result.
Case 2: read_nifti of that volume from .nii and from .nii.gz (host, seconds), and one volume end to end: read both files, upload, resample
to 1 mm, percentile rescale, SitkToTensor (the chain of the experiments).
Every ratio is a finding, not a gate.  Not measured: hardware counters, other dtypes and sizes, a loader thread overlapping the read with
the training step, agreement with ITK / SimpleITK (not installed).
python tools/bench_preprocess.py [--iters 10] [--rounds 5] [--shape 160x384x384] [--out profiles/preprocess_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
from deepatlas_amd import ops
from deepatlas_amd.lib import transforms as T
from deepatlas_amd.lib.nifti import read_nifti, write_nifti
from bench_edt import HBM_ACHIEVABLE, alternate


def stats(ts):
    ts = np.asarray(ts)
    return {'ms': round(float(np.median(ts)), 4), 'ms_min': round(float(ts.min()), 4), 'ms_max': round(float(ts.max()), 4)}


def host_ms(fn, rounds):
    fn()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def emit(rows, row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def host_nearest(x, tabs):
    (ld, _, _, ind), (lh, _, _, inh), (lw, _, _, inw) = tabs
    out = x[ld][:, lh][:, :, lw]
    out[~(ind[:, None, None] & inh[None, :, None] & inw[None, None, :])] = 0
    return out


def host_linear(x, tabs):
    (ld, hd, fd, ind), (lh, hh, fh, inh), (lw, hw, fw, inw) = tabs
    X = x.astype(np.float32)
    a, b = X[..., lw], X[..., hw]
    X = fw * (b - a) + a
    a, b = X[:, lh], X[:, hh]
    X = fh[:, None] * (b - a) + a
    a, b = X[ld], X[hd]
    X = fd[:, None, None] * (b - a) + a
    X[~(ind[:, None, None] & inh[None, :, None] & inw[None, None, :])] = 0
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=3)
    ap.add_argument('--shape', type=str, default='160x384x384')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_preprocess.py measures on the GPU'
    dev = torch.device('cuda:0')
    D, H, W = (int(v) for v in a.shape.split('x'))
    V = D * H * W
    rng = np.random.RandomState(0)
    lab = ((np.arange(D)[:, None, None] // 20 + np.arange(H)[None, :, None] // 48 + np.arange(W)[None, None, :] // 48) % 6).astype(np.uint8)
    x = (lab.astype(np.float32) * 300 + rng.gamma(2.0, 60.0, size=(D, H, W))).astype(np.int16)                  # raw MR-like intensities
    xt, lt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    rows = []
    base = {'shape': [D, H, W], 'dtype': 'int16'}

    def share(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 4)

    # resample 0.7 -> 1.0 mm
    scale = (1.0 / 0.7,) * 3
    size = tuple(int(np.ceil(0.7 * n / 1.0)) for n in (D, H, W))
    Vo = size[0] * size[1] * size[2]
    for interp, host, out_bytes in (('nearest', host_nearest, 2), ('linear', host_linear, 4)):
        tabs = [ops.resample_axis_table(n, m, s, 0.0, interp) for n, m, s in zip((D, H, W), size, scale)]
        k = lambda: ops.resample_volume(xt, size, scale, (0.0, 0.0, 0.0), interp, 0)
        got, want = k().cpu().numpy(), host(x, tabs)
        s = stats(alternate([('kernel', k)], a.rounds, a.iters)['kernel'])
        # compulsory: the input voxels the output reads (at most all of them) once, the output once
        comp = min(V, Vo * (1 if interp == 'nearest' else 8)) * 2 + Vo * out_bytes
        h = host_ms(lambda: host(x, tabs), a.host_rounds)
        emit(rows, dict(base, variant='resample_volume 0.7 -> 1.0 mm, ' + interp, out_shape=list(size), **s, compulsory_bytes=comp,
                        share_of_achievable_hbm_over_compulsory=share(comp, s['ms']), host_numpy_indexing=h, host_over_kernel=round(h['ms'] / s['ms'], 1),
                        max_abs_diff_to_host=float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())))

    # moments: two passes over the input
    k = lambda: ops.volume_moments(xt)
    s = stats(alternate([('kernel', k)], a.rounds, a.iters)['kernel'])
    h = host_ms(lambda: (x.mean(dtype=np.float64), x.var(dtype=np.float64, ddof=1)), a.host_rounds)
    c, m, v = k()
    emit(rows, dict(base, variant='volume_moments (result on the host)', **s, compulsory_bytes=2 * V * 2, share_of_achievable_hbm_over_compulsory=share(2 * V * 2, s['ms']),
                    host_numpy_mean_var=h, host_over_kernel=round(h['ms'] / s['ms'], 1),
                    rel_diff_to_host=[abs(m - x.mean(dtype=np.float64)) / abs(m), abs(v - x.var(dtype=np.float64, ddof=1)) / v]))

    # percentiles: three passes over the input
    k = lambda: ops.volume_percentiles(xt, (0.5, 99.5))
    s = stats(alternate([('kernel', k)], a.rounds, a.iters)['kernel'])
    xf = x.astype(np.float32)
    h = host_ms(lambda: np.percentile(xf, [0.5, 99.5]), a.host_rounds)
    emit(rows, dict(base, variant='volume_percentiles (0.5, 99.5) (result on the host)', **s, compulsory_bytes=3 * V * 2,
                    share_of_achievable_hbm_over_compulsory=share(3 * V * 2, s['ms']), host_numpy_percentile=h, host_over_kernel=round(h['ms'] / s['ms'], 1),
                    equal_to_host=bool(np.array_equal(np.asarray(k()), np.percentile(xf.astype(np.float64), [0.5, 99.5])))))

    # rescale
    p_lo, p_hi = ops.volume_percentiles(xt, (0.5, 99.5))
    k = lambda: ops.affine_intensity(xt, p_lo, p_hi - p_lo, clamp=True)
    s = stats(alternate([('kernel', k)], a.rounds, a.iters)['kernel'])
    h = host_ms(lambda: np.clip((xf - np.float32(p_lo)) / np.float32(p_hi - p_lo), 0, 1), a.host_rounds)
    emit(rows, dict(base, variant='affine_intensity with clamp', **s, compulsory_bytes=V * 6, share_of_achievable_hbm_over_compulsory=share(V * 6, s['ms']),
                    host_numpy=h, host_over_kernel=round(h['ms'] / s['ms'], 1)))

    # label look-up
    lut = np.arange(256, dtype=np.int32)
    lut[[2, 5]] = 0
    k = lambda: ops.label_lut(lt, lut)
    s = stats(alternate([('kernel', k)], a.rounds, a.iters)['kernel'])
    h = host_ms(lambda: lut.astype(np.uint8)[lab], a.host_rounds)
    emit(rows, dict(base, dtype='uint8', variant='label_lut (256 entries)', **s, compulsory_bytes=V * 2, share_of_achievable_hbm_over_compulsory=share(V * 2, s['ms']),
                    host_numpy_take=h, host_over_kernel=round(h['ms'] / s['ms'], 1)))

    # case 2: the reader, and one volume end to end
    tmp = tempfile.mkdtemp()
    files = {}
    for ext in ('.nii', '.nii.gz'):
        files[ext] = (write_nifti(os.path.join(tmp, 'v_image' + ext), x, spacing=(0.7, 0.7, 0.7)), write_nifti(os.path.join(tmp, 'v_masks' + ext), lab, spacing=(0.7, 0.7, 0.7)))
        h = host_ms(lambda: read_nifti(files[ext][0]), a.host_rounds)
        emit(rows, dict(base, variant='read_nifti ' + ext, file_bytes=os.path.getsize(files[ext][0]), **h))
    chain = T.Compose([T.Resample((1.0, 1.0, 1.0)), T.PercentileRescale(0.5, 99.5), T.SitkToTensor()])
    for ext in ('.nii', '.nii.gz'):
        def prepare():
            vol, seg = read_nifti(files[ext][0]), read_nifti(files[ext][1])
            t0 = time.perf_counter()
            s = chain({'image': vol.array, 'segmentation': seg.array, 'name': 'v', 'spacing': vol.spacing})
            torch.cuda.synchronize()
            prepare.device_ms.append((time.perf_counter() - t0) * 1e3)
            return s
        prepare.device_ms = []
        h = host_ms(prepare, a.host_rounds)
        emit(rows, dict(base, variant='one volume end to end from ' + ext + ': read image + labels, upload, resample to 1 mm, percentile rescale, SitkToTensor', **h,
                        of_which_upload_and_device_ms=round(float(np.median(prepare.device_ms[1:])), 3)))
    out = json.dumps({'bench_preprocess': rows, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE,
                      'not_measured': ['hardware counters', 'other dtypes and sizes', 'a loader thread overlapping the read with the training step',
                                       'agreement with ITK / SimpleITK (not installed)', 'a training run on real scans']})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
