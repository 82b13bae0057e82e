#!/usr/bin/env python
"""Timing of the intensity-augmentation kernels (csrc/intensity.hip: ops.gaussian_blur, ops.bilateral_filter, ops.intensity_augment) on one
MI355X, N = 1 and N = 2, C = 1, at 80x96x80 and 160x192x160, input torch.rand.
Per kernel, HIP events on warm back-to-back calls, ROUNDS rounds alternating with a torch-on-device composition of the same formula in the same
run, median and min - max:
  blur       the reference default taps (R = 1) and the variance 4 / width 32 / error 0.01 taps; torch: three F.conv3d on a replicate-padded volume
  bilateral  radius 2 (sigma_d 0.5) and radius 4 (sigma_d 1.5), sigma_r 0.06, 50 samples; torch: shifted slices of the padded volume, offset by offset
  pointwise  every stage on (bias order 2 on a 2x2x2 mesh, inverted gamma, gain / offset, noise, clamp); torch: elementwise ops + torch.randn
Each kernel's share of the achievable HBM rate (6.3 TB/s) over its COMPULSORY bytes 2 V 4 (one read, one write of the image), the bilateral
kernel's taps per second, and the host route of the blur (D->H copy, scipy.ndimage.convolve1d three times on 16 threads over slabs, H->D copy).
The op timings are the wrappers as called (taps / tables / flags are uploaded once and kept by content; the pointwise pass uploads its
parameter table and coefficients every call); `kernels_ms` are the kernels alone,
from a torch.profiler trace taken after the timings, with the same share over their summed time.
Last: training steps of SegmentationExperiment (UNet_light, batch 1) without the `augment` key (the parent commit's step: the same route) and
with --aug-intensity --aug-blur 0.5.  Every ratio is a finding, not a gate.
Not measured here: hardware counters (LDS / HBM traffic of the bilateral kernel), C > 1, radii 1 and 3, bias orders 1 and 3, a tiled blur.
python tools/bench_intensity.py [--iters 10] [--rounds 5] [--shapes 80x96x80 160x192x160] [--out profiles/intensity_bench.json]"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
import torch.nn.functional as F
from deepatlas_amd import ops
from deepatlas_amd.lib import transforms as T
from bench_edt import HBM_ACHIEVABLE, alternate

SIGMA_R, SAMPLES = 0.06, 50
ALL_STAGES = dict(gamma=1.3, invert=True, gain=0.9, offset=0.04, noise_std=0.03, clamp=True, seed=5)


def torch_blur(x, taps):
    for axis, pad in ((4, (1, 0, 0)), (3, (0, 1, 0)), (2, (0, 0, 1))):
        t = torch.tensor(np.asarray(taps, dtype=np.float32), device=x.device)
        R = len(taps) // 2
        shape = [1, 1, 1, 1, 1]
        shape[axis] = len(taps)
        padding = (R * pad[0], R * pad[0], R * pad[1], R * pad[1], R * pad[2], R * pad[2])
        x = F.conv3d(F.pad(x, padding, mode='replicate'), t.flip(0).reshape(shape))      # (conv3d correlates; the taps are symmetric anyway)
    return x


def torch_bilateral(x, sigma_d):
    (rx, ry, rz), wd, cutoff, table, scale = ops.bilateral_tables(sigma_d, SIGMA_R, SAMPLES)
    D, H, W = x.shape[-3:]
    p = F.pad(x, (rx, rx, ry, ry, rz, rz), mode='replicate')
    tb = torch.tensor(table, dtype=torch.float32, device=x.device)
    num, den = torch.zeros_like(x), torch.zeros_like(x)
    for oz in range(2 * rz + 1):
        for oy in range(2 * ry + 1):
            for ox in range(2 * rx + 1):
                b = p[..., oz:oz + D, oy:oy + H, ox:ox + W]
                delta = (b - x).abs()
                take = delta < cutoff
                w = torch.where(take, float(wd[oz, oy, ox]) * tb[(delta * float(scale)).floor().long().clamp(max=SAMPLES - 1)], torch.zeros_like(x))
                num += w * b
                den += w
    return num / den


def _basis(size, M, order, dev):
    start, w = T.bspline_support(np.arange(size), size, M, order)
    B = np.zeros((size, M + order))
    for i in range(size):
        B[i, start[i]:start[i] + order + 1] = w[i]
    return torch.tensor(B, dtype=torch.float32, device=dev)


def torch_pointwise(x, coef, basis):
    p = ALL_STAGES
    field = torch.einsum('da,hb,wc,nabc->ndhw', basis[0], basis[1], basis[2], coef)
    v = x * torch.exp(field)[:, None]
    v = 1 - (1 - v.clamp(0, 1)) ** p['gamma']
    v = p['gain'] * v + p['offset']
    v = v + p['noise_std'] * torch.randn_like(v)
    return v.clamp(0, 1)


def host_blur(x_dev, taps, workers):
    from scipy import ndimage
    a = x_dev.cpu().numpy()[0, 0]
    t = np.asarray(taps, dtype=np.float32)
    for axis in (2, 1, 0):
        out = np.empty_like(a)
        split = 0 if axis != 0 else 1                                                     # slabs along an axis the pass does not filter
        bounds = np.linspace(0, a.shape[split], workers + 1).astype(int)

        def one(k):
            sl = [slice(None)] * 3
            sl[split] = slice(bounds[k], bounds[k + 1])
            ndimage.convolve1d(a[tuple(sl)], t, axis=axis, mode='nearest', output=out[tuple(sl)])
        with concurrent.futures.ThreadPoolExecutor(workers) as pool:
            list(pool.map(one, range(workers)))
        a = out
    return torch.from_numpy(a)[None, None].to(x_dev.device)


KERNELS = {'blur_axis_kernel<0>': 'blur pass W', 'blur_axis_kernel<1>': 'blur pass H', 'blur_axis_kernel<2>': 'blur pass D',
           'bilateral_kernel': 'bilateral', 'intensity_kernel': 'pointwise'}


def kernel_ms(fn):
    """{kernel: ms of its launches in one call of fn} from a torch.profiler trace (a run of its own, after the timings), or why it is missing."""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for k, label in KERNELS.items():
                if k in ev.key:
                    t = getattr(ev, 'device_time_total', None)
                    if t is None:
                        t = getattr(ev, 'cuda_time_total', 0.0)
                    out[label] = round(out.get(label, 0.0) + float(t) / 1e3, 4)
        return out or {'unavailable': 'no device events'}
    except Exception as e:
        return {'unavailable': repr(e)}


def kernel_share(kms, compulsory):
    tot = sum(v for v in kms.values() if isinstance(v, float))
    return round(compulsory / (tot * 1e-3) / HBM_ACHIEVABLE, 4) if tot > 0 else None


def stats(ts):
    ts = np.asarray(ts)
    return {'ms': round(float(np.median(ts)), 4), 'ms_min': round(float(ts.min()), 4), 'ms_max': round(float(ts.max()), 4)}


def emit(rows, row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def bench_shape(a, shape, N, rows):
    dev = torch.device('cuda:0')
    D, H, W = shape
    V = D * H * W
    x = torch.rand((N, 1, D, H, W), generator=torch.Generator().manual_seed(3)).to(dev)
    compulsory = 2 * N * V * 4
    base = {'shape': list(shape), 'N': N}

    def share(ms):
        return round(compulsory / (ms * 1e-3) / HBM_ACHIEVABLE, 4)

    for label, taps in (('reference default (0.5, 1, 0.9)', T.discrete_gaussian_taps(0.5, 1, 0.9)), ('variance 4, width 32, error 0.01', T.discrete_gaussian_taps(4.0, 32, 0.01))):
        k, t = (lambda: ops.gaussian_blur(x, taps)), (lambda: torch_blur(x, taps))
        diff = float((k() - t()).abs().max())
        times = alternate([('kernel', k), ('torch', t)], a.rounds, a.iters)
        s = stats(times['kernel'])
        emit(rows, dict(base, variant='gaussian_blur', taps=label, radius=len(taps) // 2, **s, moved_bytes_model=3 * compulsory, compulsory_bytes=compulsory,
                        share_of_achievable_hbm_over_compulsory=share(s['ms']), torch_conv3d_x3=stats(times['torch']),
                        torch_over_kernel=round(float(np.median(times['torch'])) / s['ms'], 2), max_abs_diff_to_torch=diff, kernels_ms=kernel_ms(k),
                        kernels_share_of_achievable_hbm_over_compulsory=kernel_share(kernel_ms(k), compulsory)))
        if N == 1:
            host = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = host_blur(x, taps, a.host_threads)
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e3)
            emit(rows, dict(base, variant='host route: D->H, scipy convolve1d x 3 on %d threads, H->D' % a.host_threads, taps=label, **stats(host),
                            host_over_kernel=round(float(np.median(host)) / s['ms'], 1), max_abs_diff_to_kernel=float((h - k()).abs().max())))

    for sigma_d in (0.5, 1.5):
        (rx, ry, rz) = ops.bilateral_tables(sigma_d, SIGMA_R, SAMPLES)[0]
        taps_n = (2 * rx + 1) * (2 * ry + 1) * (2 * rz + 1)
        k, t = (lambda: ops.bilateral_filter(x, sigma_d, SIGMA_R, SAMPLES)), (lambda: torch_bilateral(x, sigma_d))
        d = (k() - t()).abs()
        tk = alternate([('kernel', k)], a.rounds, a.iters)['kernel']
        tt = alternate([('torch', t)], 2, 1)['torch']                                     # (hundreds of launches a call: two single calls are enough)
        s = stats(tk)
        emit(rows, dict(base, variant='bilateral_filter', radius=rx, taps_per_voxel=taps_n, **s, compulsory_bytes=compulsory,
                        share_of_achievable_hbm_over_compulsory=share(s['ms']), taps_per_second=round(N * V * taps_n / (s['ms'] * 1e-3), -6),
                        torch_shifted_slices=stats(tt), torch_over_kernel=round(float(np.median(tt)) / s['ms'], 1),
                        mean_abs_diff_to_torch=float(d.mean()), share_of_voxels_off_by_more_than_1e_5=float((d > 1e-5).float().mean()), kernels_ms=kernel_ms(k),
                        kernel_taps_per_second=(lambda km: round(N * V * taps_n / (km['bilateral'] * 1e-3), -6) if 'bilateral' in km else None)(kernel_ms(k))))

    grid = T.bspline_grid((W, H, D), (2, 2, 2), 2)
    coef = np.random.RandomState(1).normal(0, 0.15, (N, grid[2], grid[1], grid[0]))
    coef_t = torch.tensor(coef, dtype=torch.float32, device=dev)
    basis = [_basis(s, 2, 2, dev) for s in (D, H, W)]
    k, t = (lambda: ops.intensity_augment(x, ALL_STAGES, coef, 2)), (lambda: torch_pointwise(x, coef_t, basis))
    quiet = dict(ALL_STAGES, noise_std=None)
    times = alternate([('kernel', k), ('torch', t)], a.rounds, a.iters)
    s = stats(times['kernel'])
    emit(rows, dict(base, variant='intensity_augment (all stages)', **s, compulsory_bytes=compulsory, share_of_achievable_hbm_over_compulsory=share(s['ms']),
                    torch_elementwise_randn=stats(times['torch']), torch_over_kernel=round(float(np.median(times['torch'])) / s['ms'], 2),
                    std_of_diff_to_torch_its_own_noise=float((k() - t()).std()), kernels_ms=kernel_ms(k),
                    kernels_share_of_achievable_hbm_over_compulsory=kernel_share(kernel_ms(k), compulsory),
                    max_abs_diff_without_noise=float((ops.intensity_augment(x, quiet, coef, 2)
                                                      - (ALL_STAGES['gain'] * (1 - (1 - (x * torch.exp(torch.einsum('da,hb,wc,nabc->ndhw', *basis, coef_t))[:, None]).clamp(0, 1)) ** ALL_STAGES['gamma'])
                                                         + ALL_STAGES['offset']).clamp(0, 1)).abs().max())))


def bench_step(a, shape, rows):
    import contextlib
    import io
    import tempfile
    import train_seg
    from deepatlas_amd.models.segmentation import SegmentationExperiment
    res = {}
    exps = {}
    for key, extra in (('without', []), ('aug_intensity_blur', ['--aug-intensity', '--aug-blur', '0.5'])):
        ns = argparse.Namespace(device='0', debug=False, preload=False, num_samples=1, num_epochs=1, lr=1e-3, test_only=False,
                                data_root='./data', log_root=tempfile.mkdtemp(), shape=list(shape), aug_intensity=bool(extra), aug_blur=0.5 if extra else None)
        with contextlib.redirect_stdout(io.StringIO()):
            exp = SegmentationExperiment(train_seg.build_config(ns))
            exp.setup_train()
            exp.initialize_model(exp.model, exp.optimizer, '')
        images, truths, _ = next(iter(exp.training_data_loader))
        exps[key] = (exp, images, truths)
        res[key] = []

    def steps(key, n):
        exp, images, truths = exps[key]
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            im, tr = exp.augment_batch(images, truths) if exp.augment else (images, truths)
            exp.train_step(im, tr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    for key in res:
        steps(key, 2)
    for _ in range(a.rounds):
        for key in res:
            res[key].append(steps(key, a.step_iters))
    med = {k: round(float(np.median(v)), 2) for k, v in res.items()}
    emit(rows, {'variant': 'SegmentationExperiment training step (UNet_light, batch 1)', 'shape': list(shape), 'ms': med,
                'ms_min_max': {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()},
                'augmentation_cost_ms': round(med['aug_intensity_blur'] - med['without'], 2),
                'note': 'without the key the step takes the route of the parent commit'})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--step-iters', type=int, default=3)
    ap.add_argument('--host-threads', type=int, default=16)
    ap.add_argument('--shapes', type=str, nargs='+', default=['80x96x80', '160x192x160'])
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_intensity.py measures on the GPU'
    assert 1 <= a.host_threads <= 16
    rows = []
    for s in a.shapes:
        shape = tuple(int(v) for v in s.split('x'))
        for N in (1, 2):
            bench_shape(a, shape, N, rows)
        bench_step(a, shape, rows)
    out = json.dumps({'bench_intensity': rows, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE,
                      'not_measured': ['hardware counters (LDS and HBM traffic of the bilateral kernel)', 'C > 1', 'bilateral radii 1 and 3',
                                       'bias orders 1 and 3', 'a tiled blur that fuses axes through LDS', 'agreement with ITK / SimpleITK (not installed)']})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
