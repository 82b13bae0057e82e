"""Every launcher stays inside the workspace its size function reports.

`_native._Workspace.get` hands out 256 bytes + 25 % more than it is asked for, so a launcher that needs a few bytes more than da_X_ws_bytes says would
never be noticed.  Here `get` of the `nat.workspace` singleton (ops and _native share the object) is replaced: it allocates 64 KiB + nbytes + 64 KiB,
fills both bands with 0xA5, returns the pointer to the middle and reports exactly nbytes.  After each op both bands must be intact (one .all() per
band, on the device) and the result must equal, bit for bit, what the same op returns with the normal workspace: a region that moved or shrank would
change the result before it reaches a band.  (None of the ops below accumulates with floating-point atomics: the warp's data gradient is taken in its
deterministic fixed-point form, the reductions are per-workgroup partials summed in a fixed order.)

A band overwritten inside the 128 KiB of slack is a failed assertion, not a fault.  The ops are called through deepatlas_amd.ops where an autograd
node reaches the entry, otherwise through the C ABI as the neighbouring tests do; inputs come from the tests' own generators at small shapes.
The whole file runs in a few seconds."""
import ctypes

import numpy as np
import pytest
import torch

import crop_cases
import edt_cases
import fusion_cases
import invert_cases
import mi_cases
import surface_cases
from test_gpu_ops import cl, dev, rnd

pytestmark = pytest.mark.gpu
BAND = 64 * 1024
FILL = 0xA5


class Guarded(object):
    """Replacement for _Workspace.get: exact size, a band of FILL on either side.  Every buffer stays alive until check()."""

    def __init__(self):
        self.bufs = []

    def get(self, nbytes, device):
        nbytes = int(nbytes)
        b = torch.empty(BAND + nbytes + BAND, dtype=torch.uint8, device=device)
        b[:BAND].fill_(FILL)
        b[BAND + nbytes:].fill_(FILL)
        self.bufs.append((b, nbytes))
        return ctypes.c_void_p(b.data_ptr() + BAND), ctypes.c_size_t(nbytes)

    def check(self):
        torch.cuda.synchronize()
        assert self.bufs, 'the op never asked for a workspace'
        for b, n in self.bufs:
            assert bool((b[:BAND] == FILL).all()), 'bytes in FRONT of a %d-byte workspace were overwritten' % n
            assert bool((b[BAND + n:] == FILL).all()), 'bytes BEHIND a %d-byte workspace were overwritten' % n


def both(monkeypatch, fn, entries=()):
    """fn() with the normal workspace, then under the guard: bands intact, the same tensors bit for bit, and the C-ABI entries named were reached."""
    from deepatlas_amd import _native as nat
    from deepatlas_amd import ops
    ref = fn()
    ops.join_side_stream()
    torch.cuda.synchronize()
    g = Guarded()
    prof = nat.CallProfiler()
    with monkeypatch.context() as m:
        m.setattr(nat.workspace, 'get', g.get)
        m.setattr(nat, 'profiler', prof)
        out = fn()
        ops.join_side_stream()
        g.check()
    seen = set(k[0] for k in prof.records)
    for e in entries:
        assert e in seen, '%s was not called (called: %s)' % (e, sorted(seen))
    assert len(ref) == len(out)
    for i, (r, o) in enumerate(zip(ref, out)):
        if r is None and o is None:
            continue
        assert r.shape == o.shape and r.dtype == o.dtype
        same = (r == o) | (torch.isnan(r) & torch.isnan(o)) if r.dtype.is_floating_point else (r == o)
        assert bool(same.all()), 'result %d differs between the normal and the exact-size workspace' % i


@pytest.fixture
def split_mode():
    from deepatlas_amd import ops
    prev = ops.set_matrix_precision('fp32_split')
    yield
    ops.set_matrix_precision(prev)


def _grads(*ts):
    return [t.grad.detach().clone() if (t is not None and t.grad is not None) else None for t in ts]


# ---- 3x3x3 convolutions: forward, data gradient, weight gradient with dbias (no activation: the bias gradient comes from da_conv3d_k3_wgrad) ----
def _conv_fn(C1, C2, Cout, stride, dims, up2=False):
    from deepatlas_amd import ops
    N, D, H, W = dims
    x1 = rnd((N, C1, D, H, W), 1)
    x2 = rnd((N, C2, D, H, W), 2) if C2 else None
    w, b = rnd((Cout, C1 + C2, 3, 3, 3), 3, 0.2), rnd((Cout,), 4, 0.1)
    so = (2 * D, 2 * H, 2 * W) if up2 else tuple((s - 1) // stride + 1 for s in (D, H, W))
    go = rnd((N, Cout) + so, 5)

    def fn():
        xg1 = cl(x1).requires_grad_(True)
        xg2 = cl(x2).requires_grad_(True) if C2 else None
        wg, bg = w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
        y = ops.Conv3dK3Fn.apply(xg1, xg2, wg, bg, stride, -1.0, *((False, False, True) if up2 else ()))
        y.backward(cl(go))
        return [y.detach()] + _grads(xg1, xg2, wg, bg)
    return fn


CONV = [
    # C1, C2, Cout, stride, entries
    (16, 0, 16, 1), (32, 16, 16, 1),          # stride 1: 16 -> 16 and the 48 -> 16 concat layer
    (16, 0, 32, 2), (16, 0, 16, 2),           # stride 2: the native kernels' channel counts and the space-to-depth route's
]
CONV_DIMS = [(1, 8, 8, 16), (2, 5, 9, 18)]


@pytest.mark.parametrize('dims', CONV_DIMS, ids=lambda d: 'x'.join(map(str, d)))
@pytest.mark.parametrize('case', CONV, ids=lambda c: 'c%d+%d_o%d_s%d' % c)
def test_conv3d(monkeypatch, split_mode, case, dims):
    C1, C2, Cout, stride = case
    both(monkeypatch, _conv_fn(C1, C2, Cout, stride, dims), ('da_conv3d_k3_fwd', 'da_conv3d_k3_dgrad', 'da_conv3d_k3_wgrad'))


@pytest.mark.parametrize('dims', CONV_DIMS, ids=lambda d: 'x'.join(map(str, d)))
@pytest.mark.parametrize('case', [(16, 0, 16, 1), (32, 16, 16, 1), (16, 0, 32, 2)], ids=lambda c: 'c%d+%d_o%d_s%d' % c)
def test_conv3d_direct_kernels(monkeypatch, split_mode, case, dims):
    from deepatlas_amd import _native as nat
    C1, C2, Cout, stride = case
    prev = nat.lib().da_set_conv_direct(1)
    try:
        both(monkeypatch, _conv_fn(C1, C2, Cout, stride, dims), ('da_conv3d_k3_fwd', 'da_conv3d_k3_dgrad', 'da_conv3d_k3_wgrad'))
    finally:
        nat.lib().da_set_conv_direct(prev)


@pytest.mark.parametrize('dims', [(1, 4, 4, 8), (2, 3, 5, 9)], ids=lambda d: 'x'.join(map(str, d)))
@pytest.mark.parametrize('case', [(16, 16, 16), (32, 0, 8)], ids=lambda c: 'c%d+%d_o%d' % c)
def test_folded_upsampling_conv(monkeypatch, split_mode, case, dims):
    C1, C2, Cout = case
    both(monkeypatch, _conv_fn(C1, C2, Cout, 1, dims, up2=True), ('da_upconv3d_k3_fwd', 'da_upconv3d_k3_dgrad', 'da_upconv3d_k3_wgrad'))


@pytest.mark.parametrize('dims', CONV_DIMS, ids=lambda d: 'x'.join(map(str, d)))
@pytest.mark.parametrize('case', [(16, 0, 16), (32, 16, 16)], ids=lambda c: 'c%d+%d_o%d' % c)
def test_conv3d_forward_with_statistics_and_batchnorm_backward(monkeypatch, split_mode, case, dims):
    from deepatlas_amd import ops
    C1, C2, Cout = case
    N, D, H, W = dims
    x1 = rnd((N, C1, D, H, W), 1)
    x2 = rnd((N, C2, D, H, W), 2) if C2 else None
    w, b = rnd((Cout, C1 + C2, 3, 3, 3), 3, 0.2), rnd((Cout,), 4, 0.1)
    gamma, beta = 1 + rnd((Cout,), 6, 0.2), rnd((Cout,), 7, 0.2)
    go = rnd((N, Cout, D, H, W), 5)

    def fn():
        xg1 = cl(x1).requires_grad_(True)
        xg2 = cl(x2).requires_grad_(True) if C2 else None
        ps = [t.to(dev()).requires_grad_(True) for t in (w, b, gamma, beta)]
        rm, rv = torch.zeros(Cout, device=dev()), torch.ones(Cout, device=dev())
        y = ops.ConvBNActFn.apply(xg1, xg2, ps[0], ps[1], ps[2], ps[3], rm, rv, True, 0.1, 1e-5, 0.01)
        y.backward(cl(go))
        return [y.detach(), rm, rv] + _grads(xg1, xg2, *ps)
    both(monkeypatch, fn, ('da_conv3d_k3_fwd_bnstats',))


# ---- the pointwise layers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cin,Cout,dims', [(128, 80, (1, 2, 3, 5)), (6, 5, (1, 2, 3, 4)), (32, 32, (2, 4, 4, 6))],
                         ids=['wide-sliced', 'direct', 'one-slice'])
def test_deconv_k2s2(monkeypatch, Cin, Cout, dims):
    """128 -> 80: da_pw_wgrad's 64 x 64 slices and their `tmp` region; 6 -> 5: channel counts the matrix path declines, the direct kernel's partials."""
    from deepatlas_amd import ops
    N, D, H, W = dims
    x, w, b = rnd((N, Cin, D, H, W), 1), rnd((Cin, Cout, 2, 2, 2), 2, 0.3), rnd((Cout,), 3, 0.1)
    go = rnd((N, Cout, 2 * D, 2 * H, 2 * W), 4)

    def fn():
        xg, wg, bg = cl(x).requires_grad_(True), w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
        y = ops.DeconvK2S2Fn.apply(xg, wg, bg)
        y.backward(cl(go))
        return [y.detach()] + _grads(xg, wg, bg)
    both(monkeypatch, fn, ('da_deconv_k2s2_fwd', 'da_deconv_k2s2_dgrad', 'da_deconv_k2s2_wgrad'))


@pytest.mark.parametrize('Cin,Cout,dims', [(16, 32, (1, 4, 6, 8)), (32, 16, (1, 4, 6, 8)), (128, 80, (1, 4, 6, 8)), (16, 32, (1, 4, 4, 8)), (16, 96, (1, 2, 2, 2))],
                         ids=['16-32', '32-16', '128-80', '16-32-small', '16-96-one-voxel'])
def test_conv_k2s2(monkeypatch, Cin, Cout, dims):
    """Cout > Cin on small volumes: the bias gradient's column-sum scratch has Cout entries, more than the transposed conv's size with the channels exchanged
    holds; da_conv_k2s2_wgrad_ws_bytes sizes it for the wider count.  At 16 -> 96 on one output voxel the scratch is larger than everything in front of it."""
    from deepatlas_amd import ops
    N, D, H, W = dims
    x, w, b = rnd((N, Cin, D, H, W), 1), rnd((Cout, Cin, 2, 2, 2), 2, 0.3), rnd((Cout,), 3, 0.1)
    go = rnd((N, Cout, D // 2, H // 2, W // 2), 4)

    def fn():
        xg, wg, bg = cl(x).requires_grad_(True), w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
        y = ops.ConvK2S2Fn.apply(xg, wg, bg)
        y.backward(cl(go))
        return [y.detach()] + _grads(xg, wg, bg)
    both(monkeypatch, fn, ('da_conv_k2s2_fwd', 'da_conv_k2s2_dgrad', 'da_conv_k2s2_wgrad'))


@pytest.mark.parametrize('Cin,Cout', [(16, 32), (8, 5), (128, 80)])
def test_conv1x1(monkeypatch, Cin, Cout):
    from deepatlas_amd import ops
    x, w, b = rnd((2, Cin, 4, 6, 10), 1), rnd((Cout, Cin, 1, 1, 1), 2, 0.3), rnd((Cout,), 3, 0.1)
    go = rnd((2, Cout, 4, 6, 10), 4)

    def fn():
        xg, wg, bg = cl(x).requires_grad_(True), w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
        y = ops.Conv1x1Fn.apply(xg, wg, bg)
        y.backward(cl(go))
        return [y.detach()] + _grads(xg, wg, bg)
    both(monkeypatch, fn, ('da_conv1x1_fwd', 'da_conv1x1_dgrad', 'da_conv1x1_wgrad'))


@pytest.mark.parametrize('dims', [(2, 5, 3, 7), (1, 8, 8, 16)], ids=lambda d: 'x'.join(map(str, d)))
def test_deconv_k2s2_bn_bwd(monkeypatch, dims):
    """The fused up-sampler backward and, in front of it, da_bn_train_stats and da_bn_act_bwd_dbias on the same tensors."""
    from deepatlas_amd import _native as nat
    from deepatlas_amd._native import call, ptr, stream
    N, D, H, W = dims
    C = 32
    g = torch.Generator().manual_seed(7)
    x = (torch.rand((N, D, H, W, C), generator=g) * 2 - 1).to(dev())
    w = (torch.rand((8, C, C), generator=g) * 0.4 - 0.2).to(dev())
    y = (torch.randn((N, 2 * D, 2 * H, 2 * W, C), generator=g) * 1.5 + 0.3).to(dev())
    go = (torch.rand((N, 2 * D, 2 * H, 2 * W, C), generator=g) * 2 - 1).to(dev())
    gamma, beta = (torch.rand(C, generator=g) * 1.5 - 0.5).to(dev()), (torch.rand(C, generator=g) - 0.5).to(dev())
    M = N * D * H * W * 8

    def fn():
        st = stream()
        stats = torch.empty((4, C), device=dev())
        rm, rv = torch.zeros(C, device=dev()), torch.ones(C, device=dev())
        wp, wn = nat.workspace.get(nat.lib().da_bn_ws_bytes(M, C), dev())
        call('da_bn_train_stats', ptr(y), M, C, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(rm), ptr(rv), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), wp, wn, st)
        dy, dgb = torch.empty_like(y), torch.empty((3, C), device=dev())
        wp, wn = nat.workspace.get(nat.lib().da_bn_ws_bytes(M, C), dev())
        call('da_bn_act_bwd_dbias', ptr(go), ptr(y), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), 0.01, 1, ptr(dy), ptr(dgb[1]), ptr(dgb[2]), ptr(dgb[0]), M, C, wp, wn, st)
        cs = torch.empty((C,), device=dev())
        wp, wn = nat.workspace.get(nat.lib().da_bn_ws_bytes(M, C), dev())
        call('da_colsum', ptr(dy), M, C, ptr(cs), wp, wn, st)
        dx1, dw1, dgb1 = torch.empty_like(x), torch.empty_like(w), torch.empty((3, C), device=dev())
        wp, wn = nat.workspace.get(nat.lib().da_deconv_k2s2_bn_bwd_ws_bytes(N, D, H, W, C, C), dev())
        call('da_deconv_k2s2_bn_bwd', ptr(go), ptr(y), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), 0.01, ptr(x), ptr(w), ptr(dx1), ptr(dw1),
             ptr(dgb1[0]), ptr(dgb1[1]), ptr(dgb1[2]), N, D, H, W, C, C, None, 0, wp, wn, st)
        return [stats, rm, rv, dy, dgb, cs, dx1, dw1, dgb1]
    both(monkeypatch, fn, ('da_bn_train_stats', 'da_bn_act_bwd_dbias', 'da_colsum', 'da_deconv_k2s2_bn_bwd'))


@pytest.mark.parametrize('C', [16, 5])
def test_batchnorm(monkeypatch, C):
    from deepatlas_amd import ops
    x = rnd((2, C, 6, 8, 10), 1, 2.0) + 0.5
    gamma, beta, go = 1 + rnd((C,), 2, 0.2), rnd((C,), 3, 0.2), rnd((2, C, 6, 8, 10), 6)

    def fn():
        xg, gg, bg = cl(x).requires_grad_(True), gamma.to(dev()).requires_grad_(True), beta.to(dev()).requires_grad_(True)
        rm, rv = torch.zeros(C, device=dev()), torch.ones(C, device=dev())
        y = ops.BNActFn.apply(xg, gg, bg, rm, rv, True, 0.1, 1e-5, 0.01)
        y.backward(cl(go))
        return [y.detach(), rm, rv] + _grads(xg, gg, bg)
    both(monkeypatch, fn, ('da_bn_train_stats',))


# ---- losses ------------------------------------------------------------------------------------------------------------------------------------
def _labels(N, shape, C, seed):
    return torch.from_numpy(edt_cases.blocky_labels(shape, C, seed=seed, n=N).astype(np.int64))


@pytest.mark.parametrize('Cin,C,N', [(16, 32, 2), (16, 32, 4), (64, 16, 2)], ids=['16-32-n2-bwd-larger', '16-32-n4-fwd-larger', '64-16'])
def test_head_dice(monkeypatch, Cin, C, N):
    """(16, 32): the backward layout is the larger one at N = 2, the forward layout at N = 4."""
    from deepatlas_amd import ops
    shape = (5, 9, 18)
    x, w, b = rnd((N, Cin) + shape, 1), rnd((C, Cin, 1, 1, 1), 2, 0.3), rnd((C,), 3, 0.1)
    lab = _labels(N, shape, C, 4)

    def fn():
        xg, wg, bg = cl(x).requires_grad_(True), w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
        loss = ops.HeadDiceFn.apply(xg, wg, bg, lab.to(dev()), 'Uniform', False, 1e-6)
        loss.backward()
        return [loss.detach()] + _grads(xg, wg, bg)
    both(monkeypatch, fn, ('da_head_dice_fwd', 'da_head_dice_bwd'))


@pytest.mark.parametrize('C', [32, 5])
def test_dice(monkeypatch, C):
    from deepatlas_amd import ops
    N, shape = 2, (5, 9, 18)
    x, lab = rnd((N, C) + shape, 1), _labels(N, shape, C, 2)

    def fn():
        xg = cl(x).requires_grad_(True)
        loss = ops.DiceFn.apply(xg, lab.to(dev()), None, 'Simple', False, True, 1e-6)
        loss.backward()
        return [loss.detach()] + _grads(xg)
    both(monkeypatch, fn, ('da_dice_fwd',))


def test_warp_dice_family(monkeypatch):
    """da_label_warp_dice_fwd, da_softwarp_dice_fwd (both roles), da_warp_dice_fwd and the deterministic data gradient of the warp."""
    from deepatlas_amd import _native as nat
    from deepatlas_amd._native import call, ptr, stream
    N, C, (D, H, W) = 2, 8, (5, 9, 18)
    lm, lt = _labels(N, (D, H, W), C, 5).to(torch.uint8).to(dev()), _labels(N, (D, H, W), C, 6).to(dev())
    disp = (rnd((N, D, H, W, 3), 7, 0.2)).to(dev())
    prob = torch.softmax(rnd((N, D, H, W, C), 8, 2.0), -1).contiguous().to(dev())
    dout = rnd((N, D, H, W, C), 9).to(dev())

    def fn():
        st = stream()
        res = []
        for name, args in (('da_label_warp_dice_fwd', (ptr(lm), 1, ptr(lt), 8, ptr(disp))),
                           ('da_softwarp_dice_fwd', (ptr(lm), 1, ptr(disp), ptr(prob), 0)),
                           ('da_softwarp_dice_fwd', (ptr(lm), 1, ptr(disp), ptr(prob), 1)),
                           ('da_warp_dice_fwd', (ptr(prob), ptr(disp), ptr(lt), 8))):
            loss, coef = torch.empty((1,), device=dev()), torch.empty((2, N, C), device=dev())
            wp, wn = nat.workspace.get(getattr(nat.lib(), name[:-4] + '_ws_bytes')(N, C), dev())
            call(name, *(args + (N, D, H, W, C, 0, 0, 1e-6, ptr(loss), ptr(coef), wp, wn, st)))
            res += [loss, coef]
        d_src = torch.empty_like(dout)
        wp, wn = nat.workspace.get(nat.lib().da_warp_bwd_dsrc_det_ws_bytes(N, D, H, W, C), dev())
        call('da_warp_bwd_dsrc_det', ptr(dout), ptr(disp), ptr(d_src), N, D, H, W, C, wp, wn, st)
        return res + [d_src]
    both(monkeypatch, fn, ('da_label_warp_dice_fwd', 'da_softwarp_dice_fwd', 'da_warp_dice_fwd', 'da_warp_bwd_dsrc_det'))


@pytest.mark.parametrize('F,dil', [(5, 1), (3, 1), (3, 2)], ids=['marching-F5', 'separable-F3', 'separable-dilated'])
def test_lncc(monkeypatch, F, dil):
    from deepatlas_amd import ops
    I, J = rnd((2, 1, 12, 14, 16), 1) * 0.5 + 0.5, rnd((2, 1, 12, 14, 16), 2) * 0.5 + 0.5

    def fn():
        a, b = I.to(dev()).requires_grad_(True), J.to(dev()).requires_grad_(True)
        loss = ops.LNCCFn.apply(a, b, F, 1e-5, dil, 1)
        loss.backward()
        return [loss.detach()] + _grads(a, b)
    both(monkeypatch, fn, ('da_lncc_fwd', 'da_lncc_bwd'))


@pytest.mark.parametrize('name', ['ragged', 'aligned'])
def test_mutual_information_forward(monkeypatch, name):
    from deepatlas_amd import ops
    N, shape, bins, sr, (vmin, vmax), _, _ = mi_cases.CASES[name]
    x, y = mi_cases.inputs(name)

    def fn():
        return [ops.MIFn.apply(x.to(dev()), y.to(dev()), bins, sr, vmin, vmax).detach()]
    both(monkeypatch, fn, ('da_mi_fwd',))


# ---- volumes and label maps -----------------------------------------------------------------------------------------------------------------------
def test_sample_crop_starts(monkeypatch):
    from deepatlas_amd import ops
    shape, window = crop_cases.MAIN
    lab = torch.from_numpy(crop_cases.ellipsoid_labels(shape, seed=0, n=2).copy())

    def fn():
        starts, info = ops.sample_crop_starts(lab.to(dev()), window, (1, 2, None), (crop_cases.min_count(0.05, int(np.prod(window))),) * 2 + (0,), seed=11)
        return [starts, info]
    both(monkeypatch, fn, ('da_crop_sample_starts',))


def test_signed_distance_maps(monkeypatch):
    from deepatlas_amd import ops
    lab = torch.from_numpy(edt_cases.blocky_labels((9, 10, 11), 4, seed=3, n=2))

    def fn():
        return [ops.signed_distance_maps(lab.to(dev()), 4, spacing=edt_cases.ANISO)]
    both(monkeypatch, fn, ('da_signed_distance_maps',))


def test_surface_distance_stats(monkeypatch):
    from deepatlas_amd import ops
    truth = edt_cases.blocky_labels((5, 6, 70), 4, block=surface_cases.BLOCK, seed=1, n=2)
    pred = surface_cases.noisy(truth, 4, seed=2)

    def fn():
        return [ops.surface_distance_stats(torch.from_numpy(pred).to(dev()), torch.from_numpy(truth).to(dev()), 4)]
    from deepatlas_amd import _native as nat
    ref = fn()
    g = Guarded()
    with monkeypatch.context() as m:
        m.setattr(nat.workspace, 'get', g.get)
        out = fn()
        g.check()
    # the gather's list order depends on the order its atomics land in, the statistics do not beyond the order of a double sum: the bound of the op's own test
    r, o = ref[0].cpu().numpy(), out[0].cpu().numpy()
    assert np.array_equal(np.isnan(r), np.isnan(o))
    assert np.allclose(np.nan_to_num(o), np.nan_to_num(r), rtol=surface_cases.STAT_RTOL, atol=0)


def test_volume_percentiles(monkeypatch):
    from deepatlas_amd import ops
    vol = rnd((9, 10, 11), 3, 5.0)

    def fn():
        return [torch.tensor(ops.volume_percentiles(vol.to(dev()), (1.0, 99.0)), dtype=torch.float64)]
    both(monkeypatch, fn, ('da_volume_percentiles',))


def test_invert_field(monkeypatch):
    from deepatlas_amd import ops
    u = invert_cases.field('17x30x22', 0.5)

    def fn():
        return list(ops.invert_field(u.to(dev()), return_stats=True))          # (the statistics are what needs the workspace)
    both(monkeypatch, fn, ('da_field_invert',))


def test_label_fusion_with_msd_weights(monkeypatch):
    from deepatlas_amd import ops
    case = fusion_cases.VOTE_CASES[2]                      # 24 x 40 x 56, one target, three atlases
    labels, disp = fusion_cases.vote_inputs(case)
    warped, target = fusion_cases.msd_inputs((case[0], 1, 3, 2, 0.2))

    def fn():
        wts = ops.local_msd_weights(warped.to(dev()), target.to(dev()), radius=2, sigma=0.2)
        fused, conf = ops.label_fusion(labels.to(dev()), disp.to(dev()), weights=wts, return_confidence=True)
        return [wts, fused, conf]
    both(monkeypatch, fn, ('da_local_msd_weights',))
