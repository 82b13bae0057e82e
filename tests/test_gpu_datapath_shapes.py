"""Randomised parity for the optimiser, layout, cast and data-path kernels (optim.hip, datapath.hip): da_adam_step / da_adam_step_dev / FlatAdam, the nine
da_w_* layout entry points, da_clamp01_to_f32, da_crop3d, da_partition_tiles, da_assemble_tiles (copy and vote), the bf16 casts and da_synth_volume.

Cases, builders, references and the launcher decisions (restated) live in tests/datapath_cases.py; every family runs `datapath_cases.run_cases` (the pinned cases,
then 60 derandomised ones).  tests/test_datapath_reference.py validates the references on the CPU.  Everything but Adam is compared bit for bit with numpy (or
torch on the CPU for the casts).  Every output buffer is prefilled (NaN / 0xFF) and carries 8 guard elements that must keep the prefill.  No graph capture in this
file: da_adam_step_dev is fed by da_adam_host_state through a 6-float device tensor and called directly.

Adam against the float64 reference (hyper-parameters as the float32 values the C ABI receives): after k steps from p0, with disp = p_ref - p0,
    |p_dev - p_ref| <= TOL * max|disp| + k * 2^-24 * max|p|
the second term the fp32 store of p once per step (derived, no margin), asserted after every step; m and v by dist() after the last.  da_adam_step_dev must be
bit-equal to da_adam_step in p, m, v after every step.

Tolerance table (distance from float64; p: the part of the error the store term does not cover, in units of max|disp|).  The device column is filled from one run
with DA_DATAPATH_SHAPES_REPORT set (profiles/datapath_shapes_report.json), the restatement column from the CPU companion's run of the same cases.
  quantity   device worst   fp32 restatement worst   ceiling   asserted
  adam p       2.41e-7          2.41e-7                1e-6      1e-6
  adam m       1.65e-7          1.65e-7                1e-6      1e-6
  adam v       2.27e-7          2.27e-7                1e-6      1e-6
The two columns agree in every printed digit: with contraction off, a correctly rounded sqrtf and division, the kernel IS the restatement.  The worst p is about
four fp32 roundings of the update (the two step scalars, m, the quotient).  max(4 x device, 8 x restatement) = 1.9e-6 is above the ceiling (test_adam_vs_oracle's
1e-6), so by the rule of tests/loss_cases.py the ceiling stays.
FlatAdam against torch's Adam: p 1.5e-8 (the store term covers nearly all of it at |p| ~ 0.1, lr 1e-3), m 2.9e-7, v 1.29e-5 -- the last is 1 - float32(0.999)
against 1 - 0.999, the by-construction amount itself, which the first step from zero moments shows in full.

FlatAdam is compared with torch.optim.Adam in float64, from which it differs BY CONSTRUCTION through the float32 hyper-parameters (test_datapath_reference.py derives
the amounts: v by 1.29e-5, the update by 6.7e-6 at betas (0.9, 0.999)): its bounds are the ones above plus 1.1 x those amounts.
"""
import ctypes

import numpy as np
import pytest
import torch

import datapath_cases as dc
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu
G = dc.GUARD


def _native():
    from deepatlas_amd import _native as nat
    return nat


def _up(a):
    return torch.from_numpy(np.array(a, order='C')).to(dev())          # (a copy: a flipped axis of length 1 keeps its negative stride otherwise)


def _guarded(a):
    """Device copy of a float32 array with G NaN guard elements behind it (an in-place buffer)."""
    buf = torch.full((a.size + G,), float('nan'), dtype=torch.float32, device=dev())
    buf[:a.size] = _up(a.reshape(-1))
    return buf


def _blank(n, dtype):
    """n + G elements of `dtype`, prefilled with NaN (floating types) or 0xFF bytes."""
    if dtype.is_floating_point:
        return torch.full((n + G,), float('nan'), dtype=dtype, device=dev())
    buf = torch.empty((n + G,), dtype=dtype, device=dev())
    buf.view(torch.uint8).fill_(0xFF)
    return buf


def _result(buf, n, shape=None):
    """The first n elements as numpy, after checking that the guard kept its prefill."""
    tail = buf[n:].cpu()
    assert tail.numel() == G
    if buf.dtype.is_floating_point:
        assert bool(torch.isnan(tail).all()), 'guard overwritten'
    else:
        assert bool((tail.view(torch.uint8) == 0xFF).all()), 'guard overwritten'
    out = buf[:n].cpu().numpy()
    return out.reshape(shape) if shape is not None else out


def _i3(v):
    arr = (ctypes.c_int * 3)(*[int(x) for x in v])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


# ---- Adam --------------------------------------------------------------------------------------------------------------------------
def test_adam_step_and_device_state_step_random_cases():
    nat = _native()
    tol = dc.TOL['adam']

    def body(case):
        inp, hyper, n = dc.build_adam(case), dc.adam_hyper(case), case['n']
        ref = dc.adam_ref_path(inp, hyper)
        A = [_guarded(inp[k]) for k in ('p0', 'm0', 'v0')]
        B = [_guarded(inp[k]) for k in ('p0', 'm0', 'v0')]
        state = torch.zeros(6, dtype=torch.float32, device=dev())
        lr, (b1, b2), eps, gs = case['lr'], case['betas'], case['eps'], case['gs']
        for k, g in enumerate(inp['grads']):
            step = case['t0'] + k + 1
            gd = _up(g)
            nat.call('da_adam_step', nat.ptr(A[0]), nat.ptr(gd), nat.ptr(A[1]), nat.ptr(A[2]), n, lr, b1, b2, eps, step, gs, nat.stream())
            host = (ctypes.c_float * 6)()
            nat.call('da_adam_host_state', lr, b1, b2, eps, step, gs, ctypes.cast(host, ctypes.c_void_p))
            got, want = np.array(list(host), dtype=np.float32), dc.adam_host_state(hyper, step)
            assert np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 1, (got, want)
            state.copy_(torch.tensor(list(host), dtype=torch.float32))
            nat.call('da_adam_step_dev', nat.ptr(B[0]), nat.ptr(gd), nat.ptr(B[1]), nat.ptr(B[2]), n, nat.ptr(state), nat.stream())
            for a, b, what in zip(A, B, 'pmv'):                                              # bit-equal, guards included
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'da_adam_step_dev differs from da_adam_step in %s after step %d' % (what, k + 1)
            e = dc.adam_p_excess(_result(A[0], n), inp['p0'], ref, k + 1)
            dc.note('adam', 'p', e)
            assert e <= tol['p'], 'p after %d steps: %.3e of max|disp| beyond the store term (tolerance %.1e)' % (k + 1, e, tol['p'])
        for j, what in ((1, 'm'), (2, 'v')):
            e = dc.dist(_result(A[j], n), ref[-1][j])
            dc.note('adam', what, e)
            assert e <= tol[what], '%s: %.3e (tolerance %.1e)' % (what, e, tol[what])
    dc.run_cases(dc.ADAM, body, dc.ADAM_PINNED)


class _Shift(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bias = torch.nn.Parameter(torch.linspace(-1, 1, 6))


class _Net(torch.nn.Module):
    """One tagged Conv3d weight, one tagged ConvTranspose3d(k = 2) weight, a BatchNorm3d and a bias-only parameter, the LAST of the parameter list."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv3d(3, 5, 3)
        self.up = torch.nn.ConvTranspose3d(5, 4, 2, stride=2, bias=False)
        self.bn = torch.nn.BatchNorm3d(4)
        self.tail = _Shift()


_LRS = (1e-3, 1e-3, 3e-4, 3e-4)          # lr changed before step 3
_GSCALE = (1.0, 0.5, 1.0, 1.0)           # grad_scale = 0.5 on one step


LAST = 'tail.bias'


def _fresh_net(state=None, frozen=None):
    torch.manual_seed(11)
    net = _Net()
    assert [n for n, _ in net.named_parameters()][-1] == LAST
    with torch.no_grad():
        net.bn.weight.copy_(torch.linspace(0.5, 1.5, 4))
    if state is not None:
        net.load_state_dict(state)
    if frozen is not None:
        dict(net.named_parameters())[frozen].requires_grad_(False)
    return net


def _grad_of(name, p, step):
    g = torch.Generator().manual_seed(1000 * step + sum(map(ord, name)))
    return (torch.rand(p.shape, generator=g) * 2 - 1) * 0.1


def _flat_adam(net):
    from deepatlas_amd import ops
    from deepatlas_amd.optim import FlatAdam
    net.to(dev())
    ops.tag_conv_layouts(net)
    return FlatAdam(net.parameters(), lr=_LRS[0])


def _flat_step(net, opt, step):
    opt.param_groups[0]['lr'] = _LRS[step]
    opt.zero_grad()
    for name, p in net.named_parameters():
        if p.requires_grad:
            p.grad.copy_(_grad_of(name, p, step).to(dev()))
    opt.step(grad_scale=_GSCALE[step])


def _snapshot(net, opt):
    """{name: (p, exp_avg, exp_avg_sq, step)} as CPU tensors in the module's own shapes, from state_dict()."""
    sd = opt.state_dict()
    out = {}
    for i, (name, p) in enumerate(net.named_parameters()):
        st = sd['state'][i]
        assert tuple(st['exp_avg'].shape) == tuple(p.shape) == tuple(st['exp_avg_sq'].shape)
        out[name] = (p.detach().cpu().clone(), st['exp_avg'].detach().cpu().clone(), st['exp_avg_sq'].detach().cpu().clone(), float(st['step']))
    return out


def _copy_state_dict(sd):
    return {'state': {i: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in sd['state'].items()},
            'param_groups': [dict(g) for g in sd['param_groups']]}


@pytest.mark.parametrize('native_tio', [True, False])
@pytest.mark.parametrize('frozen', [None, 'conv.weight', LAST])
def test_flat_adam_against_torch_adam_in_float64(native_tio, frozen):
    from deepatlas_amd import ops
    prev, ops.NATIVE_TIO = ops.NATIVE_TIO, native_tio
    try:
        net = _fresh_net(frozen=frozen)
        twin = _fresh_net(frozen=frozen).double()
        p0 = {n: p.detach().clone() for n, p in twin.named_parameters()}
        pmax = {n: float(p.abs().max()) for n, p in p0.items()}
        topt = torch.optim.Adam([p for p in twin.parameters()], lr=_LRS[0])
        opt = _flat_adam(net)
        d1, d2, dup = (max(v) for v in zip(*[dc.adam_hyper_dev((0.9, 0.999), lr) for lr in set(_LRS)]))
        tol = dc.TOL['adam']
        dc.lc._state['case'] = 'FlatAdam, frozen=%s, NATIVE_TIO=%s' % (frozen, native_tio)          # (what the report names next to a worst figure)
        for step in range(4):
            _flat_step(net, opt, step)
            topt.param_groups[0]['lr'] = _LRS[step]
            for name, p in twin.named_parameters():
                p.grad = _grad_of(name, p, step).double() * _GSCALE[step] if p.requires_grad else None
            topt.step()
            snap = _snapshot(net, opt)
            for name, p in twin.named_parameters():
                got_p, got_m, got_v, got_step = snap[name]
                if name == frozen:                                                          # untouched, as in torch (which keeps no state for it)
                    assert torch.equal(got_p.double(), p0[name]) and not got_m.any() and not got_v.any() and got_step == 0 and p not in topt.state
                    continue
                pmax[name] = max(pmax[name], float(p.detach().abs().max()))
                disp = float((p.detach() - p0[name]).abs().max())
                over = float((got_p.double() - p.detach()).abs().max()) - (step + 1) * 2.0 ** -24 * pmax[name]
                e = max(over, 0.0) / disp
                dc.note('flatadam', 'p', e)
                assert e <= tol['p'] + 1.1 * dup, (name, step, e)
                st = topt.state[p]
                for got, ref, what, d in ((got_m, st['exp_avg'], 'm', d1), (got_v, st['exp_avg_sq'], 'v', d2)):
                    e = dc.dist(got, ref)
                    dc.note('flatadam', what, e)
                    assert e <= tol[what] + 1.1 * d, (name, step, what, e)
                assert got_step == step + 1 == float(st['step'])
    finally:
        ops.NATIVE_TIO = prev
    dc.write_report()


@pytest.mark.parametrize('frozen', [None, 'conv.weight', LAST])
def test_flat_adam_resume_is_bit_equal_to_the_uninterrupted_run(frozen):
    """state_dict() after step 2 into a fresh model and a fresh FlatAdam: steps 3 and 4 bit-equal to the run that never stopped.  'tail.bias' is the LAST parameter:
    frozen, its step count is 0, and a load_state_dict that takes the last parameter's count resumes every parameter with the bias correction of step 1."""
    net = _fresh_net(frozen=frozen)
    opt = _flat_adam(net)
    for step in range(2):
        _flat_step(net, opt, step)
    model_sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    opt_sd = _copy_state_dict(opt.state_dict())
    for step in (2, 3):
        _flat_step(net, opt, step)
    whole = _snapshot(net, opt)
    net2 = _fresh_net(state=model_sd, frozen=frozen)
    opt2 = _flat_adam(net2)
    opt2.load_state_dict(opt_sd)
    for step in (2, 3):
        _flat_step(net2, opt2, step)
    resumed = _snapshot(net2, opt2)
    for name in whole:
        for a, b, what in zip(whole[name][:3], resumed[name][:3], ('p', 'exp_avg', 'exp_avg_sq')):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), '%s %s differs after the resume' % (name, what)
        assert whole[name][3] == resumed[name][3] == (0 if name == frozen else 4)


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
def test_layout_entry_points_random_shapes():
    nat = _native()

    def body(case):
        A, B, K = case['A'], case['B'], case['K3']
        n = A * B * K
        for name, (shape_of, _) in dc.LAYOUT.items():
            src = dc.distinct(shape_of(A, B, K), case['sd'])
            dst = _blank(n, torch.float32)
            nat.call(name, nat.ptr(_up(src)), nat.ptr(dst), A, B, K, nat.stream())
            ref = dc.layout_ref(name, src)
            assert np.array_equal(_result(dst, n, ref.shape), ref), name
        for name in dc.LAYOUT_ACC:
            src = dc.distinct(dc.LAYOUT[name[:-4]][0](A, B, K), case['sd'] + 1)
            before = np.random.default_rng(case['sd']).uniform(-1, 1, n).astype(np.float32)
            ref = dc.layout_ref(name, src, before.reshape(dc.layout_ref(name[:-4], src).shape))
            dst = _guarded(before)
            nat.call(name, nat.ptr(_up(src)), nat.ptr(dst), A, B, K, nat.stream())
            assert np.array_equal(_result(dst, n, ref.shape), ref), name
    dc.run_cases(dc.LAYOUT_CASES, body, dc.LAYOUT_PINNED)


@pytest.mark.parametrize('kind', ['oik', 'iok', 'iok_flip'])
def test_ops_weight_tio_and_grad_from_tio(kind):
    from deepatlas_amd import ops
    for sd, (a, b, k) in enumerate([(5, 3, 3), (3, 5, 3), (16, 48, 2), (7, 1, 1), (40, 17, 3)]):
        w = dc.distinct((a, b, k, k, k), sd)
        tio = dc.layout_ref('da_w_%s_to_tio' % kind, w.reshape(a, b, k ** 3))
        got = ops.weight_tio(_up(w), kind)
        assert tuple(got.shape) == tio.shape and np.array_equal(got.cpu().numpy(), tio)
        back = ops.grad_from_tio(_up(tio), kind, w.shape)
        assert tuple(back.shape) == w.shape and np.array_equal(back.cpu().numpy(), w)
        before = np.random.default_rng(sd).uniform(-1, 1, w.shape).astype(np.float32)
        acc = _up(before)
        assert ops.grad_from_tio(_up(tio), kind, w.shape, acc=acc) is None
        assert np.array_equal(acc.cpu().numpy(), before + w)


def test_k2s2_conv_weight_gradient_call_da_w_tio_to_iok_on_swapped_roles():
    """ops.py's stride-2 convolution backward hands da_w_tio_to_iok a [8][Cout][Cin] gradient with (Cout, Cin) in the (Cin, Cout) slots, on purpose:
    [8][Cout][Cin] -> [Cout][Cin][8], the Conv3d weight's layout."""
    nat = _native()
    for Cout, Cin in ((5, 3), (16, 48), (1, 7)):
        src = dc.distinct((8, Cout, Cin), Cout)
        dst = _blank(8 * Cout * Cin, torch.float32)
        nat.call('da_w_tio_to_iok', nat.ptr(_up(src)), nat.ptr(dst), Cout, Cin, 8, nat.stream())
        assert np.array_equal(_result(dst, 8 * Cout * Cin, (Cout, Cin, 8)), np.ascontiguousarray(src.transpose(1, 2, 0)))


# ---- clamp -------------------------------------------------------------------------------------------------------------------------
def test_clamp_kernel_random_cases():
    nat = _native()

    def body(case):
        a = dc.clamp_values(dc.CLAMP_DTYPES[case['code']], case['n'], case['sd'])
        dst = _blank(case['n'], torch.float32)
        nat.call('da_clamp01_to_f32', nat.ptr(_up(a)), case['code'], nat.ptr(dst), case['n'], nat.stream())
        assert dc.same_bits(_result(dst, case['n']), dc.clamp_ref(a))
    dc.run_cases(dc.CLAMP, body, dc.CLAMP_PINNED)


def test_sitk_to_tensor_clamps_in_the_source_dtype():
    """Every dtype torch.from_numpy yields, as a numpy array, a host tensor and a device tensor: the clamp happens in the source dtype, then the cast
    (int64 -2^32 + 1 -> 0, 2^32 -> 1, uint32 2^31 + 5 -> 1: a narrowing ahead of the clamp gets all three wrong)."""
    from deepatlas_amd.lib import transforms as TR

    def body(case):
        a = dc.clamp_values(case['dtype'], int(np.prod(case['vol'])), case['sd']).reshape(case['vol'])
        given = a.copy() if case['as_tensor'] == 'numpy' else torch.from_numpy(a.copy())
        if case['as_tensor'] == 'device':
            given = given.to(dev())
        out = TR.SitkToTensor()({'image': given})['image']
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (1,) + tuple(case['vol'])
        assert dc.same_bits(out.cpu().numpy()[0], dc.clamp_ref(a)), (case, out.cpu().numpy()[0].ravel()[:12], dc.clamp_ref(a).ravel()[:12])
    dc.run_cases(dc.SITK, body, dc.SITK_PINNED)


# ---- crop --------------------------------------------------------------------------------------------------------------------------
def test_crop_kernel_and_transform_random_cases():
    nat = _native()
    from deepatlas_amd.lib import transforms as TR

    def body(case):
        D, H, W = case['vol']
        c = case['crop']
        a = dc.crop_values((case['lead'], D, H, W), case['bytes'], case['sd'])
        ref = dc.crop_ref(a, c)
        shape = dc.crop_out_shape(case)
        assert ref.shape == shape
        n = int(np.prod(shape))
        dst = _blank(n, torch.float32 if case['bytes'] == 4 else torch.uint8)
        nat.call('da_crop3d', nat.ptr(_up(a)), nat.ptr(dst), case['bytes'], case['lead'], D, H, W, c[0], c[1], c[2], shape[1], shape[2], shape[3], nat.stream())
        assert np.array_equal(_result(dst, n, shape), ref)
        seg = np.random.default_rng(case['sd'] + 1).integers(0, 256, (D, H, W)).astype(np.uint8)
        sizes = [list(c)] + ([list(c[:3])] if tuple(c[:3]) == tuple(c[3:]) else [])          # the 6-value form, and the 3-value form where it says the same
        for cs in sizes:
            out = TR.CropTensor(cs)({'image': _up(a), 'segmentation': torch.from_numpy(seg)})
            assert out['image'].is_contiguous() and np.array_equal(out['image'].cpu().numpy(), ref)
            assert np.array_equal(out['segmentation'].cpu().numpy(), dc.crop_ref(seg[None], c)[0])
    dc.run_cases(dc.CROP, body, dc.CROP_PINNED)


def test_crop_tensor_keeps_eight_byte_integers_exact():
    from deepatlas_amd.lib import transforms as TR
    rng = np.random.default_rng(3)
    img = dc.distinct((2, 5, 6, 7), 1)
    for dtype, values in ((np.int64, [2 ** 40 + 3, -2 ** 33 - 1, 2 ** 31, -2 ** 63, 2 ** 63 - 1, 7]), (np.uint64, [2 ** 63 + 5, 2 ** 32, 3])):
        seg = np.array(values, dtype=dtype)[rng.integers(0, len(values), (5, 6, 7))]
        for given in (torch.from_numpy(seg.copy()), torch.from_numpy(seg.copy()).to(dev())):
            out = TR.CropTensor([1, 0, 2, 1, 2, 1])({'image': _up(img), 'segmentation': given})['segmentation']
            assert np.array_equal(out.cpu().numpy(), seg[1:4, 0:4, 2:6]) and out.cpu().numpy().dtype == dtype


# ---- partition / assemble / vote ---------------------------------------------------------------------------------------------------
def _dtype_of(nbytes):
    return torch.float32 if nbytes == 4 else torch.uint8


def test_partition_kernel_and_transform_random_cases():
    nat = _native()
    from deepatlas_amd.lib import transforms as TR

    def body(case):
        D, H, W = case['vol']
        vol = dc.volume_values(case)
        ref = dc.partition_ref(case, vol)
        dst = _blank(ref.size, _dtype_of(case['bytes']))
        (ka, ta), (kb, ov) = _i3(case['tile']), _i3(case['ov'])
        nat.call('da_partition_tiles', nat.ptr(_up(vol)), nat.ptr(dst), case['bytes'], D, H, W, ta, ov, nat.stream())
        assert np.array_equal(_result(dst, ref.size, ref.shape), ref)
        if ref.size > 200000:
            return
        img, seg = dc.volume_values(dict(case, bytes=4)), dc.volume_values(dict(case, bytes=1))
        part = TR.Partition(tuple(reversed(case['tile'])), tuple(reversed(case['ov'])), mode='eval')
        out = part({'image': img.copy(), 'segmentation': torch.from_numpy(seg.copy()), 'name': 'x'})
        assert np.array_equal(out['image'].cpu().numpy()[:, 0], dc.partition_ref(case, img)) and out['image'].dtype == torch.float32
        assert np.array_equal(out['segmentation'].cpu().numpy()[:, 0], dc.partition_ref(case, seg)) and out['segmentation'].dtype == torch.uint8
        assert np.array_equal(part.assemble(out['image'][:, 0]).cpu().numpy(), img)
    dc.run_cases(dc.GEOM, body, dc.PARTITION_PINNED)


def test_assemble_copy_random_cases():
    nat = _native()

    def body(case):
        D, H, W = case['vol']
        vol = dc.volume_values(case)
        tiles = dc.partition_brute(case, vol)
        # (what the assemble must NOT read: everything outside the tiles' cores is replaced, so that a wrong offset shows)
        eff, _ = dc.geom(case)
        core = np.zeros(case['tile'], dtype=bool)
        core[tuple(slice(o, o + e) for o, e in zip(case['ov'], eff))] = True
        tiles = np.where(core[None], tiles, tiles.dtype.type(201)).astype(tiles.dtype)
        ref = dc.assemble_ref(case, tiles)
        assert np.array_equal(ref, vol)
        dst = _blank(vol.size, _dtype_of(case['bytes']))
        (ka, ta), (kb, ov) = _i3(case['tile']), _i3(case['ov'])
        nat.call('da_assemble_tiles', nat.ptr(_up(tiles)), nat.ptr(dst), case['bytes'], D, H, W, ta, ov, 0, nat.stream())
        assert np.array_equal(_result(dst, vol.size, vol.shape), ref)
    dc.run_cases(dc.GEOM, body, dc.ASSEMBLE_PINNED)


def test_assemble_vote_random_cases():
    nat = _native()
    from deepatlas_amd.lib import transforms as TR
    seen = dict(declined=0, ran=0)

    def body(case):
        D, H, W = case['vol']
        tiles = dc.noisy_tiles(case)
        dst = _blank(D * H * W, torch.uint8)
        (ka, ta), (kb, ov) = _i3(case['tile']), _i3(case['ov'])
        part = TR.Partition(tuple(reversed(case['tile'])), tuple(reversed(case['ov'])), mode='eval')
        part._geom(case['vol'])
        if dc.cover_bound(case) > 64:                                                       # declines: an error, never a volume, nothing written
            seen['declined'] += 1
            rc = nat.lib().da_assemble_tiles(nat.ptr(_up(tiles)), nat.ptr(dst), 1, D, H, W, ta, ov, 1, nat.stream())
            assert rc == -3
            torch.cuda.synchronize()
            assert bool((dst == 0xFF).all())
            with pytest.raises(nat.NativeError, match='DA_ERR_UNSUPPORTED'):
                part.assemble(_up(tiles), is_vote=True)
            return
        seen['ran'] += 1
        ref = dc.vote_ref(case, tiles)
        nat.call('da_assemble_tiles', nat.ptr(_up(tiles)), nat.ptr(dst), 1, D, H, W, ta, ov, 1, nat.stream())
        assert np.array_equal(_result(dst, D * H * W, (D, H, W)), ref)
        if tiles.size < 200000:
            assert np.array_equal(part.assemble(_up(tiles), is_vote=True).cpu().numpy(), ref)
            assert np.array_equal(part.assemble(_up(tiles.astype(np.int64)), is_vote=True).cpu().numpy(), ref)
    dc.run_cases(dc.VOTE, body, dc.VOTE_PINNED)
    assert seen['declined'] >= 1 and seen['declined'] <= 1 + dc.VOTE_DECLINE_MAX and seen['ran'] >= len(dc.VOTE_PINNED) - 1 + 54


def test_partition_converts_wide_integers_exactly_or_refuses_by_name():
    from deepatlas_amd.lib import transforms as TR
    case = dict(vol=(5, 6, 7), tile=(4, 4, 5), ov=(1, 0, 2), bytes=4, sd=2)
    img = dc.volume_values(case)
    small = np.random.default_rng(1).integers(-2 ** 31, 2 ** 31, case['vol']).astype(np.int64)
    small.reshape(-1)[:2] = [-2 ** 31, 2 ** 31 - 1]
    part = TR.Partition(tuple(reversed(case['tile'])), tuple(reversed(case['ov'])), mode='eval')
    out = part({'image': img.copy(), 'segmentation': small.copy(), 'name': 'x'})
    assert np.array_equal(out['segmentation'].cpu().numpy()[:, 0].astype(np.int64), dc.partition_brute(case, small))
    back = part.assemble(_up(dc.partition_brute(case, small)))
    assert np.array_equal(back.cpu().numpy().astype(np.int64), small)
    wide = small.copy()
    wide[2, 3, 4] = 2 ** 32 + 7
    for bad, key in ((wide, 'segmentation'), (wide, 'image')):
        sample = {'image': img.copy(), 'segmentation': small.copy(), 'name': 'x'}
        sample[key] = bad.copy()
        with pytest.raises(ValueError, match='int64'):
            part(sample)
    with pytest.raises(ValueError, match='int64'):
        part.assemble(_up(dc.partition_brute(case, wide)))
    exact = np.random.default_rng(2).integers(-2 ** 24, 2 ** 24 + 1, case['vol']).astype(np.int64)       # an int64 image every value of which float32 holds
    out = part({'image': exact.copy(), 'segmentation': small.copy(), 'name': 'x'})
    assert out['image'].dtype == torch.float32 and np.array_equal(out['image'].cpu().numpy()[:, 0].astype(np.int64), dc.partition_brute(case, exact))
    # the vote takes labels 0 ... 255: 256 and -1 are refused by name, never wrapped
    vcase = dict(case, bytes=1, labels=(0, 1, 2))
    tiles = dc.noisy_tiles(vcase)
    part._geom(case['vol'])
    for dtype, value in ((np.int64, 256), (np.int32, 2 ** 16 + 1), (np.int16, -1), (np.int64, 2 ** 32)):
        t = tiles.astype(dtype)
        t[0, 1, 1, 1] = value
        with pytest.raises(ValueError, match=str(np.dtype(dtype))):
            part.assemble(_up(t), is_vote=True)


# ---- casts -------------------------------------------------------------------------------------------------------------------------
def test_bf16_casts_random_cases():
    nat = _native()

    def body(case):
        n = case['n']
        x = dc.cast_values(case)
        y = _blank(n, torch.int16)
        nat.call('da_cast_f32_to_bf16', nat.ptr(_up(x)), nat.ptr(y), n, nat.stream())
        got = _result(y, n).view(np.uint16)
        assert dc.same_bf16(got, dc.bf16_bits_ref(x)), np.flatnonzero(got != dc.bf16_bits_ref(x))[:8]
        b = dc.bf16_values(case)
        z = _blank(n, torch.float32)
        nat.call('da_cast_bf16_to_f32', nat.ptr(_up(b.view(np.int16))), nat.ptr(z), n, nat.stream())
        assert dc.same_bits(_result(z, n), dc.f32_from_bf16_ref(b))
    dc.run_cases(dc.CAST, body, dc.CAST_PINNED)


# ---- synthetic volumes ---------------------------------------------------------------------------------------------------------------
def test_synth_volume_random_cases():
    nat = _native()
    seen = dict(crossed=0)

    def body(case):
        N, (D, H, W) = case['N'], case['vol']
        n = N * D * H * W
        seen['crossed'] += dc.synth_crosses(case)
        img = _blank(n, torch.float32) if case['which'] in ('both', 'img') else None
        lab = _blank(n, torch.uint8) if case['which'] in ('both', 'lab') else None
        nat.call('da_synth_volume', nat.ptr(img), nat.ptr(lab), N, D, H, W, case['C'], case['mode'], case['noise'], case['seed'], case['sample0'], nat.stream())
        ri, rl = dc.synth_ref(case)
        if img is not None:
            assert dc.same_bits(_result(img, n, ri.shape), ri)
        if lab is not None:
            assert np.array_equal(_result(lab, n, rl.shape), rl)
    dc.run_cases(dc.SYNTH, body, dc.SYNTH_PINNED)
    assert seen['crossed'] >= 4
