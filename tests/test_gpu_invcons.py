"""GPU: the inverse-consistency kernels (invcons.hip) against the float64 reference of tests/invcons_cases.py, and the penalty inside the
registration step and experiment.  Every bound comes from invcons_cases.bounds(): 4 x the float32 torch evaluation's own distance from
float64, floors 5e-7 (loss, mean residual: relative) and 2e-6 (residual, its maximum, both gradients: max norm over the quantity's max).

Worst case on one MI355X over the 24 cases (distance from float64 / its bound; the float32 torch evaluation's own distance for comparison):
    quantity                      device      bound     float32 torch   case
    one way  loss (relative)      6.8e-08     5.0e-07   1.6e-08         2x2x2, 0.3 voxels
             sum |s r|^2 per sample 4.7e-08   5.0e-07   2.6e-08         7x9x66, 2
             mean |s r|           1.9e-08     5.0e-07   6.3e-09         2x2x2, 0.3
             max |s r|            1.1e-06     2.0e-06   9.3e-08         33x47x61, 8
             residual             3.3e-06     1.2e-05   3.0e-06         33x47x61, 2
             d u_a                4.7e-06     1.8e-05   4.4e-06         33x47x61, 2
             d u_b (atomics)      2.9e-06     6.7e-06   1.7e-06         7x9x66, 2
    symmetric loss                8.2e-08     5.0e-07   3.1e-08         80x96x80, 0.3
             d u_a                4.7e-06     1.7e-05   4.3e-06         33x47x61, 2
             d u_b                4.6e-06     1.3e-05   3.3e-06         33x47x61, 0.3
(worst = the largest share of its bound; the outside counts are equal to the last voxel on every case.)  Lattice case: loss 8.7e-08, residual
1.8e-07, d u_b 4.5e-07; translation pair: 8.9e-07 voxels inside the volume; descent: L_sym 21.33 -> 0.46, the float64 twin's figures.
"""
import math

import pytest
import torch

import invcons_cases as ic
import warp_cases as wc
from deepatlas_amd import ops as _ops

assert _ops.InverseConsistencyFn          # this file is about the feature: without it, it does not import

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def _one_way(u_a, u_b, grads='both', upstream=1.0):
    """One direction on the device: the dict invcons_cases.evaluate returns (loss, stats, resid from the forward entry; d_a / d_b through
    InverseConsistencyFn, None where that side's gradient is switched off)."""
    from deepatlas_amd import ops
    a = u_a.to(dev()).requires_grad_(grads in ('both', 'a'))
    b = u_b.to(dev()).requires_grad_(grads in ('both', 'b'))
    loss0, stats, resid = ops.inverse_consistency_forward(a, b)
    loss = ops.InverseConsistencyFn.apply(a, b)
    (loss * upstream if upstream != 1.0 else loss).backward()
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and loss.dim() == 0 and torch.allclose(loss.detach(), loss0, rtol=0, atol=0, equal_nan=True)          # bit for bit
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (u_a.shape[0], 4)
    return dict(loss=float(loss.detach()), stats=stats.cpu(), resid=resid.cpu(), d_a=None if a.grad is None else a.grad.cpu(),
                d_b=None if b.grad is None else b.grad.cpu())


def _symmetric(u_a, u_b, symmetric=True):
    from deepatlas_amd.lib.loss import InverseConsistencyLoss
    a, b = u_a.to(dev()).requires_grad_(True), u_b.to(dev()).requires_grad_(True)
    loss = InverseConsistencyLoss(symmetric=symmetric)(a, b)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=float(loss.detach()), d_a=a.grad.cpu(), d_b=b.grad.cpu())


def _show(what, d, bound):
    print('%s: %s' % (what, '  '.join('%s %.2e (bound %.1e)' % (k, v, bound[k]) for k, v in d.items())))


# ---- kernel parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,amp', ic.COMBOS, ids=ic.COMBO_IDS)
def test_one_direction_matches_the_float64_reference(name, amp):
    """Loss, the four statistics, the saved residual and both gradients; then either side's gradient switched off: the gather is the same bit
    for bit, the scatter (atomics: arrival order) within the same bound; and symmetric=False of the module is this direction."""
    u_a, u_b = ic.fields(name, amp)
    want, _ = ic.reference(name, amp)
    bound = ic.bounds(name, amp, False)
    got = _one_way(u_a, u_b)
    assert got['d_a'].dtype == torch.float32 and got['d_a'].shape == u_a.shape and got['d_b'].shape == u_b.shape
    _show('%s amp %g' % (name, amp), ic.check(ic.one_way_distances(got, want), bound, 'both gradients'), bound)
    only_a, only_b = _one_way(u_a, u_b, 'a'), _one_way(u_a, u_b, 'b')
    assert only_a['d_b'] is None and only_b['d_a'] is None
    assert torch.equal(only_a['d_a'], got['d_a']) and only_a['loss'] == got['loss'] == only_b['loss']
    ic.check(ic.one_way_distances(only_b, want), bound, 'd_b alone')
    mod = _symmetric(u_a, u_b, symmetric=False)
    assert mod['loss'] == got['loss'] and torch.equal(mod['d_a'], got['d_a'])
    ic.check(ic.symmetric_distances(mod, want), bound, 'symmetric=False')


@pytest.mark.parametrize('name,amp', ic.COMBOS, ids=ic.COMBO_IDS)
def test_symmetric_loss_matches_the_float64_reference(name, amp):
    """L_sym and its gradients, twice: the atomic route's run-to-run spread has to fit inside the same bound."""
    u_a, u_b = ic.fields(name, amp)
    _, want = ic.reference(name, amp)
    bound = ic.bounds(name, amp, True)
    runs = [_symmetric(u_a, u_b) for _ in range(2)]
    for got in runs:
        _show('%s amp %g symmetric' % (name, amp), ic.check(ic.symmetric_distances(got, want), bound, 'symmetric'), bound)
    assert runs[0]['loss'] == runs[1]['loss']
    for k in ('d_a', 'd_b'):
        assert ic.rel_max(runs[0][k], runs[1][k].double()) <= bound[k]


@pytest.mark.parametrize('name', ic.IDS)
def test_upstream_gradient_and_the_channels_last_layout(name):
    """-2.5 x L from channels-last fields (the layout the registration net produces): the same loss, -2.5 x the gradients."""
    amp = ic.AMPS[ic.IDS.index(name) % 3]
    u_a, u_b = ic.fields(name, amp)
    want, _ = ic.reference(name, amp)
    bound = ic.bounds(name, amp, False)
    cl = lambda t: t.to(dev()).contiguous(memory_format=torch.channels_last_3d)
    got = _one_way(cl(u_a), cl(u_b), upstream=-2.5)
    assert got['loss'] == _one_way(u_a, u_b)['loss']
    want = dict(want, d_a=-2.5 * want['d_a'], d_b=-2.5 * want['d_b'])
    ic.check(ic.one_way_distances(got, want), bound, 'upstream -2.5')


def test_zero_fields_give_exact_zeros():
    u_a, u_b = ic.lattice_fields('zero')
    got = _one_way(u_a, u_b)
    assert got['loss'] == 0.0
    for k in ('stats', 'resid', 'd_a', 'd_b'):
        assert not bool(got[k].any()), k
    sym = _symmetric(u_a, u_b)
    assert sym['loss'] == 0.0 and not bool(sym['d_a'].any()) and not bool(sym['d_b'].any())


def test_lattice_case_is_held_on_either_side():
    """u_a = 0: every sample point is a lattice point, where component k of d u_a jumps with the cell p_k falls in.  d u_a is held element-wise
    to the float64 value on either side; everything else is continuous there and compared plainly.  The bounds are those of the case of the
    same size and amplitude (5x7x29 at 2 voxels: the same generator made u_b)."""
    u_a, u_b = ic.lattice_fields('ua0')
    want = ic.evaluate(u_a, u_b, torch.float64)
    bound = ic.bounds('5x7x29', 2.0, False)
    got = _one_way(u_a, u_b)
    left, right = ic.lattice_sides(u_a, u_b)
    wc.close_either('invcons', 'd_a', got['d_a'], left, right, bound['d_a'])
    plain = dict(got, d_a=None)
    _show('lattice', ic.check(ic.one_way_distances(plain, want), bound, 'lattice'), bound)


def test_translation_pair_is_consistent_inside_the_volume():
    u_a, u_b = ic.translation_fields()
    D, H, W = ic.TRANSLATION_VOL
    got = _one_way(u_a, u_b)
    e = (got['resid'].double() * ic.scales(ic.TRANSLATION_VOL, torch.float64)).abs().amax(1)          # N x D x H x W, voxels
    print('largest residual inside %.2e voxels; outside %s' % (float(e[..., :W - 2].max()), got['stats'][:, 3].tolist()))
    assert float(e[..., :W - 2].max()) <= ic.TRANSLATION_TOL_VOX
    assert got['stats'][:, 3].tolist() == [2.0 * D * H] * ic.TRANSLATION_N          # the two border columns
    want = ic.evaluate(u_a, u_b, torch.float64)
    # everything else against float64: an error of TRANSLATION_TOL_VOX in a residual whose largest value is the shift itself (both taps outside)
    tol = ic.TRANSLATION_TOL_VOX / ic.TRANSLATION_SHIFT
    assert abs(got['loss'] - want['loss']) <= 2 * tol * want['loss']
    assert float((got['stats'][:, 2] - want['stats'][:, 2]).abs().max()) <= ic.TRANSLATION_TOL_VOX
    for k in ('d_a', 'd_b'):
        assert ic.rel_max(got[k], want[k]) <= tol, k


@pytest.mark.parametrize('value', ic.NONFINITE_VALUES)
def test_a_bad_field_does_not_pass_as_consistent(value):
    from deepatlas_amd import ops
    u_a, u_b = ic.nonfinite_fields(value)
    got = _one_way(u_a, u_b)
    assert not math.isfinite(got['loss'])
    assert not math.isfinite(_symmetric(u_a, u_b)['loss'])
    s = ops.inverse_consistency_stats(u_a.to(dev()), u_b.to(dev()))
    assert not math.isfinite(float(s['mean_vox'][1])) and float(s['max_vox'][1]) == float('inf') and math.isfinite(float(s['mean_vox'][0]))
    # the voxel itself samples nothing and counts as outside; no other voxel's gradient is touched by it
    clean = _one_way(*ic.fields('2x3x5', 2.0))
    assert got['stats'][1, 3] >= clean['stats'][1, 3] and torch.equal(got['stats'][0], clean['stats'][0])
    same = torch.ones_like(got['d_a'], dtype=torch.bool)
    same[1, :, 1, 2, 3] = False
    assert torch.equal(got['d_a'][same], clean['d_a'][same])
    assert bool(torch.isnan(got['d_a'][1, :, 1, 2, 3]).all())       # the refused voxel's own gradient is NaN, like its loss term
    assert bool(torch.isfinite(got['d_b']).all())                   # ... and it samples nothing: no add to d u_b


def test_c_abi_error_codes_on_the_device():
    from deepatlas_amd import _native
    from deepatlas_amd._native import ptr, stream
    L = _native.lib()
    N, D, H, W = 1, 4, 5, 6
    a = torch.zeros(N, D, H, W, 3, device=dev())
    loss = torch.zeros(1, device=dev())
    ws = torch.zeros(L.da_invcons_ws_bytes(N, D, H, W), dtype=torch.uint8, device=dev())
    for dims in ((0, D, H, W), (N, 1, H, W), (N, D, 1, W), (N, D, H, 1)):
        assert L.da_invcons_fwd(ptr(a), ptr(a), *dims, ptr(loss), None, None, ptr(ws), ws.numel(), stream()) == -1
        assert L.da_invcons_bwd(ptr(a), ptr(a), ptr(a), ptr(loss), ptr(a), None, *dims, 0, None, 0, stream()) == -1
    assert L.da_invcons_fwd(None, ptr(a), N, D, H, W, ptr(loss), None, None, ptr(ws), ws.numel(), stream()) == -1
    assert L.da_invcons_fwd(ptr(a), ptr(a), N, D, H, W, ptr(loss), None, None, ptr(ws), ws.numel() - 1, stream()) == -2
    assert L.da_invcons_bwd(ptr(a), ptr(a), ptr(a), ptr(loss), None, ptr(a), N, D, H, W, 1, ptr(ws), 16, stream()) == -2
    assert L.da_invcons_fwd(ptr(a), ptr(a), N, D, H, W, ptr(loss), None, None, ptr(ws), ws.numel(), stream()) == 0          # stats and resid are optional
    torch.cuda.synchronize()
    assert float(loss) == 0.0


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def test_forward_is_bit_identical_and_deterministic_mode_makes_the_gradients_so():
    from deepatlas_amd import ops
    name, amp = '17x30x22', 2.0
    u_a, u_b = ic.fields(name, amp)
    first, second = _one_way(u_a, u_b), _one_way(u_a, u_b)
    assert first['loss'] == second['loss'] and torch.equal(first['stats'], second['stats']) and torch.equal(first['resid'], second['resid'])
    assert torch.equal(first['d_a'], second['d_a'])                 # the gather has no atomics
    prev = ops.set_deterministic(True)
    try:
        runs = [_one_way(u_a, u_b) for _ in range(2)] + [_one_way(u_a, u_b, 'b')]
        syms = [_symmetric(u_a, u_b) for _ in range(2)]
    finally:
        ops.set_deterministic(prev)
    assert ops.DETERMINISTIC == prev
    for k in ('d_a', 'd_b'):
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(syms[0][k], syms[1][k]), k
    assert torch.equal(runs[0]['d_b'], runs[2]['d_b'])              # (d_a comes from another instantiation of the kernel there: held to the bound below)
    want, want_sym = ic.reference(name, amp)
    ic.check(ic.one_way_distances(runs[0], want), ic.bounds(name, amp, False), 'deterministic')
    ic.check(ic.symmetric_distances(syms[0], want_sym), ic.bounds(name, amp, True), 'deterministic symmetric')


# ---- descent ---------------------------------------------------------------------------------------------------------------------------
def test_descent_makes_two_fields_consistent():
    from deepatlas_amd.lib.loss import InverseConsistencyLoss
    a, b = ic.descent_start()
    losses = ic.descent(InverseConsistencyLoss(), a, b, device=dev())
    print('L_sym %.4g -> %.4g (ratio %.4f; float64 reference %s)' % (losses[0], losses[-1], losses[-1] / losses[0], ic.DESCENT_MEASURED))
    assert abs(losses[0] - ic.DESCENT_MEASURED[0]) < 0.01 * ic.DESCENT_MEASURED[0]
    assert losses[-1] < ic.DESCENT_RATIO * losses[0]


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def test_stats_entry_points_report_the_forward_statistics():
    from deepatlas_amd import ops
    from deepatlas_amd.lib import evalMetrics
    name, amp = '33x47x61', 2.0
    u_a, u_b = ic.fields(name, amp)
    shape, n, _ = ic.CASES[name]
    V = float(shape[0] * shape[1] * shape[2])
    fwd = _one_way(u_a, u_b)['stats']
    a, b = u_a.to(dev()).requires_grad_(True), u_b.to(dev())
    s = ops.inverse_consistency_stats(a, b)
    assert sorted(s) == ['max_vox', 'mean_vox', 'outside_frac', 'rms_vox'] and all(v.dtype == torch.float64 and tuple(v.shape) == (n,) and not v.requires_grad for v in s.values())
    same = lambda got, want: torch.allclose(got.cpu(), want, rtol=1e-14, atol=0)      # (the device divides by multiplying with 1 / V: the last bit)
    assert same(s['mean_vox'], fwd[:, 1] / V) and same(s['rms_vox'], (fwd[:, 0] / V).sqrt())
    assert torch.equal(s['max_vox'].cpu(), fwd[:, 2]) and same(s['outside_frac'], fwd[:, 3] / V)
    m = evalMetrics.inverse_consistency(a, b)
    import numpy as np
    assert sorted(m) == sorted(s) and all(isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape == (n,) for v in m.values())
    for k in s:
        assert np.array_equal(m[k], s[k].cpu().numpy()), k
    want = ic.reference(name, amp)[0]['stats']
    bound = ic.bounds(name, amp, False)
    assert np.allclose(m['mean_vox'], (want[:, 1] / V).numpy(), rtol=bound['mean'], atol=0)
    assert np.allclose(m['rms_vox'], (want[:, 0] / V).sqrt().numpy(), rtol=bound['sum2'], atol=0)          # (the root halves the relative error)
    assert np.allclose(m['max_vox'], want[:, 2].numpy(), rtol=bound['max'], atol=0) and np.allclose(m['outside_frac'], (want[:, 3] / V).numpy(), rtol=1e-14, atol=0)      # the counts are equal; the division's last bit
    assert np.all(m['max_vox'] >= m['rms_vox']) and np.all(m['rms_vox'] >= m['mean_vox']) and np.all(m['mean_vox'] > 0)


# ---- the step --------------------------------------------------------------------------------------------------------------------------
SHAPE = (16, 16, 32)
ENTRIES = ('da_invcons_fwd', 'da_invcons_bwd')


def _reg():
    from oracle import nets
    from deepatlas_amd.lib.network_factory import get_network
    reg = get_network('voxel_morph_cvpr')()
    reg.load_state_dict({k: v.clone() for k, v in nets.closed_form_fill(nets.voxelmorph_param_shapes(), seed=4).items()}, strict=True)
    return reg.to(dev())


def _pair(n=2):
    from oracle import nets
    return nets.closed_form_volume((n, 1) + SHAPE, seed=5).to(dev()), nets.closed_form_volume((n, 1) + SHAPE, seed=6).to(dev())


def _profiled(fn):
    """fn() under a CallProfiler: (result, the C entries it called)."""
    from deepatlas_amd import _native
    prev, _native.profiler = _native.profiler, _native.CallProfiler()
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {key[0] for key in _native.profiler.records}
    finally:
        _native.profiler = prev


def test_zero_weight_is_the_step_without_the_argument():
    """lam_ic = 0: no module, no doubled batch, none of the new entries called, and in deterministic mode the loss, the fields and every
    parameter gradient are bit-identical to a step constructed without the argument."""
    from deepatlas_amd import ops
    from deepatlas_amd.models.joint import RegistrationStep
    from deepatlas_amd.optim import FlatAdam
    prev = ops.set_deterministic(True)
    got = []
    try:
        for kw in ({}, {'lam_ic': 0.0}):
            torch.manual_seed(0)
            reg = _reg()
            im_m, im_t = _pair()
            ro = FlatAdam(reg.parameters(), lr=1e-3)
            step = RegistrationStep(reg, ro, **kw)
            r, called = _profiled(lambda: step.gradients(im_m, im_t))
            assert step.ic is None and 'ic' not in r and r['disp'].shape[0] == 2
            assert not called & set(ENTRIES) and 'da_bending_fwd' in called
            got.append([r['loss'].clone(), r['disp'].clone(), r['warped'].clone(), r['deform'].clone(), ro.flat_g.detach().clone()]
                       + [p.grad.detach().clone() for p in reg.parameters()])
    finally:
        ops.set_deterministic(prev)
    assert len(got[0]) == len(got[1]) > 6
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert bool(got[0][4].any())


class _ComposedIC(torch.nn.Module):
    """L_sym built from existing ops: WarpFn on the 3-channel field + torch elementwise (what the fused kernels replace)."""

    def forward(self, u_ab, u_ba):
        from deepatlas_amd import ops
        s = ic.scales(tuple(u_ab.shape[2:]), torch.float32).to(u_ab.device)

        def one(a, b):
            sr = (a + ops.WarpFn.apply(b, a)[0]) * s
            return (sr * sr).sum(1).mean()
        return 0.5 * (one(u_ab, u_ba) + one(u_ba, u_ab))


def test_step_with_the_penalty():
    """lam_ic > 0 at 16 x 16 x 32, batch 2: one doubled-batch forward, the loss is the sum of its returned parts, `ic` is the float64 reference on
    the step's own two fields, the return shapes are those of the plain step, and in deterministic mode every parameter gradient is within
    relative L2 1e-4 (warp_cases.CEIL['warp']['d_disp'], the suite's ceiling for gradients through the warp) of the same step with the loss
    composed from existing ops.  Measured on one MI355X: worst parameter 4.0e-06; `ic` 3.4e-08 from float64 on the same fields."""
    from deepatlas_amd import ops
    from deepatlas_amd.models.joint import RegistrationStep
    from deepatlas_amd.optim import FlatAdam
    im_m, im_t = _pair()
    n = im_m.shape[0]
    prev = ops.set_deterministic(True)
    grads = []
    try:
        for fused in (True, False):
            reg = _reg()
            opt = FlatAdam(reg.parameters(), lr=1e-3)
            step = RegistrationStep(reg, opt, lam_reg=0.5, lam_ic=0.7)
            if not fused:
                step.ic = _ComposedIC()
            r, called = _profiled(lambda: step.gradients(im_m, im_t))
            assert (set(ENTRIES) <= called) == fused
            grads.append([p.grad.detach().double().cpu() for p in reg.parameters()])
            if not fused:
                assert abs(float(r['ic']) - ic_fused) <= 1e-5 * ic_fused
                continue
            ic_fused = float(r['ic'])
            assert r['disp'].shape == (2 * n, 3) + SHAPE and r['warped'].shape == (2 * n, 1) + SHAPE and r['deform'].shape == (2 * n, 3) + SHAPE
            assert float(r['loss']) == float((r['sim'] + 0.5 * r['bend']) + 0.7 * r['ic'])
            d = r['disp'].cpu()
            ab = ic.evaluate(d[:n], d[n:], torch.float64)
            want = ic.symmetric_of(ab, ic.evaluate(d[n:], d[:n], torch.float64))['loss']
            bound = max(ic.bounds(nm, amp, True)['loss'] for nm, amp in ic.COMBOS)
            print('ic %.9e (float64 on the same fields %.9e, rel %.2e, bound %.1e)' % (ic_fused, want, abs(ic_fused - want) / want, bound))
            assert want > 0.0 and abs(ic_fused - want) <= bound * want
            before = opt.flat_p.detach().clone()
            out = step(im_m, im_t)                                   # the return tuple keeps its shape: the caller's direction
            torch.cuda.synchronize()
            assert len(out) == 3 and len(out[1]) == 3 and len(out[2]) == 2
            assert out[1][0].shape == (n, 3) + SHAPE and out[1][1].shape == (n, 1) + SHAPE and out[1][2].shape == (n, 3) + SHAPE
            assert step.last_disp_reverse.shape == (n, 3) + SHAPE and torch.equal(step.last_ic, r['ic'])
            assert torch.equal(out[1][0], r['disp'][:n]) and torch.equal(step.last_disp_reverse, r['disp'][n:])
            assert bool(torch.isfinite(opt.flat_p).all()) and not torch.equal(before, opt.flat_p)
    finally:
        ops.set_deterministic(prev)
    worst = max(float((a - b).norm() / b.norm()) for a, b in zip(*grads))
    print('parameter gradients, fused against composed: worst relative L2 %.2e' % worst)
    assert worst <= wc.CEIL['warp']['d_disp']


def test_step_with_the_penalty_replays_as_a_hip_graph():
    """The kernels use the workspace only (no allocation inside the entries, no synchronisation): the step captured by graphs.GraphedStep
    trains like the eager one, bit for bit (deterministic mode for the scatter)."""
    from deepatlas_amd import ops
    from deepatlas_amd.graphs import GraphedStep
    from deepatlas_amd.models.joint import RegistrationStep
    from deepatlas_amd.optim import FlatAdam
    prev = ops.set_deterministic(True)
    results = []
    try:
        for graph in (False, True):
            reg = _reg()
            im_m, im_t = _pair()
            ro = FlatAdam(reg.parameters(), lr=1e-3)
            segments, between, opts = RegistrationStep(reg, ro, lam_ic=0.7).segments(im_m, im_t)
            g = GraphedStep(segments, opts, between=between, warmup=1 if graph else 10 ** 9)
            vals = []
            for _ in range(4):                                          # graphed: 1 eager, capture + replay, 2 replays
                r = g()
                vals.append((float(r['loss'].item()), float(r['ic'].item())))      # (read at once: a replay writes the same tensors again)
            assert (g.graphs is not None) == graph
            torch.cuda.synchronize()
            results.append((vals, ro.flat_p.detach().cpu()))
            g.close()
    finally:
        ops.set_deterministic(prev)
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert all(math.isfinite(v) and v > 0.0 for _, v in results[0][0]) and len(set(results[0][0])) == 4
    assert torch.equal(results[0][1], results[1][1])


# ---- the experiment --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['lambda_ic', 'report_ic', 'neither'])
def test_experiment_reports_inverse_consistency_exactly_when_asked(mode, tmp_path, monkeypatch, capsys):
    """--lambda-ic / --report-ic through build_config into one epoch of the experiment: the validation result carries the three ic_* keys with
    finite values, the lines their parts; a run without either carries none of them."""
    import argparse
    from torch.utils.data import DataLoader
    import train_reg
    from deepatlas_amd.lib.datasets import SyntheticRegDataset
    from deepatlas_amd.models.registration import RegistrationExperiment
    monkeypatch.chdir(tmp_path)
    extra = {'lambda_ic': dict(lambda_ic=1.0, report_ic=False), 'report_ic': dict(lambda_ic=0.0, report_ic=True), 'neither': {}}[mode]
    ns = argparse.Namespace(device='0', debug=False, num_samples=3, num_epochs=1, lr=1e-3, test_only=False, data_root='./data', log_root='logs',
                            shape=list(SHAPE), **extra)
    cfg = train_reg.build_config(ns)
    cfg['training_data_loader'] = DataLoader(SyntheticRegDataset(3, SHAPE, 32, seed=230), batch_size=1, shuffle=False)
    cfg['validation_data_loader'] = DataLoader(SyntheticRegDataset(2, SHAPE, 32, seed=1230), batch_size=1, shuffle=False)
    cfg.update(lr_mode='const', samples_per_epoch=2, print_batch_period=1)
    exp = RegistrationExperiment(cfg)
    assert exp.exp_name.endswith('_ic1.0') == (mode == 'lambda_ic')
    assert (exp.lambda_ic, exp.report_ic) == {'lambda_ic': (1.0, True), 'report_ic': (0.0, True), 'neither': (0.0, False)}[mode]
    exp.train()
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith('Epoch[')]
    valid = [l for l in out.splitlines() if l.startswith('Validation:')]
    assert len(lines) == 2 and len(valid) == 1, out
    assert all((' ic: ' in l) == (mode == 'lambda_ic') for l in lines), out
    assert (exp.step.ic is not None) == (mode == 'lambda_ic')
    res = exp.last_validation
    keys = ('ic_mean_vox', 'ic_max_vox', 'ic_outside_frac')
    if mode == 'neither':
        assert not [k for k in res if k.startswith('ic_')] and 'inverse consistency' not in out and '_ic' not in exp.exp_name
    else:
        assert all(k in res and math.isfinite(res[k]) for k in keys), res
        assert 0.0 <= res['ic_mean_vox'] <= res['ic_max_vox'] and 0.0 <= res['ic_outside_frac'] <= 1.0
        assert 'inverse consistency' in valid[0] and ' vox mean' in valid[0]
    if mode == 'lambda_ic':
        assert all(float(l.split(' ic: ')[1].split()[0]) >= 0.0 for l in lines)
