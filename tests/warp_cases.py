"""Shared by tests/test_gpu_warp_shapes.py (the warp.hip kernels against float64) and tests/test_warp_reference.py (the fp32 CPU oracle against float64,
no GPU): hypothesis strategies and explicit per-branch examples for ops.WarpFn / WarpLabelsFn / LabelWarpDiceFn / SegPhaseLossFn, builders that turn a
case into well-conditioned fp32 CPU inputs, the float64 references and the tolerances.  Layout, `run_cases`, the worst-case record and the
DA_LOSS_SHAPES_REPORT file are those of tests/loss_cases.py (one record for both modules: keys 'warp/...', 'warplabels/...', 'lwd/...', 'segphase/...',
'adjoint/...').

The reference is torch-CPU float64 throughout: the identity grid k / (size - 1) * 2 - 1 formed in float64 (oracle.nets.identity_transform rounds it to fp32
first: that one is the fp32 oracle's), F.grid_sample(bilinear, zeros, align_corners=True) through oracle.nets.warp_trilinear, one-hot maps built with C + 1
channels and the last one dropped (a label outside [0, C) counts for no class), F.softmax, oracle.losses.dice_loss, every gradient by autograd.  Voxels
whose coordinate is non-finite or >= 1e9 in magnitude get the normalised coordinate -4 on all three axes before the reference runs (warp.hip
is_finite_coord: every tap out of range, no gradient).

Conditioning.  The gradient of a trilinear sample with respect to its coordinate is one-sided at lattice points: at zero displacement torch's own fp32 and
fp64 d_disp differ by a rel-l2 of 0.8, because an fp32 coordinate falls into either neighbouring cell.  So a DRAWN field (amplitude 0.05 / 0.3 / 2 / 8
voxels, scaled by 2 / (size - 1) per axis) has every component whose float64 voxel coordinate lies within DELTA = 1e-4 of an integer moved by 4 DELTA
(`off_lattice`; the fp32 coordinate arithmetic is good to a few 1e-6 voxels, so both precisions then sit in the same cell) and is compared everywhere
against ONE reference.  The PINNED lattice fields ('zero', 'shift': where training starts) compare everything but d_disp in the ordinary way; d_disp is
held, element by element, to the float64 value at the field moved by -1e-6 or +1e-6 voxel along that component's axis (`lattice_sides`, `close_either`).

Plain module, no fixtures, no pytest settings."""
import numpy as np
import torch
from hypothesis import strategies as st

import loss_cases as lc
from loss_cases import run_cases, note, close, rnd, _cyc, _f64, _leaf      # noqa: F401  (run_cases / note / close are used by the two test files)
from oracle import losses, nets

DELTA = 1e-4               # no drawn coordinate is closer than this to an integer (voxels)
LATTICE_STEP = 1e-6        # the two sides of a lattice point at which a pinned lattice case takes its d_disp reference (voxels)
AMPS = [0.05, 0.3, 2.0, 8.0]
HUGE = 1e9                 # warp.hip is_finite_coord
# What fp32 coordinates cost a sampled value, per voxel of axis length S - 1: the voxel coordinate ((k / (S - 1) * 2 - 1 + disp) + 1) / 2 * (S - 1) takes five
# roundings of at most 2^-24 on values of magnitude <= 2 in normalised units, 3e-7 (S - 1) / 2 voxels, and an i.i.d. source in [-1, 1] changes by up to 2 per
# voxel: 3e-7 (S - 1) of max|src|.  That is torch's own fp32 grid_sample against float64 as much as the kernels' (measured on the examples here: 1.1e-5 at
# S = 60, 5.9e-6 at S = 47), so on the long volumes the fp32 oracle cannot sit within a quarter of a 2e-5 tolerance: for `warped` and `d_src` the CPU companion
# asserts max(tolerance / 4, COORD_ERR (S - 1)), capped at the tolerance, instead of the plain quarter (equal to it up to S = 17).
COORD_ERR = 3e-7

# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# CEIL: what the suite asserted for the same quantity before these files (tests/test_gpu_ops.py, test_gpu_random_shapes.py, test_gpu_nets.py): forward warp
# and d_src 2e-5 (1e-5 on the fixed cases), d_disp 1e-4, deform 1e-6; the label warp's d_disp 1e-5 and its forward at the forward warp's 1e-5; the
# label-warp Dice 2e-6 of max(1, |loss|) and, on d_disp, 1e-5 against the op-by-op kernels / 1e-4 at full size (the latter is the ceiling here); the segmentation phase 1e-5 of max(1, |loss|) and 1e-4 on the logit gradient; the adjoint
# scatter 2e-5 absolute.  TOL follows loss_cases.TOL's rule: where the worst case measured on an MI355X (table in test_gpu_warp_shapes.py) is more than
# 10 x below the ceiling, max(4 x device worst, 8 x fp32-CPU-oracle worst) rounded up to two digits; otherwise the ceiling stays.
CEIL = {
    'warp': {'warped': 2e-5, 'deform': 1e-6, 'd_src': 2e-5, 'd_disp': 1e-4},
    'warplabels': {'fwd': 1e-5, 'd_disp': 1e-5},
    'lwd': {'loss': 2e-6, 'd_disp': 1e-4},
    'segphase': {'loss': 1e-5, 'dlogits': 1e-4},
    'adjoint': {'A': 2e-5, 'B': 2e-5},
}
TOL = {
    'warp': {'warped': 2e-5, 'deform': 6.8e-7, 'd_src': 2e-5, 'd_disp': 9.8e-6},      # warped 1.1e-5, d_src 8.0e-6 measured, less than 10 x below: stay
    'warplabels': {'fwd': 1e-5, 'd_disp': 1e-5},                                      # 2.9e-6 and 1.1e-6 (9.3 x below) measured: stay
    'lwd': {'loss': 2e-6, 'd_disp': 3.5e-5},                                          # loss 4.2e-7 measured: stays
    'segphase': {'loss': 3.5e-7, 'dlogits': 4.1e-5},
    'adjoint': {'A': 2e-5, 'B': 2e-5},                                                # 5.8e-6 / 6.2e-6 measured: stay
}
assert all(TOL[f][k] <= CEIL[f][k] for f in CEIL for k in CEIL[f])


def close_either(family, what, got, left, right, tol):
    """A lattice case's d_disp: every element within `tol` (in units of max|ref|) of the reference on one side of the lattice point or the other."""
    got, left, right = (t.detach().cpu().double().numpy() for t in (got, left, right))
    assert got.shape == left.shape == right.shape, (got.shape, left.shape)
    assert np.isfinite(got).all(), 'non-finite values'
    scale = max(float(np.abs(left).max()), float(np.abs(right).max()), 1e-30)
    e = float(np.minimum(np.abs(got - left), np.abs(got - right)).max() / scale)
    note(family, what + ' (lattice, either side)', e)
    assert e < tol, '%s %s at a lattice point: %.3e (tolerance %.1e)' % (family, what, e, tol)
    return e


# ---- fields ----------------------------------------------------------------------------------------------------------------------
def identity(vol, dtype):
    """3 x D x H x W, channel 0 = W axis: the fp32 oracle's own grid for float32, the same formula evaluated in float64 for float64."""
    if dtype == torch.float32:
        return nets.identity_transform(vol)
    D, H, W = vol
    ax = lambda n: torch.arange(n, dtype=torch.float64) / (n - 1) * 2.0 - 1
    return torch.stack([ax(W).view(1, 1, W).expand(D, H, W), ax(H).view(1, H, 1).expand(D, H, W), ax(D).view(D, 1, 1).expand(D, H, W)])


def _per_axis(vol, fn):
    D, H, W = vol
    return torch.tensor([fn(W), fn(H), fn(D)], dtype=torch.float64).view(1, 3, 1, 1, 1)


def axis_scale(vol):
    """one voxel in normalised units, per displacement channel (x, y, z) = (W, H, D)"""
    return _per_axis(vol, lambda s: 2.0 / (s - 1))


def voxel_coords(disp, vol):
    """float64 voxel coordinates (grid_sampler_unnormalize, align_corners=True) of an N x 3 x D x H x W field"""
    return (disp.double() + identity(vol, torch.float64) + 1) / 2 * _per_axis(vol, lambda s: float(s - 1))


def bad_voxels(disp, vol):
    """N x 1 x D x H x W: voxels with a non-finite coordinate or one of magnitude >= 1e9 on any axis"""
    g = disp.double() + identity(vol, torch.float64)
    return (~torch.isfinite(g) | (g.abs() >= HUGE)).any(1, keepdim=True)


def lattice_distance(disp, vol):
    """the smallest distance of any coordinate component to an integer, in voxels, over the voxels whose coordinates are all finite"""
    c = voxel_coords(disp, vol)
    c = c[~bad_voxels(disp, vol).expand_as(c)]            # (a bad voxel samples at -4 whatever its other components say)
    return float((c - c.round()).abs().min()) if c.numel() else 1.0


def off_lattice(disp, vol):
    """every component whose float64 voxel coordinate is within DELTA of an integer moved by 4 DELTA (the field stays fp32)"""
    step = (4 * DELTA) * axis_scale(vol)
    for _ in range(4):
        c = voxel_coords(disp, vol)
        near = torch.isfinite(c) & ((c - c.round()).abs() < DELTA)
        if not bool(near.any()):
            break
        disp = torch.where(near, (disp.double() + step).float(), disp)
    return disp


NONFINITE = [(float('nan'), 0.01, 0.0), (0.0, float('inf'), 0.0), (0.0, 0.0, 1e30), (float('-inf'), float('nan'), -1e30)]


def build_field(case):
    """N x 3 x D x H x W fp32.  'rand': uniform in +- amp voxels, off the lattice.  'zero' / 'shift': the lattice fields (shift: whole voxels (x, y, z)).
    'nonfinite': a 'rand' field with a NaN, an inf, a 1e30 and a mixed displacement at four voxels (first, last and two inside)."""
    n, vol = case['n'], tuple(case['vol'])
    kind = case.get('field', 'rand')
    shape = (n, 3) + vol
    if kind == 'zero':
        return torch.zeros(shape)
    if kind == 'shift':
        k = torch.tensor(case['shift'], dtype=torch.float64).view(1, 3, 1, 1, 1)
        return (k * axis_scale(vol)).float().expand(shape).contiguous()
    u = off_lattice((rnd(shape, case['sd'] + 1).double() * case['amp'] * axis_scale(vol)).float(), vol)
    if kind == 'nonfinite':
        V = vol[0] * vol[1] * vol[2]
        flat = u.reshape(n, 3, V)
        for i, (v, val) in enumerate(zip((0, V // 3, V // 2, V - 1), NONFINITE)):
            flat[i % n, :, v] = torch.tensor(val)
        u = flat.reshape(shape)
    return u


def is_lattice(case):
    return case.get('field', 'rand') in ('zero', 'shift')


def _grid(inp, dtype, disp, want_grad):
    """(disp leaf, deform, sampling grid) of the reference: the bad voxels' displacement is a constant 0 and their grid coordinate -4"""
    bad = inp['bad']
    u0 = (inp['disp'] if disp is None else disp).to(dtype)
    u = torch.where(bad, torch.zeros_like(u0), u0).detach().requires_grad_(bool(want_grad))
    deform = u + identity(inp['vol'], dtype)
    return u, deform, torch.where(bad, torch.full_like(deform, -4.0), deform)


def lattice_sides(ref_d_disp, inp):
    """(left, right): component a of each is the float64 d_disp component a at the field moved by -+ LATTICE_STEP voxel along axis a"""
    sides = []
    for sign in (-1.0, 1.0):
        comps = []
        for a in range(3):
            delta = torch.zeros((1, 3, 1, 1, 1), dtype=torch.float64)
            delta[0, a] = sign * LATTICE_STEP
            comps.append(ref_d_disp(inp, torch.float64, inp['disp'].double() + delta * axis_scale(inp['vol']))[:, a])
        sides.append(torch.stack(comps, 1))
    return sides


_REFS = {}


def cached(ref, case, inp):
    """the float64 reference of one case, computed once per process and shared by the tests that need it (callers do not modify it)"""
    key = (ref.__name__, repr(case))
    if key not in _REFS:
        _REFS[key] = ref(inp, torch.float64)
    return _REFS[key]


_vol = st.one_of(st.tuples(st.integers(2, 6), st.integers(2, 9), st.integers(2, 70)),
                 st.sampled_from([(2, 2, 2), (2, 3, 43), (3, 5, 17), (4, 8, 8), (5, 7, 59), (4, 9, 25), (7, 9, 60)]))
_small_vol = st.one_of(st.tuples(st.integers(2, 5), st.integers(2, 7), st.integers(2, 37)), st.sampled_from([(2, 2, 2), (3, 5, 17), (4, 8, 8), (4, 9, 25)]))


# ---- WarpFn ----------------------------------------------------------------------------------------------------------------------
# warp.hip da_warp_fwd: C / 4 in {2, 4, 8} and N <= 65535 -> warp_fwd_grouped_kernel, cdiv(V, 512) blocks per sample, the block -> range map through
#     da_xcd_item_of_block when that count is a multiple of 8;  other C with C / 4 a power of two <= 64 (4, 64, 128, 256; 8 ... 32 at N > 65535) ->
#     warp_fwd_kernel<4>, lpv = C / 4;  everything else (1, 3, 12, 260) -> warp_fwd_kernel<1>.
# da_warp_bwd: d_src for C in {8, 16, 32, 64} -> warp_bwd_dsrc_lane_kernel (then d_disp alone through warp_bwd_kernel); C = 4, 128, 256 ->
#     warp_bwd_kernel<4> forms d_src by atomics itself; C = 1, 3, 12, 260 -> warp_bwd_kernel<1>.  grads = 'src' / 'disp': the d_disp == nullptr /
#     d_src == nullptr routes.  The generic kernels' da_xcd_loop splits the range per XCD when cdiv(N V lpv, 256) is a multiple of 8.
WARP_C = [1, 3, 4, 8, 12, 16, 32, 64, 128, 256, 260]
WARP = st.fixed_dictionaries(dict(
    C=st.sampled_from(WARP_C), n=st.integers(1, 3), vol=_vol, amp=st.sampled_from(AMPS), grads=st.sampled_from(['both', 'both', 'src', 'disp']),
    gdef=st.booleans(), sd=st.integers(0, 999)))


def _w(C, n, vol, amp=0.3, grads='both', gdef=True, sd=0, **kw):
    return dict(C=C, n=n, vol=vol, amp=amp, grads=grads, gdef=gdef, sd=sd, **kw)


WARP_PINNED = (
    # one per channel count = per forward / backward kernel and lpv, the other options cycling
    [_w(C, 1 + i % 3, _cyc([(5, 7, 11), (3, 5, 17), (2, 9, 29)], i), _cyc(AMPS, i), 'both', i % 2 == 0, i) for i, C in enumerate(WARP_C)]
    # gradient to one input only, for every backward route
    + [_w(C, 1 + i % 2, (3, 5, 17), _cyc(AMPS, i), g, g == 'disp', 20 + i) for i, (C, g) in enumerate((C, g) for C in (3, 4, 16, 64, 128, 260) for g in ('src', 'disp'))]
    # grouped kernel: V = 3780 -> 8 blocks per sample (the XCD remap), V = 2065 -> 5 blocks (no remap; V no multiple of 64 / 256 / 512), V = 8 -> one partial wave
    + [_w(8, 2, (7, 9, 60), 2.0, sd=40), _w(16, 1, (7, 9, 60), 0.3, sd=41), _w(32, 1, (7, 9, 60), 8.0, sd=42),
       _w(8, 1, (5, 7, 59), 0.3, sd=43), _w(32, 3, (5, 7, 59), 2.0, sd=44), _w(16, 2, (2, 2, 2), 0.05, sd=45)]
    # N = 65536 > 65535 (grid.y): C = 8 leaves the grouped kernel for warp_fwd_kernel<4> with lpv = 2; 16 MB of source
    + [_w(8, 65536, (2, 2, 2), 0.3, sd=46)]
    # generic kernels with cdiv(N V lpv, 256) = 8: da_xcd_loop's per-XCD ranges (lpv = 16, 1, and the scalar kernel)
    + [_w(64, 1, (2, 7, 9), 0.3, sd=47), _w(4, 1, (7, 9, 31), 2.0, sd=48), _w(3, 1, (7, 9, 31), 0.3, sd=49)]
    # lattice fields: zero displacement and a whole-voxel shift
    + [_w(1, 2, (3, 5, 17), field='zero', sd=50), _w(32, 1, (5, 7, 11), field='zero', sd=51), _w(128, 1, (3, 5, 17), field='zero', sd=52),
       _w(8, 2, (5, 7, 11), field='shift', shift=(1, -1, 2), sd=53), _w(12, 1, (3, 5, 17), field='shift', shift=(-2, 1, 0), sd=54),
       _w(64, 1, (5, 7, 11), field='shift', shift=(3, 0, -1), sd=55)]
    # non-finite and huge displacements at four voxels: grouped, <4> with lpv 1 / 16, scalar
    + [_w(C, 1 + i % 2, (3, 5, 17), 0.3, 'both', False, 60 + i, field='nonfinite') for i, C in enumerate((16, 4, 64, 3))]
)


def build_warp(case):
    C, n, vol = case['C'], case['n'], tuple(case['vol'])
    disp = build_field(case)
    return dict(src=rnd((n, C) + vol, case['sd']), disp=disp, go=rnd((n, C) + vol, case['sd'] + 2), gd=rnd((n, 3) + vol, case['sd'] + 3) if case['gdef'] else None,
                vol=vol, grads=case['grads'], bad=bad_voxels(disp, vol))


def ref_warp(inp, dtype, disp=None):
    src = _leaf(inp['src'], dtype, inp['grads'] in ('both', 'src'))
    u, deform, grid = _grid(inp, dtype, disp, inp['grads'] in ('both', 'disp'))
    warped = nets.warp_trilinear(src, grid)
    tot = (warped * inp['go'].to(dtype)).sum()
    if inp['gd'] is not None:
        tot = tot + (deform * inp['gd'].to(dtype)).sum()
    tot.backward()
    return dict(warped=_f64(warped), deform=_f64(deform), d_src=None if src.grad is None else _f64(src.grad), d_disp=None if u.grad is None else _f64(u.grad))


def ref_warp_d_disp(inp, dtype, disp):
    return ref_warp(dict(inp, grads='disp'), dtype, disp)['d_disp']


# ---- label maps ------------------------------------------------------------------------------------------------------------------
def wild_labels(kind, shape, C, sd, wide, wild=True):
    """(n, d, h, w) labels: 'iid' / 'blocky' (loss_cases.labels_for) or 'const' (one class everywhere: one histogram key per wave); wild: one voxel in twelve
    carries a label outside [0, C) -- C or C + 5, and for int64 also -1 and -2.  A 'const' map stays constant."""
    if kind == 'const':
        lab = torch.full(shape, int(sd) % C, dtype=torch.long)
    else:
        lab = lc.labels_for(kind, shape, C, sd, True)
        if wild:
            g = torch.Generator().manual_seed(int(sd) + 13)
            outs = torch.tensor([-2, -1, C, C + 5] if wide else [C, C + 5])
            hit = torch.rand(shape, generator=g) < 1.0 / 12
            lab = torch.where(hit, outs[torch.randint(0, len(outs), shape, generator=g)], lab)
    return lab if wide else lab.to(torch.uint8)


def one_hot(lab, C, dtype):
    """N x C x D x H x W: C + 1 channels, every label outside [0, C) sent to the last one, which is dropped"""
    l = lab.long()
    idx = torch.where((l >= 0) & (l < C), l, torch.full_like(l, C)).unsqueeze(1)
    return torch.zeros((l.shape[0], C + 1) + tuple(l.shape[1:]), dtype=dtype).scatter_(1, idx, 1.0)[:, :C].contiguous()


# ---- WarpLabelsFn ----------------------------------------------------------------------------------------------------------------
# da_warp_labels_fwd: C % 4 == 0 -> warp_labels_fwd_kernel<4> (a lane per channel quad), else <1> (a lane per channel); da_warp_labels_bwd: one kernel
WARPLABELS_C = [1, 2, 3, 4, 5, 8, 12, 31, 32, 64]
WARPLABELS = st.fixed_dictionaries(dict(
    C=st.sampled_from(WARPLABELS_C), n=st.integers(1, 3), vol=_small_vol, amp=st.sampled_from(AMPS), wide=st.booleans(), kind=st.sampled_from(['iid', 'blocky']),
    sd=st.integers(0, 999)))
WARPLABELS_PINNED = (
    [dict(C=C, n=1 + i % 3, vol=_cyc([(5, 7, 11), (3, 5, 17), (2, 9, 29)], i), amp=_cyc(AMPS, i), wide=i % 2 == 0, kind=_cyc(['iid', 'blocky'], i // 2), sd=i)
     for i, C in enumerate(WARPLABELS_C)]
    + [dict(C=8, n=1, vol=(7, 9, 31), amp=0.3, wide=False, kind='iid', sd=20),          # cdiv(V, 256) = 8 blocks: the backward's per-XCD ranges
       dict(C=5, n=2, vol=(3, 5, 17), amp=0.3, wide=True, kind='iid', sd=21, field='zero'),
       dict(C=4, n=1, vol=(5, 7, 11), amp=0.3, wide=False, kind='blocky', sd=22, field='shift', shift=(1, 1, -1)),
       dict(C=12, n=2, vol=(3, 5, 17), amp=0.3, wide=True, kind='iid', sd=23, field='nonfinite'),
       dict(C=3, n=1, vol=(3, 5, 17), amp=0.3, wide=False, kind='iid', sd=24, field='nonfinite')]
)


def build_warplabels(case):
    C, n, vol = case['C'], case['n'], tuple(case['vol'])
    disp = build_field(case)
    return dict(labels=wild_labels(case['kind'], (n,) + vol, C, case['sd'], case['wide']), C=C, disp=disp, go=rnd((n, C) + vol, case['sd'] + 2), vol=vol,
                bad=bad_voxels(disp, vol))


def ref_warplabels(inp, dtype, disp=None):
    u, _, grid = _grid(inp, dtype, disp, True)
    warped = nets.warp_trilinear(one_hot(inp['labels'], inp['C'], dtype), grid)
    (warped * inp['go'].to(dtype)).sum().backward()
    return dict(fwd=_f64(warped), d_disp=_f64(u.grad))


def ref_warplabels_d_disp(inp, dtype, disp):
    return ref_warplabels(inp, dtype, disp)['d_disp']


# ---- LabelWarpDiceFn -------------------------------------------------------------------------------------------------------------
# da_label_warp_dice_fwd: any C <= 64 and N <= 64 (C = 65: DA_ERR_UNSUPPORTED, N = 65: DA_ERR_BADARG); label_warp_dice_partial_kernel on a grid of
# (cdiv(V, 512), N): sample n = blockIdx.y, wave-level histograms over the distinct labels a wave sees, V % 64 != 0 handled by `live` lanes, the per-XCD
# ranges of da_xcd_loop when cdiv(V, 512) is a multiple of 8; da_label_warp_dice_bwd: one kernel over N V voxels.
WEIGHTS = ['Uniform', 'Simple', 'Volume']
LWD = st.fixed_dictionaries(dict(
    C=st.integers(1, 64), n=st.integers(1, 3), vol=_small_vol, amp=st.sampled_from(AMPS), wt=st.sampled_from(WEIGHTS), no_bg=st.booleans(), wm=st.booleans(),
    wtg=st.booleans(), km=st.sampled_from(['iid', 'blocky', 'const']), kt=st.sampled_from(['iid', 'blocky', 'const']), gl=st.sampled_from([0.37, -1.9, 2.5]),
    sd=st.integers(0, 999)))


def _l(C, n, vol, i, **kw):
    d = dict(C=C, n=n, vol=vol, amp=_cyc(AMPS, i), wt=_cyc(WEIGHTS, i), no_bg=i % 2 == 1, wm=i % 4 < 2, wtg=i % 3 == 0, km=_cyc(['iid', 'blocky', 'iid', 'const'], i),
             kt=_cyc(['blocky', 'iid', 'iid'], i), gl=_cyc([0.37, -1.9, 2.5], i), sd=i)
    d.update(kw)
    return d


LWD_PINNED = (
    [_l(C, 1 + C % 3, _cyc([(3, 5, 7), (2, 3, 43), (3, 5, 17)], C), C) for C in range(1, 65)]                       # every class count (V = 105, 258, 255)
    + [_l(5, 64, (2, 2, 3), 70, km='iid', kt='iid'),                                                              # N = 64 on a tiny volume: blockIdx.y up to 63
       _l(7, 3, (3, 5, 17), 71, km='const', kt='const', wm=False, wtg=False),                                     # one key per wave in both maps
       _l(64, 2, (5, 7, 11), 72, km='iid', kt='iid', amp=0.3),                                                    # C = 64, per-voxel random labels: a wave full of keys
       _l(32, 2, (7, 9, 60), 73, km='blocky', kt='blocky', amp=2.0),                                              # cdiv(V, 512) = 8: per-XCD ranges
       _l(6, 2, (3, 5, 17), 74, field='zero'), _l(32, 1, (5, 7, 11), 75, field='shift', shift=(1, 0, -1)),
       _l(9, 2, (3, 5, 17), 76, field='nonfinite', amp=0.3)]
)


def build_lwd(case):
    C, n, vol = case['C'], case['n'], tuple(case['vol'])
    disp = build_field(case)
    return dict(lab_m=wild_labels(case['km'], (n,) + vol, C, case['sd'], case['wm']), lab_t=wild_labels(case['kt'], (n,) + vol, C, case['sd'] + 5, case['wtg']),
                C=C, disp=disp, vol=vol, wt=case['wt'], no_bg=case['no_bg'] and C > 1, gl=case['gl'], bad=bad_voxels(disp, vol))


def ref_lwd(inp, dtype, disp=None):
    u, _, grid = _grid(inp, dtype, disp, True)
    warped = nets.warp_trilinear(one_hot(inp['lab_m'], inp['C'], dtype), grid)
    l = losses.dice_loss(warped, one_hot(inp['lab_t'], inp['C'], dtype), inp['C'], inp['wt'], inp['no_bg'], False, eps=1e-6)
    (l * inp['gl']).backward()
    return dict(loss=float(l.detach().double()), d_disp=_f64(u.grad))


def ref_lwd_d_disp(inp, dtype, disp):
    return ref_lwd(inp, dtype, disp)['d_disp']


# ---- SegPhaseLossFn --------------------------------------------------------------------------------------------------------------
# ops.SegPhaseLossFn at the class counts ops.fused_anatomy_supported lets through.  da_warp_dice_fwd: C = 8, 16, 32 -> warp_dice_grouped_kernel,
# C = 4, 64 -> warp_dice_partial_kernel (lpv 1 / 16), cdiv(V, 1024 / lpv) blocks per sample, remapped through da_xcd_item_of_block when a multiple of 8.
# da_seg_anat_dlogits: C = 32 -> seg_anat_dlogits_lane_kernel<32>; C = 4, 8, 16 -> seg_anat_dlogits_kernel with tv = 256; C = 64 -> tv = 128; N cdiv(V, tv)
# tiles, taken per XCD when a multiple of 8.  da_warp_adjoint_labels: the LDS-box kernel, target labels outside [0, C) into A_extra.
SEG_C = [4, 8, 16, 32, 64]
SEG = st.fixed_dictionaries(dict(
    C=st.sampled_from(SEG_C), n=st.integers(1, 2), vol=_vol, amp=st.sampled_from(AMPS), wt=st.sampled_from(WEIGHTS), no_bg=st.booleans(), labelled=st.booleans(),
    wm=st.booleans(), wtg=st.booleans(), kt=st.sampled_from(['iid', 'blocky']), ups=st.sampled_from(['both', 'both', 'anat']), sd=st.integers(0, 999)))


def _s(C, n, vol, i, **kw):
    d = dict(C=C, n=n, vol=vol, amp=_cyc(AMPS, i), wt=_cyc(WEIGHTS, i), no_bg=i % 2 == 1, labelled=i % 3 != 2, wm=i % 2 == 0, wtg=i % 4 < 2, kt=_cyc(['iid', 'blocky'], i),
             ups=_cyc(['both', 'anat'], i // 2), sd=i)
    d.update(kw)
    return d


SEG_PINNED = (
    [_s(C, 1 + (i + j) % 2, _cyc([(5, 7, 11), (3, 5, 17), (2, 9, 29)], i + j), 2 * i + j, labelled=j == 0) for i, C in enumerate(SEG_C) for j in (0, 1)]
    # V = 900, N cdiv(V, tv) = 8 tiles: N = 2 at tv = 256 (C = 4, 8, 16; C = 32: 8 workgroups of the lane kernel), N = 1 at tv = 128 (C = 64) -> per-XCD tiles
    + [_s(4, 2, (4, 9, 25), 20), _s(8, 2, (4, 9, 25), 29), _s(16, 2, (4, 9, 25), 21), _s(32, 2, (4, 9, 25), 22), _s(64, 1, (4, 9, 25), 23)]
    # Dice partial grids that are multiples of 8 (remapped): C = 8 / 32 grouped at V = 3780 / 4095 (8 / 32 blocks), C = 64 at V = 495 (8 blocks), C = 4 at
    # V = 7560 (8 blocks); and not: C = 16 at V = 3780 (15 blocks)
    + [_s(8, 1, (7, 9, 60), 24), _s(32, 1, (7, 9, 65), 25), _s(64, 2, (5, 9, 11), 26), _s(4, 1, (6, 18, 70), 27), _s(16, 1, (7, 9, 60), 28)]
    + [_s(8, 2, (3, 5, 17), 30, field='zero'), _s(64, 1, (3, 5, 17), 31, field='zero', labelled=True), _s(16, 1, (5, 7, 11), 32, field='shift', shift=(1, -1, 0)),
       _s(32, 2, (3, 5, 17), 33, field='nonfinite', amp=0.3), _s(4, 1, (3, 5, 17), 34, field='nonfinite', amp=0.3), _s(64, 2, (3, 5, 17), 35, field='nonfinite', amp=0.3)]
)


def build_seg(case):
    C, n, vol = case['C'], case['n'], tuple(case['vol'])
    disp = build_field(case)
    gs, ga = (0.6, -1.7) if case['ups'] == 'both' else (None, 1.3)
    return dict(logits=rnd((n, C) + vol, case['sd'], 3.0), lab_m=lc.labels_for('iid', (n,) + vol, C, case['sd'] + 3, case['wm']) if case['labelled'] else None,
                lab_t=wild_labels(case['kt'], (n,) + vol, C, case['sd'] + 5, case['wtg']), C=C, disp=disp, vol=vol, wt=case['wt'], no_bg=case['no_bg'], gs=gs, ga=ga,
                bad=bad_voxels(disp, vol))


def ref_seg(inp, dtype, disp=None):
    x = _leaf(inp['logits'], dtype)
    _, _, grid = _grid(inp, dtype, disp, False)
    warped = nets.warp_trilinear(torch.softmax(x, 1), grid)
    l_anat = losses.dice_loss(warped, one_hot(inp['lab_t'], inp['C'], dtype), inp['C'], inp['wt'], inp['no_bg'], False, eps=1e-6)
    l_sup = losses.dice_loss(x, inp['lab_m'].long(), inp['C'], inp['wt'], inp['no_bg'], True, eps=1e-6) if inp['lab_m'] is not None else None
    tot = l_anat * inp['ga']
    if l_sup is not None and inp['gs'] is not None:
        tot = tot + l_sup * inp['gs']
    tot.backward()
    return dict(l_sup=0.0 if l_sup is None else float(l_sup.detach().double()), l_anat=float(l_anat.detach().double()), dlogits=_f64(x.grad))


# ---- the adjoint label scatter ---------------------------------------------------------------------------------------------------
def adjoint_scatter_ref(u, lab, C):
    """float64 scatter of da_warp_adjoint_labels: B[n][c][s] = the trilinear weight that the target voxels of label c put on source voxel s, A[n][s] the same
    for the target voxels whose label is outside [0, C).  u: N x D x H x W x 3 fp32 field, lab: N x D x H x W integer labels.  Voxels with a non-finite or
    huge coordinate contribute nothing.  Returns (A, B) as N x V and N x C x V."""
    N, D, H, W = lab.shape
    V = D * H * W
    zz, yy, xx = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing='ij')
    scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)])
    ident = torch.stack([xx * scale[0] - 1, yy * scale[1] - 1, zz * scale[2] - 1], -1).double()
    l = lab.long()
    cls = torch.where((l >= 0) & (l < C), l, torch.full_like(l, C))
    ref = torch.zeros((N, C + 1, V), dtype=torch.float64)
    grid = u.double() + ident
    fin = (grid.abs() < HUGE).all(-1) & ~torch.isnan(grid).any(-1)
    pos = [((torch.nan_to_num(grid[..., a]) + 1) / 2) * (s - 1) for a, s in ((0, W), (1, H), (2, D))]
    p0 = [torch.floor(q) for q in pos]
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                ix, iy, iz = p0[0] + cx, p0[1] + cy, p0[2] + cz
                wgt = ((pos[0] - p0[0]) if cx else (p0[0] + 1 - pos[0])) * ((pos[1] - p0[1]) if cy else (p0[1] + 1 - pos[1])) * ((pos[2] - p0[2]) if cz else (p0[2] + 1 - pos[2]))
                ok = fin & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H) & (iz >= 0) & (iz < D)
                for n in range(N):
                    sel = ok[n]
                    dst = cls[n][sel] * V + ((iz[n][sel] * H + iy[n][sel]) * W + ix[n][sel]).long()
                    ref[n].view(-1).index_add_(0, dst, wgt[n][sel])
    return ref[:, C], ref[:, :C]
