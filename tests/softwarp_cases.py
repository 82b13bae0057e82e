"""Shared by tests/test_gpu_softwarp_dice.py (the kernels against float64) and tests/test_softwarp_reference.py (the fp32 CPU composition against float64,
no GPU): cases, builders, float64 references and tolerances for the Dice between a WARPED LABEL MAP and a DENSE tensor -- ops.LabelWarpSoftDiceFn
(registration phase of a pair whose fixed image is unlabelled: source = warp(onehot(lab_m)), target = probabilities, gradient to the displacement) and
ops.SoftmaxLabelWarpDiceFn (segmentation phase: source = softmax(logits), target = the warped one-hot, gradient to the logits).  Built on tests/warp_cases.py
(fields, label maps, one-hot, the reference's grid) and tests/loss_cases.py (run_cases, the worst-case record); record keys 'softlwd/...', 'softseg/...'.

Reference: torch-CPU float64 -- oracle.nets.warp_trilinear(one_hot(lab_m)) on the float64 grid of warp_cases._grid, F.softmax, oracle.losses.dice_loss with a
5-D (soft) target, gradients by autograd.  None of it is the code under test.  The probabilities of the registration-phase term are an INPUT (the fp32
softmax of logits of scale 3, the same tensor on both sides); the logits of the segmentation-phase term have scale 3 as in warp_cases.build_seg.

Plain module, no fixtures, no pytest settings."""
import torch
from hypothesis import strategies as st

import warp_cases as wc
from warp_cases import run_cases, note, close, close_either, rnd, _cyc, _f64, _leaf, _grid, build_field, wild_labels, one_hot, off_lattice   # noqa: F401
from oracle import losses, nets

SOFT_C = [4, 8, 16, 32, 64]                      # ops.fused_anatomy_supported
DECLINED_C = [12, 65]                            # da_softwarp_dice_* return DA_ERR_UNSUPPORTED; the ops compose WarpLabelsFn + DiceFn
VOLS = [(3, 5, 17), (5, 7, 11), (2, 9, 29), (4, 9, 25), (7, 9, 60)]      # V = 255, 385, 522, 900, 3780: cdiv(V, 512) = 1, 1, 2, 2, 8 workgroups per sample
WEIGHTS = wc.WEIGHTS
AMPS = wc.AMPS

# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# CEIL: what the suite already asserts for the same quantities (warp_cases.CEIL 'lwd' and 'segphase').  TOL follows warp_cases.TOL's rule: where the worst
# case measured on an MI355X (table in test_gpu_softwarp_dice.py) is more than 10 x below the ceiling, max(4 x device worst, 8 x fp32-CPU-oracle worst)
# rounded up to two digits; otherwise the ceiling stays.  Losses in units of max(1, |loss|), gradients as max(rel-l2, max-abs / max|ref|).
CEIL = {
    'softlwd': {'loss': 2e-6, 'd_disp': 1e-4},
    'softseg': {'loss': 1e-5, 'dlogits': 1e-4},
}
TOL = {
    'softlwd': {'loss': 3.0e-7, 'd_disp': 8.3e-6},       # device 5.4e-8 / 1.1e-6 (lattice fields 4.1e-7), fp32 composition 3.7e-8 / 1.04e-6
    'softseg': {'loss': 3.1e-7, 'dlogits': 6.7e-5},      # device 6.5e-8 / 7.4e-6, fp32 composition 3.9e-8 / 8.3e-6
}
assert all(TOL[f][k] <= CEIL[f][k] for f in CEIL for k in CEIL[f])

# ---- cases -----------------------------------------------------------------------------------------------------------------------
# da_softwarp_dice_fwd / _bwd_logits: one kernel instance per class count (C / 4 = 1, 2, 4, 8, 16 lanes per voxel), grid (cdiv(V, 512), N), a workgroup's range in
# whole 256-voxel steps, remapped through da_xcd_item_of_block when the grid is a multiple of 8 (7 x 9 x 60); V % 64 != 0 everywhere: partial waves.
# da_softwarp_dice_bwd_disp: one kernel over N V voxels (da_xcd_loop).
_vol = st.one_of(st.tuples(st.integers(2, 5), st.integers(2, 7), st.integers(2, 37)), st.sampled_from(VOLS))
CASES = st.fixed_dictionaries(dict(
    C=st.sampled_from(SOFT_C), n=st.integers(1, 2), vol=_vol, amp=st.sampled_from(AMPS), wt=st.sampled_from(WEIGHTS), no_bg=st.booleans(), wm=st.booleans(),
    km=st.sampled_from(['iid', 'blocky', 'const']), wild=st.booleans(), gl=st.sampled_from([0.37, -1.9, 2.5]), sd=st.integers(0, 999)))


def _c(C, n, vol, i, **kw):
    d = dict(C=C, n=n, vol=vol, amp=_cyc(AMPS, i), wt=_cyc(WEIGHTS, i), no_bg=i % 2 == 1, wm=i % 4 < 2, km=_cyc(['iid', 'blocky', 'iid', 'const'], i),
             wild=i % 3 != 1, gl=_cyc([0.37, -1.9, 2.5], i), sd=i)
    d.update(kw)
    return d


PINNED = (
    # every class count on every volume, N = 1 and 2, the other options cycling (25 consecutive indices: all weightings x no_bg, every label kind, every amplitude)
    [_c(C, 1 + (i + j) % 2, VOLS[(i + j) % 5], 5 * i + j) for i, C in enumerate(SOFT_C) for j in range(5)]
    # lattice fields and non-finite displacements
    + [_c(8, 2, (3, 5, 17), 30, field='zero'), _c(64, 1, (5, 7, 11), 31, field='zero'), _c(32, 1, (5, 7, 11), 32, field='shift', shift=(1, 0, -1)),
       _c(4, 2, (2, 9, 29), 33, field='shift', shift=(-2, 1, 0)), _c(16, 2, (3, 5, 17), 34, field='nonfinite', amp=0.3),
       _c(32, 1, (4, 9, 25), 35, field='nonfinite', amp=0.3), _c(64, 2, (3, 5, 17), 36, field='nonfinite', amp=2.0)]
)


def build(case):
    C, n, vol = case['C'], case['n'], tuple(case['vol'])
    disp = build_field(case)
    logits = rnd((n, C) + vol, case['sd'] + 2, 3.0)
    return dict(lab_m=wild_labels(case['km'], (n,) + vol, C, case['sd'], case['wm'], wild=case['wild']), C=C, disp=disp, vol=vol, wt=case['wt'],
                no_bg=case['no_bg'], gl=case['gl'], bad=wc.bad_voxels(disp, vol), logits=logits, prob=torch.softmax(logits, 1))


def ref_softlwd(inp, dtype, disp=None):
    """Dice(source = warp(onehot(lab_m)), target = prob): loss and d_disp"""
    u, _, grid = _grid(inp, dtype, disp, True)
    warped = nets.warp_trilinear(one_hot(inp['lab_m'], inp['C'], dtype), grid)
    l = losses.dice_loss(warped, inp['prob'].to(dtype), inp['C'], inp['wt'], inp['no_bg'], False, eps=1e-6)
    (l * inp['gl']).backward()
    return dict(loss=float(l.detach().double()), d_disp=_f64(u.grad))


def ref_softlwd_d_disp(inp, dtype, disp):
    return ref_softlwd(inp, dtype, disp)['d_disp']


def ref_softseg(inp, dtype):
    """Dice(source = softmax(logits), target = warp(onehot(lab_m)).detach()): loss and dlogits"""
    x = _leaf(inp['logits'], dtype)
    _, _, grid = _grid(inp, dtype, None, False)
    with torch.no_grad():
        target = nets.warp_trilinear(one_hot(inp['lab_m'], inp['C'], dtype), grid)
    l = losses.dice_loss(x, target, inp['C'], inp['wt'], inp['no_bg'], True, eps=1e-6)
    (l * inp['gl']).backward()
    return dict(loss=float(l.detach().double()), dlogits=_f64(x.grad))


cached = wc.cached
is_lattice = wc.is_lattice
lattice_sides = wc.lattice_sides
