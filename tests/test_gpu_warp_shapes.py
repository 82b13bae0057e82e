"""Randomised float64 parity for the warp family of deepatlas_amd/csrc/warp.hip: ops.WarpFn (da_warp_fwd / da_warp_bwd / da_warp_bwd_dsrc_det),
ops.WarpLabelsFn, ops.LabelWarpDiceFn, ops.SegPhaseLossFn and the raw da_warp_adjoint_labels scatter.

Reference: torch-CPU float64 (tests/warp_cases.py: float64 identity grid, F.grid_sample, one-hot maps with C + 1 channels, F.softmax, oracle.losses.dice_loss,
autograd) -- no other kernel of warp.hip stands on the reference side, so a mistake shared by make_taps, the bounds rules or the Dice finish is visible.
Every family runs `loss_cases.run_cases`: the explicit examples below, then 60 derandomised hypothesis examples, none of which leaves a comparison out.
tests/test_warp_reference.py runs the same examples on the CPU and bounds the fp32 oracle's own distance, so a tolerance here is a statement about the kernel.

Launcher branch <- explicit example (warp_cases.*_PINNED; test_pinned_cases_name_their_branches re-derives the counts from the launcher formulas)
  da_warp_fwd   warp_fwd_grouped_kernel (C = 8, 16, 32): cdiv(V, 512) blocks per sample -- 7 x 9 x 60 (V = 3780: 8 blocks, block -> range through
                    da_xcd_item_of_block), 5 x 7 x 59 (V = 2065: 5 blocks, plain order, V no multiple of 64 / 256 / 512), 2 x 2 x 2 (one partial wave), N = 2, 3
                warp_fwd_kernel<4>: C = 4, 64, 128, 256 (lpv 1, 16, 32, 64); C = 8 at N = 65536 on 2 x 2 x 2 (grid.y limit: lpv 2 outside the grouped kernel);
                    C = 64 on 2 x 7 x 9 and C = 4 on 7 x 9 x 31 (8 workgroups: da_xcd_loop's per-XCD ranges)
                warp_fwd_kernel<1>: C = 1, 3, 12 (a multiple of 4 whose quarter is no power of two), 260; C = 3 on 7 x 9 x 31 (per-XCD ranges)
  da_warp_bwd   warp_bwd_dsrc_lane_kernel + warp_bwd_kernel<4> for d_disp alone: C = 8, 16, 32, 64;  warp_bwd_kernel<4> with its own d_src atomics: C = 4, 128,
                    256;  warp_bwd_kernel<1>: C = 1, 3, 12, 260;  grads = 'src' (d_disp == nullptr; the lane kernel alone at C = 16, 64) and 'disp'
                    (d_src == nullptr) at C = 3, 4, 16, 64, 128, 260;  a non-zero upstream gradient on `deform` (gdef)
  da_warp_bwd_dsrc_det: the same examples under ops.set_deterministic(True), d_src held to the same float64 reference, two runs bit-identical
  da_warp_labels_fwd  <4>: C = 4, 8, 12, 32, 64;  <1>: C = 1, 2, 3, 5, 31;  uint8 and int64 labels, labels equal to C and C + 5, negative int64 labels
  da_label_warp_dice_fwd / _bwd: every C from 1 to 64 (V = 105, 258, 255, N = 1 ... 3), N = 64 on 2 x 2 x 3, both maps constant (one histogram key per wave),
                    C = 64 with per-voxel random labels (a wave full of keys), 7 x 9 x 60 (8 blocks: per-XCD ranges), N = 65 / C = 65 refused
  da_warp_dice_fwd    warp_dice_grouped_kernel: C = 8, 16, 32 (8 / 32 blocks remapped at 7 x 9 x 60 / 7 x 9 x 65, 15 blocks at C = 16);  warp_dice_partial_kernel:
                    C = 4 (lpv 1; 8 blocks at 6 x 18 x 70) and C = 64 (lpv 16; 8 blocks at 5 x 9 x 11)
  da_seg_anat_dlogits seg_anat_dlogits_kernel tv = 256: C = 4, 8, 16;  tv = 128: C = 64;  seg_anat_dlogits_lane_kernel<32>: C = 32;  4 x 9 x 25 with N = 2
                    (N = 1 at C = 64): 8 tiles, taken per XCD, the last one partial;  labels_m = None;  an upstream gradient on l_anat alone
  da_warp_adjoint_labels: target labels outside [0, C) in every SegPhaseLossFn example with kt = 'iid' / 'blocky' (A_extra), and the raw call below
  lattice fields (zero displacement, a whole-voxel shift) and a NaN / inf / 1e30 displacement at four voxels: one example or more per family

Worst case over all examples on an MI355X (tensors: max(rel-l2, max-abs / max|ref|); losses in units of max(1, |ref|); the adjoint scatter absolute), the
fp32 CPU oracle's worst case on the same examples, the ceiling (what the suite asserted for the quantity before) and what is asserted here:
  family / quantity                  device worst   fp32 oracle worst   ceiling    asserted
  WarpFn warped                         1.1e-5          1.1e-5           2e-5       2e-5     (less than 10 x below the ceiling: stays)
  WarpFn deform                         8.5e-8          8.5e-8           1e-6       6.8e-7
  WarpFn d_src                          8.0e-6          8.0e-6           2e-5       2e-5     (stays)
  WarpFn d_src, fixed-point             7.3e-6            -              2e-5       2e-5     (ops.set_deterministic(True); warped, deform, d_disp as above)
  WarpFn d_disp                         1.1e-6          1.2e-6           1e-4       9.8e-6
  WarpFn d_disp, lattice fields         2.9e-7          4.8e-7           1e-4       9.8e-6   (against the nearer of the two one-sided references)
  WarpLabelsFn forward                  2.9e-6          3.2e-6           1e-5       1e-5     (stays)
  WarpLabelsFn d_disp                   1.1e-6          1.1e-6           1e-5       1e-5     (9.3 x below: stays);  lattice fields 1.4e-7 / 1.4e-7
  LabelWarpDiceFn loss                  4.2e-7          8.6e-8           2e-6       2e-6     (stays)
  LabelWarpDiceFn d_disp                3.9e-6          4.4e-6           1e-4       3.5e-5   lattice fields 2.1e-7 / 2.7e-7
  SegPhaseLossFn l_sup, l_anat          4.4e-8          4.3e-8           1e-5       3.5e-7
  SegPhaseLossFn d logits               5.3e-6          5.0e-6           1e-4       4.1e-5
  da_warp_adjoint_labels A / B (abs)    5.8e-6 / 6.2e-6   -              2e-5       2e-5     (stays)
Asserted = max(4 x device worst, 8 x fp32 oracle worst) rounded up to two digits where the device's worst is more than 10 x below the ceiling, else the ceiling.
The sampled values (warped, d_src, the label warp's forward) sit where torch's own fp32 grid_sample sits: their error is the fp32 voxel coordinate's, which
grows with the axis length (1.1e-5 at 60 voxels, device and oracle alike; warp_cases.COORD_ERR); no kernel here is further from float64 than the fp32 oracle
by more than its last digit, and no comparison found a defect in warp.hip or ops.py.
"""
import numpy as np
import pytest
import torch

import warp_cases as wc
from test_gpu_ops import cl, dev

pytestmark = pytest.mark.gpu


def _d_disp(family, case, inp, got, ref, ref_d_disp, tag=''):
    """d_disp against the one float64 reference; a lattice case: against the reference on either side of the lattice point.  Exactly zero where the
    coordinate is non-finite or huge."""
    got = got.detach().cpu()
    if wc.is_lattice(case):
        wc.close_either(family, 'd_disp' + tag, got, *wc.lattice_sides(ref_d_disp, inp), wc.TOL[family]['d_disp'])
    else:
        wc.close(family, 'd_disp' + tag, got, ref, wc.TOL[family]['d_disp'])
    assert float(got[inp['bad'].expand_as(got)].abs().sum()) == 0.0


# ---- WarpFn ----------------------------------------------------------------------------------------------------------------------
def _warp_device(inp):
    from deepatlas_amd import ops
    s = cl(inp['src']).requires_grad_(inp['grads'] in ('both', 'src'))
    u = cl(inp['disp']).requires_grad_(inp['grads'] in ('both', 'disp'))
    warped, deform = ops.WarpFn.apply(s, u)
    outs, gouts = [warped], [cl(inp['go'])]
    if inp['gd'] is not None:
        outs.append(deform); gouts.append(cl(inp['gd']))
    torch.autograd.backward(outs, gouts)
    return warped.detach(), deform.detach(), s.grad, u.grad


def _warp_compare(case, inp, got, tag=''):
    r = wc.cached(wc.ref_warp, case, inp)
    warped, deform, d_src, d_disp = got
    bad = inp['bad']
    wc.close('warp', 'warped' + tag, warped, r['warped'], wc.TOL['warp']['warped'])
    zero = torch.zeros(())
    wc.close('warp', 'deform' + tag, torch.where(bad, zero, deform.cpu()), torch.where(bad, zero.double(), r['deform']), wc.TOL['warp']['deform'])
    assert (d_src is None) == (r['d_src'] is None) and (d_disp is None) == (r['d_disp'] is None)
    if d_src is not None:
        wc.close('warp', 'd_src' + tag, d_src, r['d_src'], wc.TOL['warp']['d_src'])
    if d_disp is not None:
        _d_disp('warp', case, inp, d_disp, r['d_disp'], wc.ref_warp_d_disp, tag)


def test_warp_random_shapes():
    """ops.WarpFn: warped, deform, d_src, d_disp for C in {1, 3, 4, 8, 12, 16, 32, 64, 128, 256, 260}, N 1 ... 3 (and 65536), ragged volumes up to 7 x 9 x 60,
    displacements of 0.05 ... 8 voxels, gradients to both inputs or one, with and without an upstream gradient on `deform`."""
    def body(case):
        inp = wc.build_warp(case)
        _warp_compare(case, inp, _warp_device(inp))
    wc.run_cases(wc.WARP, body, pinned=wc.WARP_PINNED)


def test_warp_deterministic_random_shapes():
    """The same examples under ops.set_deterministic(True): d_src comes from the fixed-point accumulation of da_warp_bwd_dsrc_det, is held to the same float64
    reference and tolerance, and two runs are bit-identical in every output."""
    from deepatlas_amd import ops

    def body(case):
        inp = wc.build_warp(case)
        a, b = _warp_device(inp), _warp_device(inp)
        for x, y in zip(a, b):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32)), case
        _warp_compare(case, inp, a, ' (deterministic)')
    prev = ops.set_deterministic(True)
    try:
        wc.run_cases(wc.WARP, body, pinned=wc.WARP_PINNED)
    finally:
        ops.set_deterministic(prev)


# ---- WarpLabelsFn ----------------------------------------------------------------------------------------------------------------
def test_warp_labels_random_shapes():
    """ops.WarpLabelsFn: the warp of a label map as if it were its one-hot encoding, forward and d_disp; C % 4 == 0 and != 0, uint8 / int64 labels, labels
    outside [0, C) (they count for no class)."""
    from deepatlas_amd import ops

    def body(case):
        inp = wc.build_warplabels(case)
        r = wc.cached(wc.ref_warplabels, case, inp)
        u = cl(inp['disp']).requires_grad_(True)
        out = ops.WarpLabelsFn.apply(inp['labels'].to(dev()), u, inp['C'])
        out.backward(cl(inp['go']))
        wc.close('warplabels', 'fwd', out, r['fwd'], wc.TOL['warplabels']['fwd'])
        _d_disp('warplabels', case, inp, u.grad, r['d_disp'], wc.ref_warplabels_d_disp)
    wc.run_cases(wc.WARPLABELS, body, pinned=wc.WARPLABELS_PINNED)


# ---- LabelWarpDiceFn -------------------------------------------------------------------------------------------------------------
def test_label_warp_dice_random_shapes():
    """ops.LabelWarpDiceFn: loss and d_disp for every C from 1 to 64, N 1 ... 3 and 64, the three Dice weightings, no_bg, mixed label widths, labels outside
    [0, C) in both maps, constant maps and per-voxel random ones, an upstream gradient different from 1."""
    from deepatlas_amd import ops

    def body(case):
        inp = wc.build_lwd(case)
        r = wc.cached(wc.ref_lwd, case, inp)
        u = cl(inp['disp']).requires_grad_(True)
        l = ops.LabelWarpDiceFn.apply(inp['lab_m'].to(dev()), inp['lab_t'].to(dev()), u, inp['C'], inp['wt'], inp['no_bg'], 1e-6)
        (l * inp['gl']).backward()
        wc.close('lwd', 'loss', l.item(), r['loss'], wc.TOL['lwd']['loss'], 'rel1')
        _d_disp('lwd', case, inp, u.grad, r['d_disp'], wc.ref_lwd_d_disp)
    wc.run_cases(wc.LWD, body, pinned=wc.LWD_PINNED)


def test_label_warp_dice_refuses_what_it_cannot_index():
    """N = 65 (the finish kernel's per-sample table) and C = 65 (the per-wave histogram of 64 classes) raise; nothing is written out of bounds first."""
    from deepatlas_amd import ops, _native as nat
    lab = torch.zeros((65, 2, 2, 3), dtype=torch.uint8, device=dev())
    with pytest.raises(nat.NativeError, match='da_label_warp_dice_fwd failed: DA_ERR_BADARG'):
        ops.LabelWarpDiceFn.apply(lab, lab, torch.zeros((65, 3, 2, 2, 3), device=dev()), 5, 'Uniform', False, 1e-6)
    with pytest.raises(nat.NativeError, match='da_label_warp_dice_fwd failed: DA_ERR_UNSUPPORTED'):
        ops.LabelWarpDiceFn.apply(lab[:1], lab[:1], torch.zeros((1, 3, 2, 2, 3), device=dev()), 65, 'Uniform', False, 1e-6)


# ---- the adjoint label scatter (before the last run_cases, which writes the report) -------------------------------------------------
def test_adjoint_label_scatter_with_out_of_range_labels():
    """da_warp_adjoint_labels called directly with a non-NULL A: target labels outside [0, C) (negative ones for int64) put their weights into A, the others
    into B; a NaN, a 1e30 and a far-out-of-volume coordinate contribute nothing.  Against the float64 scatter of test_adjoint_label_scatter_box_and_direct_paths
    (warp_cases.adjoint_scatter_ref)."""
    from deepatlas_amd import _native as nat
    call, ptr = nat.call, nat.ptr
    g = torch.Generator().manual_seed(17)
    N, D, H, W, C = 2, 5, 9, 37, 5
    V = D * H * W
    scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)])
    u = torch.randn((N, 1, 1, 1, 3), generator=g).expand(N, D, H, W, 3) * 0.7 * scale + torch.randn((N, D, H, W, 3), generator=g) * 0.2 * scale
    u = u.contiguous()
    u[:, ::2] = (torch.randn((N, D, H, W, 3), generator=g) * 8.0 * scale)[:, ::2]
    u[0, 3, 4, 5, 0] = float('nan'); u[1, 2, 3, 4] = 7.0; u[1, 4, 8, 36, 2] = 1e30
    zz, yy, xx = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing='ij')
    blocky = (zz // 3 + yy // 4 + xx // 13) % (C + 1)                       # piecewise constant, one region of label C
    for nbytes, lab in ((8, torch.randint(-2, C + 3, (N, D, H, W), generator=g)), (1, torch.stack([blocky, (blocky + 2) % (C + 2)]).to(torch.uint8))):
        wc.lc._state['case'] = 'adjoint raw call, %d-byte labels' % nbytes
        A_ref, B_ref = wc.adjoint_scatter_ref(u, lab, C)
        assert float(A_ref.sum()) > 1.0 and float(B_ref.sum()) > 1.0
        A, B = torch.full((N, V), 7.0, device=dev()), torch.full((N, C, V), 7.0, device=dev())      # (the launcher zero-fills both)
        ld, ud = lab.to(dev()).contiguous(), u.to(dev())                       # (held in names: ptr() keeps no reference)
        call('da_warp_adjoint_labels', ptr(ld), nbytes, ptr(ud), ptr(A), ptr(B), N, D, H, W, C, nat.stream())
        torch.cuda.synchronize()
        for what, got, ref in (('A', A, A_ref), ('B', B, B_ref)):
            assert bool(torch.isfinite(got).all())
            e = float((got.cpu().double() - ref).abs().max())
            wc.note('adjoint', what, e)
            assert e < wc.TOL['adjoint'][what], (what, nbytes, e)


# ---- SegPhaseLossFn --------------------------------------------------------------------------------------------------------------
def test_seg_phase_loss_random_shapes():
    """ops.SegPhaseLossFn: both losses and the gradient with respect to the logits (float64 softmax -> warp -> Dice, and the supervised Dice) for C in
    {4, 8, 16, 32, 64}, N 1 / 2, with and without labels_m, mixed label widths, target labels outside [0, C), arbitrary upstream gradients on both outputs or
    on l_anat alone."""
    from deepatlas_amd import ops

    def body(case):
        inp = wc.build_seg(case)
        r = wc.cached(wc.ref_seg, case, inp)
        x = cl(inp['logits']).requires_grad_(True)
        lab_m = inp['lab_m'].to(dev()) if inp['lab_m'] is not None else None
        l_sup, l_anat = ops.SegPhaseLossFn.apply(x, lab_m, cl(inp['disp']), inp['lab_t'].to(dev()), inp['wt'], inp['no_bg'], 1e-6)
        tot = l_anat * inp['ga']
        if inp['gs'] is not None:
            tot = tot + l_sup * inp['gs']                    # (labels_m = None: l_sup is the constant 0 and its upstream gradient must change nothing)
        tot.backward()
        wc.close('segphase', 'loss', l_sup.item(), r['l_sup'], wc.TOL['segphase']['loss'], 'rel1')
        wc.close('segphase', 'loss', l_anat.item(), r['l_anat'], wc.TOL['segphase']['loss'], 'rel1')
        wc.close('segphase', 'dlogits', x.grad, r['dlogits'], wc.TOL['segphase']['dlogits'])
    wc.run_cases(wc.SEG, body, pinned=wc.SEG_PINNED)
