"""Float64 parity for the Dice between a warped label map and a dense tensor (deepatlas_amd/csrc/warp.hip da_softwarp_dice_*): ops.LabelWarpSoftDiceFn
(loss and d_disp) and ops.SoftmaxLabelWarpDiceFn (loss and dlogits).

Reference: torch-CPU float64 (tests/softwarp_cases.py: warp_trilinear of the one-hot map on the float64 grid, F.softmax, oracle.losses.dice_loss with a soft
target, autograd) -- no kernel of warp.hip stands on the reference side.  The explicit examples name every launcher branch: each C in {4, 8, 16, 32, 64} (one
kernel instance each) on 3 x 5 x 17, 5 x 7 x 11, 2 x 9 x 29, 4 x 9 x 25 and 7 x 9 x 60 (V never a multiple of 64; 1, 1, 2, 2 and 8 workgroups per sample, the
last one remapped per XCD), N = 1 and 2, the three weightings with and without no_bg, uint8 / int64 labels, iid / blocky / constant maps, labels outside
[0, C), fields of 0.05 ... 8 voxels, zero and whole-voxel shifts (d_disp held to either side), non-finite displacements; then 60 derandomised hypothesis
examples over the same axes.  tests/test_softwarp_reference.py runs the same examples on the CPU and bounds the fp32 composition's own distance.

Worst case over all examples on an MI355X, the fp32 CPU composition's worst case on the same examples, the ceiling (what the suite asserts for the same
quantity of LabelWarpDiceFn / SegPhaseLossFn) and what is asserted here (the rule of warp_cases.TOL):
  quantity                               device worst   fp32 composition worst   ceiling    asserted
  LabelWarpSoftDiceFn loss                  5.4e-8            3.7e-8              2e-6       3.0e-7
  LabelWarpSoftDiceFn d_disp                1.1e-6            1.04e-6             1e-4       8.3e-6   lattice fields 4.1e-7 / 4.1e-7 (nearer one-sided reference)
  SoftmaxLabelWarpDiceFn loss               6.5e-8            3.9e-8              1e-5       3.1e-7
  SoftmaxLabelWarpDiceFn dlogits            7.4e-6            8.3e-6              1e-4       6.7e-5
Every device figure is more than 10 x below its ceiling, so each tolerance is max(4 x device worst, 8 x fp32 composition worst) rounded up to two digits;
the second term decides all four (the kernels sum in double and sit as close to float64 as the fp32 composition does).  No comparison found a defect.
"""
import numpy as np
import pytest
import torch

import softwarp_cases as sc
from test_gpu_ops import cl, dev

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _softlwd_device(inp):
    from deepatlas_amd import ops
    u = cl(inp['disp']).requires_grad_(True)
    l = ops.LabelWarpSoftDiceFn.apply(inp['lab_m'].to(dev()), u, cl(inp['prob']), inp['C'], inp['wt'], inp['no_bg'], 1e-6)
    (l * inp['gl']).backward()
    return l.detach().reshape(1), u.grad


def _softseg_device(inp):
    from deepatlas_amd import ops
    x = cl(inp['logits']).requires_grad_(True)
    l = ops.SoftmaxLabelWarpDiceFn.apply(x, inp['lab_m'].to(dev()), cl(inp['disp']), inp['wt'], inp['no_bg'], 1e-6)
    (l * inp['gl']).backward()
    return l.detach().reshape(1), x.grad


def _compare(case, inp, lwd, seg, tag=''):
    r = sc.cached(sc.ref_softlwd, case, inp)
    sc.close('softlwd', 'loss' + tag, lwd[0].item(), r['loss'], sc.TOL['softlwd']['loss'], 'rel1')
    got = lwd[1].detach().cpu()
    if sc.is_lattice(case):
        sc.close_either('softlwd', 'd_disp' + tag, got, *sc.lattice_sides(sc.ref_softlwd_d_disp, inp), sc.TOL['softlwd']['d_disp'])
    else:
        sc.close('softlwd', 'd_disp' + tag, got, r['d_disp'], sc.TOL['softlwd']['d_disp'])
    assert float(got[inp['bad'].expand_as(got)].abs().sum()) == 0.0            # no gradient where the coordinate is non-finite or huge
    r = sc.cached(sc.ref_softseg, case, inp)
    sc.close('softseg', 'loss' + tag, seg[0].item(), r['loss'], sc.TOL['softseg']['loss'], 'rel1')
    sc.close('softseg', 'dlogits' + tag, seg[1], r['dlogits'], sc.TOL['softseg']['dlogits'])


def test_softwarp_dice_random_shapes():
    """Both functions against float64 on every example; a second run is bit-identical in every output, and so is a run under ops.set_deterministic(True)
    (the kernels hold no atomics: deterministic mode runs them as they are)."""
    from deepatlas_amd import ops

    def body(case):
        inp = sc.build(case)
        lwd, seg = _softlwd_device(inp), _softseg_device(inp)
        _compare(case, inp, lwd, seg)
        prev = ops.set_deterministic(True)
        try:
            again = _softlwd_device(inp) + _softseg_device(inp)
        finally:
            ops.set_deterministic(prev)
        for runs in (_softlwd_device(inp) + _softseg_device(inp), again):
            for a, b in zip(lwd + seg, runs):
                assert np.array_equal(_bits(a), _bits(b)), case
    sc.run_cases(sc.CASES, body, pinned=sc.PINNED)


@pytest.mark.parametrize('C', sc.DECLINED_C)
def test_declined_class_counts_fall_back_to_the_composition(C):
    """C = 12 (a multiple of 4 whose quarter is no power of two) and C = 65: the entries return DA_ERR_UNSUPPORTED and the two functions run WarpLabelsFn + DiceFn,
    held to the same float64 reference and tolerances."""
    from deepatlas_amd import _native as nat
    case = sc._c(C, 2, (3, 5, 17), 40 + C)
    inp = sc.build(case)
    lab, u, p = inp['lab_m'].to(dev()).contiguous(), cl(inp['disp']).permute(0, 2, 3, 4, 1).contiguous(), cl(inp['prob']).permute(0, 2, 3, 4, 1).contiguous()
    out, coef = torch.zeros(1, device=dev()), torch.zeros((2, 2, C), device=dev())
    wp, wn = nat.workspace.get(nat.lib().da_softwarp_dice_ws_bytes(2, C), dev())
    lb = 1 if lab.dtype == torch.uint8 else 8
    for role in (0, 1):
        with pytest.raises(nat.NativeError, match='da_softwarp_dice_fwd failed: DA_ERR_UNSUPPORTED'):
            nat.call('da_softwarp_dice_fwd', nat.ptr(lab), lb, nat.ptr(u), nat.ptr(p), role, 2, 3, 5, 17, C, 0, 0, 1e-6, nat.ptr(out), nat.ptr(coef), wp, wn, nat.stream())
    for name in ('da_softwarp_dice_bwd_disp', 'da_softwarp_dice_bwd_logits'):
        with pytest.raises(nat.NativeError, match=name + ' failed: DA_ERR_UNSUPPORTED'):
            nat.call(name, nat.ptr(lab), lb, nat.ptr(u), nat.ptr(p), nat.ptr(coef), nat.ptr(out), nat.ptr(p), 2, 3, 5, 17, C, nat.stream())
    sc.wc.lc._state['case'] = case
    _compare(case, inp, _softlwd_device(inp), _softseg_device(inp), ' (composition)')
