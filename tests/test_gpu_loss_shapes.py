"""Randomised float64 parity for the kernels that turn network outputs into the number being optimised: Dice / softmax / fused softmax + Dice,
the cross-entropy family, NCC, bending energy, gradient loss, LNCC, and the integer label kernels.

Reference: oracle/losses.py (and torch.softmax) evaluated in float64 on the widened fp32 inputs; numpy integer counting for the label kernels.
The device side goes through the public surfaces (lib.loss classes / get_loss_function, ops.SoftmaxFn, ops.one_hot, ops.argmax_dice_counts,
ops.label_overlap_counts), forward and backward.  Cases, builders, references and tolerances live in tests/loss_cases.py; every family runs
`loss_cases.run_cases`: explicit examples that reach each launcher branch by construction, then 60 derandomised hypothesis examples (the settings of
test_gpu_random_shapes.py), and an assertion that at least 90 % of them ran their comparison.  tests/test_loss_reference.py runs the same examples
on the CPU and shows the fp32 oracle within a quarter of each tolerance of float64, so a tolerance here is a statement about the kernel.

Launcher branch <- sampled value
  losses.hip lpv_for (Dice fwd / bwd, softmax fwd / bwd, da_softmax_dice_fwd, argmax):  C = 4, 8, 16, 32, 64, 128, 256 -> lpv 1, 2, 4, 8, 16, 32, 64
      (slots 256 ... 4);  C = 1, 2, 3, 5, 12 (a multiple of 4 whose quarter is no power of two), 31 -> generic kernels; da_softmax_dice_fwd declines those.
      V = 8, 255, 256, 385, 2565, 2849 and drawn ragged volumes: below / equal to / far above one 256-voxel block, not multiples of 4 or 64.
  xent.hip xe_lanes:  C = 4, 8, 16, 32, 64 -> quad kernels L = 1, 2, 4, 8, 16;  C = 1, 2, 3, 5, 12, 33 -> thread per voxel;  form '2d_misaligned'
      (an M x C view 4 bytes into a buffer, which ops.XentFn hands over uncopied) with C = 4 ... 64 -> thread per voxel through the alignment test;
      C = 65 -> DA_ERR_UNSUPPORTED.
  losses.hip da_ncc_fwd (loss_cases.NCC_PINNED, one explicit example or more per line):
      x, y 16-byte aligned and (N = 1 or V % 4 == 0) -> ncc_partial_kernel<true>, float4 body from element 0 + scalar tail: V = 3 (tail only), 6, 105,
          N = 2 with V = 120;  grid capped at kBlocks: 1 x 131 x 127 x 129;  the fp32 -> double flush (first executed at 8 388 608 voxels per sample): 208^3.
      N > 1 with V % 4 = 1, 2, 3 -> ncc_partial_kernel<false>, scalar head of 3 / 2 / 1 + float4 body + tail per sample: N = 2 ... 4 with V = 105, 126, 99;
          N = 3 with V = 3 (head only);  capped grid: 2 x 131 x 127 x 129;  its body's flush: 2 x 207 x 209 x 211.
      x and y views 4 / 8 / 12 bytes past a 16-byte boundary (ops.NCCFn keeps a contiguous view uncopied), N = 1 -> <false> with head 3 / 2 / 1; N = 3 on top.
      x and y in different float4 phases (one of them 4 or 12 bytes off) -> the all-scalar loop; its own 64-step flush: 208^3 with x 4 bytes off.
      a sample that ends before the boundary (V = 2, 4 bytes off: head 3 > V) -> all scalar: test_ncc_degenerate_inputs.
  reglosses.hip da_lncc_fwd / lncc_march_ok:  F = 5, 9 at dilation 1, stride 1 -> z-marching kernels (volumes from exactly the window span: one window, to
      several x / y tiles);  F = 3, 7 -> separable passes;  LNCCLoss with smallest side 14 ... 24 -> separable passes with window 7 ... 12 at stride 2 / 3;
      smallest side 10 -> window 5, the marching form with LNCCLoss's eps.
  bending / gradient loss:  'L1' / 'L2' template variants, three spacings, normalize on / off, exactly 3 voxels on one axis (interior of one plane).

Worst case over all examples on an MI355X (distance from float64: tensors max(rel-l2, max-abs / max|ref|); values as in tests/test_gpu_ops.py), the
fp32 CPU oracle's worst case on the same examples, the ceiling (what tests/test_gpu_ops.py asserts against fp32 references) and what is asserted here:
  family / quantity            device worst   fp32 oracle worst   ceiling    asserted
  Dice loss (abs)                 9.4e-8          6.3e-8           1e-5       5.0e-7
  Dice d_src                      4.8e-7          4.8e-7           1e-4       3.9e-6
  softmax + Dice probabilities    1.5e-7            -              1e-6       1e-6    (less than 10 x below the ceiling: stays)
  softmax forward                 1.6e-7          2.0e-7           1e-6       1e-6    (less than 10 x below the ceiling: stays)
  softmax backward                3.5e-7          4.7e-7           1e-5       3.8e-6
  cross-entropy family loss       9.5e-8          1.3e-7           1e-5       1.1e-6
  cross-entropy family gradient   5.0e-7          3.6e-7           1e-4       2.9e-6
  NCC loss (abs)                  9.3e-8          1.9e-7           1e-5       1.6e-6
  NCC gradient                    1.2e-6          5.2e-7           1e-4       4.8e-6
  NCC, first voxel 0 (loss / grad) 3.7e-7 / 2.7e-6  -            1e-5 / 1e-4   the ceiling (test_ncc_unrepresentative_pivot)
  bending loss L2 / L1 (rel)      8.2e-8 / 1.0e-7 1.6e-7       1e-4 / 1e-5    1.3e-6
  bending gradient                1.3e-7          1.7e-7           1e-4       1.4e-6
  gradient-loss value             8.8e-8          1.1e-7           1e-5       8.6e-7
  gradient-loss gradient          1.2e-7          1.5e-7           1e-5       1.3e-6
  LNCC value                      1.1e-6            -              1e-4       4.6e-6
  LNCC gradients                  3.3e-6        (e_ref, below)     2e-4       max(1.4e-5, 2 e_ref)
Asserted = max(4 x device worst, 8 x fp32 oracle worst) wherever that is more than 10 x below the ceiling (loss_cases.TOL says why the oracle enters).
rel-l2 and max-abs are both below the figure given (the larger of the two is recorded).

LNCC per example class: e_ref = the fp32 CPU oracle's distance from float64 (gradients, worst example), next to the device's:
  class                                 e_ref      device gradient   device value
  marching F = 5                        4.7e-6        2.0e-6           6.9e-7
  marching F = 9                        2.6e-5        3.0e-6           8.0e-7
  separable F = 3                       3.5e-6        3.3e-6           1.1e-6
  separable F = 7                       8.8e-6        2.0e-6           6.4e-7
  multi-scale, window 7 ... 12 strided  1.2e-5        9.3e-7           1.4e-7
  multi-scale, window 5 (marching)      2.3e-6        6.0e-7           1.0e-7
  multi-scale, stride 1 (window 3 ... 6) 2.1e-6       7.0e-7           1.1e-7
On these inputs e_ref never reaches 1e-4, and where it is largest (F = 9, the strided multi-scale windows) the device is several times closer to float64
than the fp32 oracle: the running plane sums of the marching form cost less than the oracle's own conv3d order.  No finding about a summation order.
(The images are correlated by construction, J = 0.6 I + 0.4 noise.  Between independent images the window cross term cancels to noise, and with the few
windows of a volume near the span the fp32 oracle's own gradient was 1e-3 from float64 at F = 9: a statement about the inputs, not about a kernel.)
"""
import numpy as np
import pytest
import torch

import loss_cases as lc
from test_gpu_ops import cl, dev

pytestmark = pytest.mark.gpu


def _grad_leaf(t, want=True):
    return cl(t).requires_grad_(bool(want))


# ---- Dice ------------------------------------------------------------------------------------------------------------------------
def test_dice_random_shapes():
    """DiceLossMultiClass: every lpv and the generic form, all weightings, no_bg, logits or probabilities, both label widths, soft targets, label maps
    with absent classes; loss and d_src.  (The class, like the reference, refuses a spatial axis of length 1: volumes start at 2 x 2 x 2.)"""
    from deepatlas_amd.lib.loss import DiceLossMultiClass

    def body(case):
        inp = lc.build_dice(case)
        l64, g64 = lc.ref_dice(inp, torch.float64)
        x = _grad_leaf(inp['x'])
        t = cl(inp['target']) if inp['soft'] else inp['target'].to(dev())
        l = DiceLossMultiClass(n_class=inp['C'], weight_type=inp['wt'], no_bg=inp['no_bg'], softmax=inp['softmax'], eps=1e-6)(x, t)
        l.backward()
        lc.close('dice', 'loss', l.item(), l64, lc.TOL['dice']['loss'], 'abs')
        lc.close('dice', 'grad', x.grad, g64, lc.TOL['dice']['grad'])
    lc.run_cases(lc.DICE, body, pinned=lc.DICE_PINNED)


def test_softmax_dice_direct_entry():
    """da_softmax_dice_fwd (the Dice partial kernel that also writes softmax(src); in Python only SegPhaseLossFn reaches it) called directly for every class
    count: loss, the coefficients through da_dice_bwd, and the probabilities, against float64; a class count of the generic form is declined with
    DA_ERR_UNSUPPORTED (callers then run da_dice_fwd + da_softmax_fwd)."""
    from deepatlas_amd import ops, _native as nat
    call, ptr = nat.call, nat.ptr
    d, h, w = 5, 7, 11
    for i, C in enumerate(lc.DICE_C):
        for wide in (False, True):
            N = 1 + (i + wide) % 3
            V = d * h * w
            inp = dict(x=lc.rnd((N, C, d, h, w), 100 + i, 3.0), target=lc.labels_for(lc._cyc(['iid', 'sparse', 'blocky'], i + wide), (N, d, h, w), C, i, wide), C=C,
                       wt=lc._cyc(['Uniform', 'Simple', 'Volume'], i + wide), no_bg=(i % 2 == 1) and C > 1, softmax=True, soft=False)
            a = ops.ndhwc(cl(inp['x']))
            lab, nbytes = ops._labels(inp['target'].to(dev()).reshape(N, -1))
            prob, loss, coef = torch.empty_like(a), torch.empty(1, device=dev()), torch.empty((2, N, C), device=dev())
            wp, wn = ops._ws(nat.lib().da_dice_ws_bytes(N, V, C), a)
            ok = nat.call_supported('da_softmax_dice_fwd', ptr(a), ptr(lab), nbytes, ptr(prob), N, V, C, ops._WEIGHT_TYPES[inp['wt']], int(inp['no_bg']), 1e-6,
                                    ptr(loss), ptr(coef), wp, wn, nat.stream())
            assert ok == (lc.DICE_LPV[C] > 0), C
            if not ok:
                continue
            d_src, one = torch.empty_like(a), torch.ones(1, device=dev())
            call('da_dice_bwd', ptr(a), ptr(lab), nbytes, None, ptr(coef), ptr(one), ptr(d_src), N, V, C, 1, nat.stream())
            l64, g64 = lc.ref_dice(inp, torch.float64)
            lc.close('dice', 'loss', loss.item(), l64, lc.TOL['dice']['loss'], 'abs')
            lc.close('dice', 'grad', ops.ncdhw(d_src), g64, lc.TOL['dice']['grad'])
            lc.close('dice', 'prob', ops.ncdhw(prob), torch.softmax(inp['x'].double(), 1), lc.TOL['dice']['prob'])


# ---- softmax ---------------------------------------------------------------------------------------------------------------------
def test_softmax_random_shapes():
    """ops.SoftmaxFn forward and backward: logits of scale 4, saturated rows of scale 80, per-voxel offsets of +-100 (overflow / underflow without the max
    subtraction), a row with one dominant logit."""
    from deepatlas_amd import ops

    def body(case):
        inp = lc.build_softmax(case)
        y64, d64 = lc.ref_softmax(inp, torch.float64)
        x = _grad_leaf(inp['x'])
        y = ops.SoftmaxFn.apply(x)
        y.backward(cl(inp['go']))
        lc.close('softmax', 'fwd', y, y64, lc.TOL['softmax']['fwd'])
        lc.close('softmax', 'bwd', x.grad, d64, lc.TOL['softmax']['bwd'])
    lc.run_cases(lc.SOFTMAX, body, pinned=lc.SOFTMAX_PINNED)


# ---- cross-entropy family --------------------------------------------------------------------------------------------------------
def _xent_device(inp):
    from deepatlas_amd.lib.loss import get_loss_function
    if inp['form'] == '2d_misaligned':
        M, C = inp['x'].shape
        buf = torch.zeros(M * C + 1, device=dev())
        x = buf[1:].view(M, C)                                   # contiguous, 4 bytes past the allocation's (>= 256-byte) alignment
        x.copy_(inp['x'])
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        x.requires_grad_(True)
    else:
        x = _grad_leaf(inp['x'])
    lab = inp['labels'].to(dev())
    if inp['mode'] == 'ce':
        l = get_loss_function('cross_entropy')(ignore_index=inp['ignore'], reduction='mean' if inp['mean'] else 'sum')(x, lab)
    elif inp['mode'] == 'focal':
        l = get_loss_function('focal')(inp['C'], alpha=inp['alpha'], gamma=inp['gamma'], size_average=inp['mean'], soft_max=inp['softmax'])(x, lab)
    else:
        l = get_loss_function('soft_cross_entropy')(n_class=inp['C'], softmax=inp['softmax'])(x, cl(inp['soft_target']))
    l.backward()
    return l.item(), x.grad


def test_cross_entropy_family_random_shapes():
    """'cross_entropy' (mean / sum, an ignore_index that occurs / does not), 'focal' (alpha, gamma 0 / 1.5 / 2, soft_max, size_average) and
    'soft_cross_entropy' (softmax on / off) on 5-D logits and the M x C form, every quad kernel and the thread-per-voxel form, including the quad class
    counts from a misaligned pointer (ops.XentFn keeps a contiguous 2-D view uncopied, so the misalignment reaches xe_lanes)."""
    def body(case):
        inp = lc.build_xent(case)
        l64, g64 = lc.ref_xent(inp, torch.float64)
        l, g = _xent_device(inp)
        lc.close('xent', 'loss', l, l64, lc.TOL['xent']['loss'], 'rel1')
        lc.close('xent', 'grad', g, g64, lc.TOL['xent']['grad'])
    lc.run_cases(lc.XENT, body, pinned=lc.XENT_PINNED)


def test_cross_entropy_refuses_more_than_64_classes():
    from deepatlas_amd import _native as nat
    from deepatlas_amd.lib.loss import get_loss_function
    x = cl(lc.rnd((1, 65, 2, 3, 4), 1))
    with pytest.raises(nat.NativeError, match='da_xent_fwd failed: DA_ERR_UNSUPPORTED'):
        get_loss_function('cross_entropy')()(x, torch.zeros((1, 2, 3, 4), dtype=torch.uint8, device=dev()))


# ---- NCC -------------------------------------------------------------------------------------------------------------------------
def _offset_leaf(t, off, want):
    """`t` on the device as a leaf; off > 0: a contiguous view that starts `off` floats past the allocation's (>= 256-byte) alignment."""
    if not off:
        return _grad_leaf(t, want)
    buf = torch.zeros(t.numel() + off, device=dev())
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v.requires_grad_(bool(want))


def _ncc_body(case, tol=None, tag=''):
    from deepatlas_amd.lib.loss import NormalizedCrossCorrelationLoss
    tol = tol or lc.TOL['ncc']
    inp = lc.build_ncc(case)
    l64, gx64, gy64 = lc.ref_ncc(inp, torch.float64)
    x, y = _offset_leaf(inp['x'], inp['off'][0], 'x' in inp['grads']), _offset_leaf(inp['y'], inp['off'][1], 'y' in inp['grads'])
    l = NormalizedCrossCorrelationLoss()(x, y)
    l.backward()
    lc.close('ncc', 'loss' + tag, l.item(), l64, tol['loss'], 'abs')
    for g, g64 in ((x.grad, gx64), (y.grad, gy64)):
        assert (g is None) == (g64 is None)
        if g64 is not None:
            lc.close('ncc', 'grad' + tag, g, g64, tol['grad'])


def test_ncc_random_shapes():
    """NormalizedCrossCorrelationLoss for N = 1 ... 4 and every residue of V mod 4 (a batch with V % 4 != 0 starts its later samples off a 16-byte boundary),
    V from 3 upward, images with a mean far from zero, gradient to x, y or both, 5-D and flattened inputs.  The explicit examples (loss_cases.NCC_PINNED) hold
    the case that showed the raw-product sums, every head length, misaligned views, the all-scalar form, the grid cap and, above 8.4 M voxels per sample,
    the fp32 -> double flush of each loop."""
    lc.run_cases(lc.NCC, _ncc_body, pinned=lc.NCC_PINNED)


def test_ncc_degenerate_inputs():
    """Where the reference's NCC is 0 / 0: a constant image, and V = 1.  The kernel sums x - x[0] (losses.hip), so a constant gives exactly zero sums and a zero
    variance like the reference's x - mean, and the loss is NaN here as there.  V = 2 is |ncc| = 1 exactly with a zero gradient: the loss is compared, the
    gradient only bounded."""
    from deepatlas_amd.lib.loss import NormalizedCrossCorrelationLoss
    from oracle import losses
    crit = NormalizedCrossCorrelationLoss()
    for shape in ((1, 1, 1, 1, 1), (2, 1, 3, 5, 7), (1, 1, 4, 8, 8)):
        x, y = torch.full(shape, 0.3), lc.rnd(shape, 3) * 0.5 + 0.25
        assert not np.isfinite(float(losses.ncc_loss(x.double(), y.double())))
        assert not np.isfinite(crit(x.to(dev()), y.to(dev())).item()), shape
    x, y = torch.tensor([[0.25, 1.5], [3.0, -1.0]]), torch.tensor([[2.0, 0.5], [1.0, -4.0]])       # ncc = -1, +1 -> loss 1
    for off in (0, 1):                                      # off = 1, N = 1: the sample ends before the next 16-byte boundary (head 3 > V) -> all scalar
        xs, ys = (x, y) if off == 0 else (x[:1], y[:1])
        xg = _offset_leaf(xs, off, True)
        l = crit(xg, _offset_leaf(ys, off, False))
        l.backward()
        assert abs(l.item() - float(losses.ncc_loss(xs.double(), ys.double()))) < lc.TOL['ncc']['loss']
        assert float(xg.grad.abs().max()) < 1e-5            # exact value 0; terms of order 1 cancel in fp32


def test_ncc_unrepresentative_pivot():
    """The kernel sums x - x[0], y - y[0]: that removes mean^2 from the one-pass variance only when the first voxel is representative.  With a first voxel
    of 0 under an image of mean 6.5 (a background corner under a shifted intensity range) the sums are the raw ones again and their conditioning is
    mean^2 / variance = 56: what is guaranteed then is the suite's ceiling, not the tightened tolerance.  The figure is recorded as 'ncc/... first voxel 0'."""
    for case in (dict(n=2, vol=(16, 32, 32), offset=5.0, slope=0.7, grads='xy', flat=True, sd=21, first_zero=True),
                 dict(n=1, vol=(1, 1, 6), offset=5.0, slope=0.7, grads='xy', flat=True, sd=881, first_zero=True)):
        lc._state['case'] = case
        _ncc_body(case, tol=lc.CEIL['ncc'], tag=' first voxel 0')


# ---- bending energy, gradient loss -----------------------------------------------------------------------------------------------
def test_bending_and_gradient_loss_random_shapes():
    """BendingEnergyLoss and gradientLoss on the same drawn fields: N 1 ... 3, ragged volumes from the stencil's minimum of 3 (exactly 3 on one axis in two
    cases of five), 'L1' / 'L2', isotropic, scaled and anisotropic spacing, normalize on / off."""
    from deepatlas_amd.lib.loss import BendingEnergyLoss, get_loss_function

    def body(case):
        inp = lc.build_reg(case)
        kw = dict(norm=inp['norm'], spacing=inp['spacing'], normalize=inp['normalize'])
        for fam, crit, ref, key, kind in (('bending', BendingEnergyLoss(**kw), lc.ref_bending, 'loss_' + inp['norm'], 'rel'),
                                          ('gradloss', get_loss_function('gradient')(**kw), lc.ref_gradloss, 'loss', 'rel1')):
            l64, g64 = ref(inp, torch.float64)
            u = _grad_leaf(inp['u'])
            l = crit(u)
            l.backward()
            lc.close(fam, key, l.item(), l64, lc.TOL[fam][key], kind)
            lc.close(fam, 'grad ' + inp['norm'], u.grad, g64, lc.TOL[fam]['grad'])
    lc.run_cases(lc.REG, body, pinned=lc.REG_PINNED)


def test_bending_and_gradient_loss_below_the_stencil():
    """Fewer than 3 voxels on an axis: the reference takes the mean of an empty interior (NaN); the launchers refuse the shape with DA_ERR_BADARG."""
    from deepatlas_amd import _native as nat
    from deepatlas_amd.lib.loss import BendingEnergyLoss, get_loss_function
    from oracle import losses
    u = lc.rnd((1, 3, 2, 5, 6), 1)
    assert not np.isfinite(float(losses.bending_energy_loss(u.double()))) and not np.isfinite(float(losses.gradient_loss(u.double())))
    with pytest.raises(nat.NativeError, match='da_bending_fwd failed: DA_ERR_BADARG'):
        BendingEnergyLoss()(cl(u))
    with pytest.raises(nat.NativeError, match='da_gradloss_fwd failed: DA_ERR_BADARG'):
        get_loss_function('gradient')()(cl(u))


# ---- LNCC ------------------------------------------------------------------------------------------------------------------------
def _lncc_body(make_crit):
    def body(case):
        inp = lc.build_lncc(case)
        r64 = lc.ref_lncc(inp, torch.float64)
        e_loss, e_ref = lc.lncc_eref(inp, r64)
        cls = lc.lncc_class(case)
        I, J = inp['I'].to(dev()).requires_grad_('I' in inp['grads']), inp['J'].to(dev()).requires_grad_('J' in inp['grads'])
        l = make_crit(inp)(I, J)
        l.backward()
        lc.note('lncc', 'e_ref ' + cls, e_ref)
        lc.close('lncc', 'loss ' + cls, l.item(), r64[0], lc.TOL['lncc']['loss'], 'rel1')
        for g, g64 in ((I.grad, r64[1]), (J.grad, r64[2])):
            assert (g is None) == (g64 is None)
            if g64 is not None:
                # the fp32 oracle itself drifts from float64 as the window grows: the kernels do the same fp32 arithmetic in another order and may cost
                # the same order of error, not more -- 2 x the oracle's own distance, never below the suite's LNCC tolerance
                lc.close('lncc', 'grad ' + cls, g, g64, max(lc.TOL['lncc']['grad'], 2 * e_ref))
    return body


def test_lncc_random_shapes():
    """VoxelMorphLNCC (registry 'lncc') with windows 3, 5, 7, 9 (5 and 9: z-marching kernels; 3 and 7: separable passes), volumes from exactly the window
    span upward, one- and two-sided gradients."""
    from deepatlas_amd.lib.loss import get_loss_function
    lc.run_cases(lc.LNCC, _lncc_body(lambda inp: get_loss_function('lncc')(filter_size=inp['F']).to(dev())), pinned=lc.LNCC_PINNED)


def test_lncc_multiscale_random_shapes():
    """LNCCLoss at a smallest side <= 24: one scale, window ms // 2, stride max((k + 1) // 4, 1) -- the separable form with a stride from ms = 14 on."""
    from deepatlas_amd.lib.loss import LNCCLoss
    lc.run_cases(lc.LNCC_MS, _lncc_body(lambda inp: LNCCLoss()), pinned=lc.LNCC_MS_PINNED)


# ---- label kernels: bit-exact against numpy ---------------------------------------------------------------------------------------
def test_one_hot_random_shapes():
    from deepatlas_amd import ops

    def body(case):
        mask = lc.build_one_hot(case)
        assert np.array_equal(ops.one_hot(mask.to(dev()), case['C']).cpu().numpy(), lc.ref_one_hot(mask, case['C']))
    lc.run_cases(lc.ONE_HOT, body, pinned=lc.ONE_HOT_PINNED)


def test_argmax_dice_counts_random_shapes():
    """Logits on 1, 2 or 4 integer levels: exact ties everywhere, the first maximum wins (torch.max), across the lanes of a voxel too."""
    from deepatlas_amd import ops

    def body(case):
        logits, truth = lc.build_argmax(case)
        counts, pred = ops.argmax_dice_counts(cl(logits), truth.to(dev()))
        ref_counts, ref_pred = lc.ref_argmax(logits, truth)
        assert np.array_equal(pred.cpu().numpy(), ref_pred.astype(np.uint8))
        assert np.array_equal(counts.cpu().numpy(), ref_counts)
    lc.run_cases(lc.ARGMAX, body, pinned=lc.ARGMAX_PINNED)


def test_label_overlap_counts_random_shapes():
    """C up to 1024, uint8 / int64 on either side, labels outside [0, C) (negative ones for int64) ignored, long runs and ragged lengths."""
    from deepatlas_amd import ops

    def body(case):
        p, t = lc.build_overlap(case)
        c = ops.label_overlap_counts(p.to(dev()), t.to(dev()), case['C']).cpu().numpy()
        assert np.array_equal(c, lc.ref_counts(p.numpy().astype(np.int64), t.numpy().astype(np.int64), case['C']))
    lc.run_cases(lc.OVERLAP, body, pinned=lc.OVERLAP_PINNED)
