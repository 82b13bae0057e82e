"""CPU companion of tests/test_gpu_loss_shapes.py (no GPU): on the SAME derandomised examples (tests/loss_cases.py run_cases), the fp32 CPU oracle
(oracle/losses.py, torch.softmax) must sit within a quarter of each family's tolerance of its own float64 evaluation.  That makes the device
test's tolerance a statement about the kernel and not about the conditioning of the generated inputs, and it stops a later edit of the strategies
from drifting into ill-conditioned territory.  LNCC is the exception (its window variances cancel; the device test bounds it by the fp32 oracle's own
distance): here only that distance is kept below loss_cases.LNCC_EREF_MAX.  The integer label references are checked against torch's own operations."""
import numpy as np
import torch

import loss_cases as lc


def _quarter(family, key):
    return lc.TOL[family][key] / 4


def test_dice_inputs_are_well_conditioned():
    def body(case):
        inp = lc.build_dice(case)
        l32, g32 = lc.ref_dice(inp, torch.float32)
        l64, g64 = lc.ref_dice(inp, torch.float64)
        lc.close('cpu dice', 'loss', l32, l64, _quarter('dice', 'loss'), 'abs')
        lc.close('cpu dice', 'grad', g32, g64, _quarter('dice', 'grad'))
    lc.run_cases(lc.DICE, body, pinned=lc.DICE_PINNED)


def test_softmax_inputs_are_well_conditioned():
    def body(case):
        inp = lc.build_softmax(case)
        y32, d32 = lc.ref_softmax(inp, torch.float32)
        y64, d64 = lc.ref_softmax(inp, torch.float64)
        lc.close('cpu softmax', 'fwd', y32, y64, _quarter('softmax', 'fwd'))
        lc.close('cpu softmax', 'bwd', d32, d64, _quarter('softmax', 'bwd'))
    lc.run_cases(lc.SOFTMAX, body, pinned=lc.SOFTMAX_PINNED)


def test_cross_entropy_family_inputs_are_well_conditioned():
    def body(case):
        inp = lc.build_xent(case)
        l32, g32 = lc.ref_xent(inp, torch.float32)
        l64, g64 = lc.ref_xent(inp, torch.float64)
        lc.close('cpu xent', 'loss', l32, l64, _quarter('xent', 'loss'), 'rel1')
        lc.close('cpu xent', 'grad', g32, g64, _quarter('xent', 'grad'))
    lc.run_cases(lc.XENT, body, pinned=lc.XENT_PINNED)


def test_ncc_inputs_are_well_conditioned():
    def body(case):
        inp = lc.build_ncc(case)
        r32, r64 = lc.ref_ncc(inp, torch.float32), lc.ref_ncc(inp, torch.float64)
        lc.close('cpu ncc', 'loss', r32[0], r64[0], _quarter('ncc', 'loss'), 'abs')
        for a, b in zip(r32[1:], r64[1:]):
            if b is not None:
                lc.close('cpu ncc', 'grad', a, b, _quarter('ncc', 'grad'))
    lc.run_cases(lc.NCC, body, pinned=lc.NCC_PINNED)


def test_bending_and_gradient_loss_inputs_are_well_conditioned():
    def body(case):
        inp = lc.build_reg(case)
        l32, g32 = lc.ref_bending(inp, torch.float32)
        l64, g64 = lc.ref_bending(inp, torch.float64)
        lc.close('cpu bending', 'loss', l32, l64, _quarter('bending', 'loss_' + inp['norm']), 'rel')
        lc.close('cpu bending', 'grad', g32, g64, _quarter('bending', 'grad'))
        l32, g32 = lc.ref_gradloss(inp, torch.float32)
        l64, g64 = lc.ref_gradloss(inp, torch.float64)
        lc.close('cpu gradloss', 'loss', l32, l64, _quarter('gradloss', 'loss'), 'rel1')
        lc.close('cpu gradloss', 'grad', g32, g64, _quarter('gradloss', 'grad'))
    lc.run_cases(lc.REG, body, pinned=lc.REG_PINNED)


def test_lncc_yardstick_stays_meaningful():
    """No quarter rule for LNCC: only that the fp32 oracle itself stays within LNCC_EREF_MAX of float64 on every drawn window."""
    def body(case):
        inp = lc.build_lncc(case)
        e_loss, e_grad = lc.lncc_eref(inp, lc.ref_lncc(inp, torch.float64))
        lc.note('cpu lncc', 'e_ref ' + lc.lncc_class(case), e_grad)
        assert e_loss < lc.LNCC_EREF_MAX and e_grad < lc.LNCC_EREF_MAX, (case, e_loss, e_grad)
    lc.run_cases(lc.LNCC, body, pinned=lc.LNCC_PINNED)
    lc.run_cases(lc.LNCC_MS, body, pinned=lc.LNCC_MS_PINNED)


def test_label_references_agree_with_torch():
    """The numpy references of the bit-exact label tests against torch's own scatter / max / comparisons."""
    from oracle import losses

    def one_hot(case):
        mask = lc.build_one_hot(case)
        assert np.array_equal(lc.ref_one_hot(mask, case['C']), losses.mask_to_one_hot(mask, case['C']).numpy())

    def argmax(case):
        logits, truth = lc.build_argmax(case)
        counts, pred = lc.ref_argmax(logits, truth)
        tp = torch.max(logits, 1)[1]
        assert np.array_equal(pred, tp.numpy())
        oh_p, oh_t = losses.mask_to_one_hot(tp.unsqueeze(1), case['C']), losses.mask_to_one_hot(truth.unsqueeze(1), case['C'])
        n = logits.shape[0]
        ref = torch.stack([oh_p.reshape(n, case['C'], -1).sum(2), oh_t.reshape(n, case['C'], -1).sum(2), (oh_p * oh_t).reshape(n, case['C'], -1).sum(2)], 2)
        assert np.array_equal(counts, ref.numpy().astype(np.int64))

    def overlap(case):
        p, t = lc.build_overlap(case)
        counts = lc.ref_counts(p.numpy().astype(np.int64), t.numpy().astype(np.int64), case['C'])
        c = torch.arange(case['C']).view(1, -1, 1)
        pl, tl = p.long().unsqueeze(1), t.long().unsqueeze(1)
        ref = torch.stack([(pl == c).sum(2), (tl == c).sum(2), ((pl == c) & (tl == c)).sum(2)], 2)
        assert np.array_equal(counts, ref.numpy())
    lc.run_cases(lc.ONE_HOT, one_hot, pinned=lc.ONE_HOT_PINNED)
    lc.run_cases(lc.ARGMAX, argmax, pinned=lc.ARGMAX_PINNED)
    lc.run_cases(lc.OVERLAP, overlap, pinned=lc.OVERLAP_PINNED)


def test_both_files_see_the_same_examples():
    """run_cases is seeded: two runs of one strategy with different bodies see the same cases in the same order, the explicit per-branch ones first."""
    a, b = [], []
    lc.run_cases(lc.XENT, a.append, pinned=lc.XENT_PINNED)
    lc.run_cases(lc.XENT, lambda case: b.append(dict(case)), pinned=lc.XENT_PINNED)
    assert a == b and a[:len(lc.XENT_PINNED)] == lc.XENT_PINNED
    assert {c['C'] for c in lc.XENT_PINNED} == set(lc.XENT_C) and {c['C'] for c in lc.DICE_PINNED} == set(lc.DICE_C)
    assert {c['C'] for c in lc.SOFTMAX_PINNED} == set(lc.DICE_C) and {c['C'] for c in lc.ARGMAX_PINNED} == set(lc.DICE_C)
