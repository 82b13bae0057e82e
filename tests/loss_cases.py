"""Shared by tests/test_gpu_loss_shapes.py (HIP kernels against float64) and tests/test_loss_reference.py (the fp32 CPU oracle against
float64, no GPU): hypothesis strategies that name every launcher branch of the loss / softmax / label-count kernels, builders that turn
a drawn case into well-conditioned fp32 CPU inputs, the float64 reference wrappers around oracle/losses.py, and the tolerances.

Both test files run their families through `run_cases`, ONE seeded, derandomised hypothesis function, so the CPU companion sees exactly
the examples the device test sees: what it proves about their conditioning holds for the device run.

Measuring: with DA_LOSS_SHAPES_REPORT=<path> set, run_cases writes the worst distance recorded so far per family and quantity (and the case that
gave it) to that JSON file when it returns; the tables in test_gpu_loss_shapes.py were filled from it.

Plain module, no fixtures, no pytest settings."""
import json
import os

import numpy as np
import torch
from hypothesis import given, seed, settings, example, strategies as st, HealthCheck

from conftest import rel_l2, max_abs_rel
from oracle import losses, nets

SET = dict(max_examples=60, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
MIN_COMPARED = 54          # 90 % of the 60 drawn examples must have run a comparison (nothing here drops a case, so in practice all do)


def run_cases(strategy, body, pinned=()):
    """Run `body(case)` over the `pinned` explicit examples (one per launcher branch: reached by construction, not by luck) and the 60
    derandomised examples of `strategy`; asserts that at least 90 % of them ran their comparison to the end and returns how many did."""
    ran = [0]

    def go(case):
        _state['case'] = case
        body(case)
        ran[0] += 1
    for c in reversed(list(pinned)):
        go = example(case=c)(go)
    go = seed(160950)(settings(**SET)(given(case=strategy)(go)))
    go()
    assert ran[0] >= MIN_COMPARED + len(pinned), ran[0]
    path = os.environ.get('DA_LOSS_SHAPES_REPORT')
    if path:
        with open(path, 'w') as f:
            json.dump(WORST, f, indent=1, sort_keys=True)
    return ran[0]


def _cyc(seq, i):
    return seq[i % len(seq)]


# ---- distances and the worst-case record -----------------------------------------------------------------------------------------
WORST = {}                 # 'family/what' -> [largest distance seen in this process, the case that gave it]
_state = {'case': None}    # the case run_cases is working on


def note(family, what, value):
    key = '%s/%s' % (family, what)
    if float(value) >= WORST.get(key, [0.0])[0]:
        WORST[key] = [float(value), repr(_state['case'])]


def dist(a, b):
    """check()'s two criteria as one number: max(rel-l2, largest element error in units of max|ref|)."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all(), 'non-finite values'
    return max(rel_l2(a, b), max_abs_rel(a, b))


def scalar_err(got, ref, kind):
    """'abs': |got - ref|;  'rel1': in units of max(1, |ref|);  'rel': in units of |ref|  (the three forms tests/test_gpu_ops.py uses)."""
    got, ref = float(got), float(ref)
    assert np.isfinite(got), got
    e = abs(got - ref)
    return e if kind == 'abs' else e / max(1.0, abs(ref)) if kind == 'rel1' else e / abs(ref)


def close(family, what, got, ref, tol, kind=None):
    """Record and assert one comparison: tensors by dist(), scalars by scalar_err(kind)."""
    e = scalar_err(got, ref, kind) if kind else dist(got, ref)
    note(family, what, e)
    assert e < tol, '%s %s: %.3e (tolerance %.1e)' % (family, what, e, tol)
    return e


# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# CEIL: what tests/test_gpu_ops.py asserts for the same op against fp32 references (TOL = 1e-4 of check(); 1e-5 on Dice / NCC / gradient-loss /
# cross-entropy values; bending 1e-4 ('L2') and 1e-5 ('L1') of the value; softmax 1e-6 / 1e-5; LNCC 1e-4 on the value, 2e-4 on gradients).
# TOL: what the two new files assert, never above CEIL.  Where the worst case measured on an MI355X over all examples (table in test_gpu_loss_shapes.py)
# is more than 10 x below the ceiling, the tolerance is max(4 x device worst, 8 x fp32-CPU-oracle worst) rounded up to two digits.  4 x: the examples
# are derandomised, so the margin only has to absorb compiler / runtime changes, not sampling.  The second term keeps the CPU companion's rule (fp32
# oracle within a quarter of the tolerance) satisfiable: several kernels accumulate in double and are CLOSER to float64 than the fp32 oracle is, and a
# quarter of 4 x their error would sit below the oracle's own rounding.  4 x oracle worst is exactly that rule; the further factor 2 is headroom for
# another CPU's vector width / thread count changing torch's reduction order.  That factor is a guess, not a measurement (the one figure recorded on two
# hosts, the fp32 oracle's LNCC F = 3 distance on one example, was 2.6e-6 on one CPU and 3.5e-6 on the other), and it is the one place where these
# tolerances are looser than 4 x the device's own worst case.
CEIL = {
    'dice': {'loss': 1e-5, 'grad': 1e-4, 'prob': 1e-6},
    'softmax': {'fwd': 1e-6, 'bwd': 1e-5},
    'xent': {'loss': 1e-5, 'grad': 1e-4},
    'ncc': {'loss': 1e-5, 'grad': 1e-4},
    'bending': {'loss_L2': 1e-4, 'loss_L1': 1e-5, 'grad': 1e-4},
    'gradloss': {'loss': 1e-5, 'grad': 1e-5},
    'lncc': {'loss': 1e-4, 'grad': 2e-4},
}
TOL = {
    'dice': {'loss': 5.0e-7, 'grad': 3.9e-6, 'prob': 1e-6},              # prob: 1.5e-7 measured, less than 10 x below: stays
    'softmax': {'fwd': 1e-6, 'bwd': 3.8e-6},                             # fwd: 1.6e-7 measured, less than 10 x below: stays
    'xent': {'loss': 1.1e-6, 'grad': 2.9e-6},
    'ncc': {'loss': 1.6e-6, 'grad': 4.8e-6},
    'bending': {'loss_L2': 1.3e-6, 'loss_L1': 1.3e-6, 'grad': 1.4e-6},
    'gradloss': {'loss': 8.6e-7, 'grad': 1.3e-6},
    # LNCC: no quarter rule (the fp32 oracle itself drifts); value 4 x 1.13e-6; gradients max('grad', 2 x the fp32 oracle's own distance on the example),
    # 'grad' = 4 x the 3.3e-6 measured where the suite's 2e-4 stood
    'lncc': {'loss': 4.6e-6, 'grad': 1.4e-5},
}
assert all(TOL[f][k] <= CEIL[f][k] for f in CEIL for k in CEIL[f])
LNCC_EREF_MAX = 5e-4       # the CPU companion keeps the LNCC strategies where the fp32 yardstick itself is within this of float64


def rnd(shape, sd, scale=1.0):
    g = torch.Generator().manual_seed(int(sd))
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _f64(t):
    return t.detach().to(torch.float64)


def _leaf(t, dtype, grad=True):
    """A fresh leaf holding exactly the fp32 values of `t`, widened to `dtype`."""
    return t.detach().clone().to(dtype).requires_grad_(bool(grad))


# ---- Dice ------------------------------------------------------------------------------------------------------------------------
# losses.hip lpv_for(C): C / 4 lanes per voxel when C / 4 is a power of two <= 64, else the generic kernels
DICE_C = [1, 2, 3, 4, 5, 8, 12, 16, 31, 32, 64, 128, 256]
DICE_LPV = {1: 0, 2: 0, 3: 0, 4: 1, 5: 0, 8: 2, 12: 0, 16: 4, 31: 0, 32: 8, 64: 16, 128: 32, 256: 64}
# V = 8, 255, 256, 385 and 2849 / 2565 (far above one 256-voxel block, neither a multiple of 4 nor of 64) next to the drawn ragged volumes; every axis >= 2:
# DiceLossMultiClass, like the reference (lib/loss.py:419), compares the source's extent with the SQUEEZED target's and so refuses an axis of length 1
_dice_vol = st.one_of(st.tuples(st.integers(2, 7), st.integers(2, 11), st.integers(2, 37)),
                      st.sampled_from([(2, 2, 2), (3, 5, 17), (4, 8, 8), (5, 7, 11), (7, 11, 37), (5, 9, 57)]))
DICE = st.fixed_dictionaries(dict(
    C=st.sampled_from(DICE_C), n=st.integers(1, 3), vol=_dice_vol, wt=st.sampled_from(['Uniform', 'Simple', 'Volume']), no_bg=st.booleans(),
    softmax=st.booleans(), wide=st.booleans(), target=st.sampled_from(['iid', 'blocky', 'sparse', 'soft']), sd=st.integers(0, 999)))
# one explicit example per class count (= per lpv 1 ... 64 and the generic form), the other options cycling
DICE_PINNED = [dict(C=C, n=1 + i % 3, vol=_cyc([(5, 7, 11), (3, 5, 17), (2, 9, 29)], i), wt=_cyc(['Uniform', 'Simple', 'Volume'], i), no_bg=i % 2 == 1,
                    softmax=i % 4 < 2, wide=i % 2 == 0, target=_cyc(['iid', 'blocky', 'sparse', 'soft'], i), sd=i) for i, C in enumerate(DICE_C)]


def labels_for(kind, shape, C, sd, wide):
    """(n, d, h, w) index labels: 'iid' uniform over the classes, 'blocky' piecewise constant (oracle.nets.closed_form_labels; small volumes
    leave most classes out), 'sparse' i.i.d. over every third class only (the others do not occur at all)."""
    g = torch.Generator().manual_seed(int(sd) + 7)
    if kind == 'blocky':
        lab = nets.closed_form_labels(shape, C, seed=int(sd)).long()
    elif kind == 'sparse':
        lab = (torch.randint(0, (C + 2) // 3, shape, generator=g) * 3) % C
    else:
        lab = torch.randint(0, C, shape, generator=g)
    return lab.long() if wide else lab.to(torch.uint8)


def build_dice(case):
    C, n, (d, h, w) = case['C'], case['n'], case['vol']
    shape = (n, C, d, h, w)
    x = rnd(shape, case['sd'], 3.0)
    if not case['softmax']:
        x = torch.softmax(x, 1)                           # softmax=False: the module is handed probabilities
    if case['target'] == 'soft':
        tgt = torch.softmax(rnd(shape, case['sd'] + 1, 2.0), 1)
    else:
        tgt = labels_for(case['target'], (n, d, h, w), C, case['sd'], case['wide'])
    return dict(x=x, target=tgt, C=C, wt=case['wt'], no_bg=case['no_bg'] and C > 1, softmax=case['softmax'], soft=case['target'] == 'soft')


def ref_dice(inp, dtype, softmax=None):
    x = _leaf(inp['x'], dtype)
    t = inp['target'].to(dtype) if inp['soft'] else inp['target'].long()
    l = losses.dice_loss(x, t, inp['C'], inp['wt'], inp['no_bg'], inp['softmax'] if softmax is None else softmax, eps=1e-6)
    l.backward()
    return float(l.detach().double()), _f64(x.grad)


# ---- softmax ---------------------------------------------------------------------------------------------------------------------
# 'plain4': logits of scale 4.  'plain80': scale 80 on every odd voxel (saturated rows; exp() of the raw logits leaves fp32's range in the sum), scale 4 on
# the even ones -- a saturated row's backward is a difference of rounded probabilities, so the ordinary rows carry the norm the criteria divide by.
# 'offset': a per-voxel offset of up to +-100 under scale-4 logits (exp(100) overflows without the max subtraction, exp(-100) underflows).
SOFTMAX = st.fixed_dictionaries(dict(
    C=st.sampled_from(DICE_C), n=st.integers(1, 2), vol=st.tuples(st.integers(1, 5), st.integers(1, 7), st.integers(1, 19)),
    mode=st.sampled_from(['plain4', 'plain80', 'offset']), sd=st.integers(0, 999)))
SOFTMAX_PINNED = [dict(C=C, n=1 + i % 2, vol=_cyc([(3, 5, 7), (1, 2, 19), (4, 7, 9)], i), mode=_cyc(['plain4', 'plain80', 'offset'], i), sd=i)
                  for i, C in enumerate(DICE_C)]


def build_softmax(case):
    C, n, (d, h, w) = case['C'], case['n'], case['vol']
    shape = (n, C, d, h, w)
    x = rnd(shape, case['sd'], 4.0)
    if case['mode'] == 'plain80':
        odd = (torch.arange(n * d * h * w) % 2 == 1).reshape(n, 1, d, h, w)
        x = torch.where(odd, x * 20.0, x)
    elif case['mode'] == 'offset':
        x = x + rnd((n, 1, d, h, w), case['sd'] + 1, 100.0)
    if d * h * w > 1:                                      # one row with a single dominant logit
        x[0, :, -1, -1, -1] = -30.0
        x[0, case['sd'] % C, -1, -1, -1] = 30.0
    return dict(x=x, go=rnd(shape, case['sd'] + 2))


def ref_softmax(inp, dtype):
    x = _leaf(inp['x'], dtype)
    y = torch.softmax(x, 1)
    y.backward(inp['go'].to(dtype))
    return _f64(y), _f64(x.grad)


# ---- cross-entropy family --------------------------------------------------------------------------------------------------------
# xent.hip xe_lanes(C, pointers): quad kernels L = C / 4 in {1, 2, 4, 8, 16}; thread-per-voxel form for every other C <= 64 and for a pointer
# that is not 16-byte aligned; C > 64 refused
XENT_C = [1, 2, 3, 4, 5, 8, 12, 16, 32, 33, 64]
XENT_LANES = {1: 0, 2: 0, 3: 0, 4: 1, 5: 0, 8: 2, 12: 0, 16: 4, 32: 8, 33: 0, 64: 16}
XENT = st.fixed_dictionaries(dict(
    C=st.sampled_from(XENT_C), mode=st.sampled_from(['ce', 'focal', 'soft']), form=st.sampled_from(['5d', '5d', '2d', '2d_misaligned']),
    n=st.integers(1, 2), vol=st.tuples(st.integers(1, 5), st.integers(1, 7), st.integers(1, 19)), mean=st.booleans(),
    ignore=st.sampled_from(['default', 'hit', 'miss']), alpha=st.booleans(), gamma=st.sampled_from([0.0, 1.5, 2.0]), softmax=st.booleans(),
    wide=st.booleans(), sd=st.integers(0, 999)))
# one explicit example per class count and mode (every quad kernel L = 1 ... 16 and the thread-per-voxel form), and the quad class counts again
# from a logits pointer 4 bytes off a 16-byte boundary (xe_lanes then falls back to the thread-per-voxel form)
XENT_PINNED = [dict(C=C, mode=mode, form=_cyc(['5d', '2d'], i + j), n=1 + (i + j) % 2, vol=_cyc([(3, 5, 7), (1, 2, 19), (4, 7, 9)], i + j), mean=(i + j) % 3 != 0,
                    ignore=_cyc(['default', 'hit', 'miss'], i), alpha=i % 2 == 0, gamma=_cyc([0.0, 1.5, 2.0], i), softmax=(i + j) % 2 == 0, wide=i % 2 == 1, sd=i)
               for i, C in enumerate(XENT_C) for j, mode in enumerate(['ce', 'focal', 'soft'])]
XENT_PINNED += [dict(C=C, mode=mode, form='2d_misaligned', n=2, vol=(3, 5, 7), mean=True, ignore='hit', alpha=True, gamma=2.0, softmax=True, wide=False, sd=C)
                for C, mode in ((4, 'ce'), (8, 'focal'), (16, 'soft'), (32, 'ce'), (64, 'focal'))]


def build_xent(case):
    C, n, (d, h, w) = case['C'], case['n'], case['vol']
    shape = (n, C, d, h, w)
    x = rnd(shape, case['sd'], 3.0)
    out = dict(C=C, mode=case['mode'], form=case['form'], mean=case['mean'], softmax=case['softmax'], gamma=case['gamma'], alpha=None, ignore=-100)
    if case['mode'] != 'ce' and not case['softmax']:
        x = torch.softmax(x, 1)                           # focal soft_max=False / soft CE softmax=False are handed probabilities ...
        if case['mode'] == 'soft':
            x = x.clamp(min=1e-8)                         # ... clamped, for soft CE (min p here is e^-6 / 64: the clamp never binds)
    lab = labels_for('iid', (n, d, h, w), C, case['sd'], case['wide'])
    tgt = torch.softmax(rnd(shape, case['sd'] + 1, 2.0), 1)
    if case['mode'] == 'ce':
        first = int(lab.reshape(-1)[0])
        if case['ignore'] == 'hit' and bool((lab != first).any()):
            out['ignore'] = first                         # an ignore_index that occurs (and leaves voxels to average over)
        elif case['ignore'] != 'default':
            out['ignore'] = C + 1                         # one that does not occur
    if case['mode'] == 'focal' and case['alpha']:
        out['alpha'] = rnd((C, 1), case['sd'] + 3, 0.375) + 0.625       # in [0.25, 1]
    if case['form'] != '5d':                              # the M x C form
        x = x.movedim(1, -1).reshape(-1, C).contiguous()
        tgt = tgt.movedim(1, -1).reshape(-1, C).contiguous()
        lab = lab.reshape(-1)
    out.update(x=x, labels=lab, soft_target=tgt)
    return out


def ref_xent(inp, dtype):
    x = _leaf(inp['x'], dtype)
    if inp['mode'] == 'ce':
        l = losses.cross_entropy_loss(x, inp['labels'].long(), ignore_index=inp['ignore'], reduction='mean' if inp['mean'] else 'sum')
    elif inp['mode'] == 'focal':
        l = losses.focal_loss(x, inp['labels'].long(), inp['C'], alpha=inp['alpha'], gamma=inp['gamma'], size_average=inp['mean'], soft_max=inp['softmax'])
    else:
        l = losses.soft_cross_entropy_loss(x, inp['soft_target'].to(dtype), softmax=inp['softmax'])
    l.backward()
    return float(l.detach().double()), _f64(x.grad)


# ---- NCC -------------------------------------------------------------------------------------------------------------------------
# losses.hip da_ncc_fwd.  ncc_partial_kernel<true>: x, y 16-byte aligned and (N = 1 or V % 4 == 0) -> float4 body from element 0 + scalar tail.
# ncc_partial_kernel<false>: any other layout -> per sample a scalar head of 0 - 3 elements to the next 16-byte boundary, float4 body, scalar tail; a
# sample whose x and y have no common float4 phase, or that ends before the boundary (V < head), goes through the scalar loop alone.
# Grid: nblocks = min(ceil((V / 4 + 1) / 1024), kBlocks = 512) blocks of 256 threads per sample, so a thread runs about 4 float4 iterations until the cap is
# reached at V = 2.1 M, and the flush of the fp32 partials into double (every 16 float4 iterations; every 64 scalar ones) is first executed at
# V >= 16 x 4 x 256 x 512 = 8 388 608 voxels per sample (64 x 256 x 512, the same number, for an all-scalar sample).  Below that it never runs: only the
# 208^3 and 207 x 209 x 211 cases of NCC_PINNED cover it.
# V = 1 is degenerate (0 / 0) and V = 2 has |ncc| = 1 with a zero gradient: asserted once in the device file, not drawn.
# 'off' (explicit cases only, flat form): x and y start that many floats past a 16-byte boundary (views into a larger buffer, which ops.NCCFn keeps uncopied).
_ncc_vol = st.one_of(st.tuples(st.integers(1, 5), st.integers(1, 7), st.integers(3, 35)),
                     st.sampled_from([(1, 1, 3), (1, 1, 5), (1, 1, 6), (1, 1, 7), (16, 32, 32), (1, 127, 129), (2, 91, 90), (3, 43, 127), (1, 5, 3277), (7, 49, 48)]))
NCC = st.fixed_dictionaries(dict(
    n=st.integers(1, 4), vol=_ncc_vol, offset=st.sampled_from([0.0, 5.0]), slope=st.sampled_from([0.7, -1.3]), grads=st.sampled_from(['x', 'y', 'xy']),
    flat=st.booleans(), sd=st.integers(0, 999)))
NCC_BIG = [dict(n=2, vol=(131, 127, 129), offset=5.0, slope=0.7, grads='xy', flat=False, sd=11),       # V = 2146173 (odd): capped grid, head + body + tail
           dict(n=1, vol=(131, 127, 129), offset=5.0, slope=-1.3, grads='x', flat=True, sd=12)]        # the aligned form at the cap, with a tail
NCC_PINNED = [
    # the example that showed the raw-product sums 8.8e-6 (loss) / 3.0e-5 (gradient) from float64 before the kernel summed about a pivot
    dict(n=1, vol=(1, 1, 6), offset=5.0, slope=0.7, grads='xy', flat=True, sd=881),
    # V < 4 (tail only; with N = 3 every later sample is a head only)
    dict(n=1, vol=(1, 1, 3), offset=5.0, slope=-1.3, grads='xy', flat=True, sd=1),
    dict(n=3, vol=(1, 1, 3), offset=0.0, slope=0.7, grads='x', flat=False, sd=2),
    # N > 1 with V % 4 = 1, 2, 3 (heads of 3 / 2 / 1 elements on the later samples) and 0 (aligned form with a batch)
    dict(n=2, vol=(3, 5, 7), offset=5.0, slope=0.7, grads='xy', flat=False, sd=3),
    dict(n=3, vol=(2, 7, 9), offset=0.0, slope=-1.3, grads='y', flat=True, sd=4),
    dict(n=4, vol=(1, 9, 11), offset=5.0, slope=0.7, grads='x', flat=False, sd=5),
    dict(n=2, vol=(4, 5, 6), offset=5.0, slope=-1.3, grads='xy', flat=True, sd=6),
    # misaligned bases: N = 1 with both tensors 4 / 8 / 12 bytes off (head 3 / 2 / 1), a batch on top of an offset, and no common phase (all scalar)
    dict(n=1, vol=(3, 5, 7), offset=5.0, slope=0.7, grads='xy', flat=True, sd=7, off=(1, 1)),
    dict(n=1, vol=(4, 5, 6), offset=0.0, slope=-1.3, grads='x', flat=True, sd=8, off=(2, 2)),
    dict(n=1, vol=(1, 9, 11), offset=5.0, slope=0.7, grads='y', flat=True, sd=9, off=(3, 3)),
    dict(n=3, vol=(1, 9, 11), offset=5.0, slope=-1.3, grads='xy', flat=True, sd=10, off=(2, 2)),
    dict(n=1, vol=(3, 5, 7), offset=5.0, slope=0.7, grads='xy', flat=True, sd=13, off=(1, 0)),
    dict(n=2, vol=(4, 5, 6), offset=0.0, slope=-1.3, grads='xy', flat=True, sd=14, off=(0, 3)),
] + NCC_BIG + [
    # the double flush: the aligned body, the all-scalar loop, and the head / body / tail form's body, each above 8 388 608 voxels per sample
    dict(n=1, vol=(208, 208, 208), offset=5.0, slope=0.7, grads='x', flat=True, sd=15),
    dict(n=1, vol=(208, 208, 208), offset=5.0, slope=-1.3, grads='y', flat=True, sd=16, off=(1, 0)),
    dict(n=2, vol=(207, 209, 211), offset=5.0, slope=0.7, grads='x', flat=False, sd=17),
]


def build_ncc(case):
    n, (d, h, w) = case['n'], case['vol']
    shape = (n, d * h * w) if case['flat'] else (n, 1, d, h, w)
    x = (rnd(shape, case['sd']) + 1) * 1.5 + case['offset']                        # variance 0.75, mean `offset` + 1.5
    y = case['slope'] * x + rnd(shape, case['sd'] + 1, 1.5)                        # |ncc| about 0.57 / 0.79
    if case.get('first_zero'):                                                     # a first voxel far from the intensity range (the kernel's pivot)
        x.reshape(n, -1)[:, 0] = 0.0
        y.reshape(n, -1)[:, 0] = 0.0
    return dict(x=x, y=y, grads=case['grads'], off=case.get('off', (0, 0)))


def ref_ncc(inp, dtype):
    x = _leaf(inp['x'], dtype, 'x' in inp['grads'])
    y = _leaf(inp['y'], dtype, 'y' in inp['grads'])
    l = losses.ncc_loss(x, y)
    l.backward()
    return float(l.detach().double()), (_f64(x.grad) if x.grad is not None else None), (_f64(y.grad) if y.grad is not None else None)


# ---- bending energy and gradient loss ---------------------------------------------------------------------------------------------
SPACINGS = [(1.0, 1.0, 1.0), (2.0, 2.0, 2.0), (1.0, 2.0, 1.5)]
REG = st.fixed_dictionaries(dict(
    n=st.integers(1, 3), d=st.integers(3, 8), h=st.integers(3, 10), w=st.integers(3, 19), thin=st.sampled_from([None, None, 0, 1, 2]),
    norm=st.sampled_from(['L1', 'L2']), spacing=st.sampled_from(SPACINGS), normalize=st.booleans(), sd=st.integers(0, 999)))
# 'L1' / 'L2' x the three spacings x normalize, the axis that is exactly 3 cycling through D, H, W and none
REG_PINNED = [dict(n=1 + i % 3, d=4 + i % 4, h=5 + i % 5, w=6 + i % 11, thin=_cyc([0, 1, 2, None], i), norm=norm, spacing=sp, normalize=nz, sd=i)
              for i, (norm, sp, nz) in enumerate((a, b, c) for a in ('L1', 'L2') for b in SPACINGS for c in (False, True))]


def build_reg(case):
    dims = [case['d'], case['h'], case['w']]
    if case['thin'] is not None:
        dims[case['thin']] = 3                            # exactly the stencil's minimum on one axis
    # a continuous distribution: no difference is exactly zero, so 'L1' never sits on its kink (the sub-gradient there is a convention)
    return dict(u=rnd((case['n'], 3) + tuple(dims), case['sd'], 2.0), norm=case['norm'], spacing=case['spacing'], normalize=case['normalize'])


def ref_bending(inp, dtype):
    u = _leaf(inp['u'], dtype)
    l = losses.bending_energy_loss(u, inp['spacing'], inp['normalize'], inp['norm'])
    l.backward()
    return float(l.detach().double()), _f64(u.grad)


def ref_gradloss(inp, dtype):
    u = _leaf(inp['u'], dtype)
    l = losses.gradient_loss(u, inp['norm'], inp['spacing'], inp['normalize'])
    l.backward()
    return float(l.detach().double()), _f64(u.grad)


# ---- LNCC ------------------------------------------------------------------------------------------------------------------------
# reglosses.hip lncc_march_ok: dilation 1, stride 1 and F in {5, 9} take the z-marching kernels, everything else the separable passes
LNCC = st.fixed_dictionaries(dict(
    F=st.sampled_from([3, 5, 7, 9]), n=st.integers(1, 2), ed=st.integers(0, 6), eh=st.integers(0, 9), ew=st.integers(0, 25),
    grads=st.sampled_from(['I', 'J', 'IJ']), sd=st.integers(0, 999)))
# LNCCLoss at a smallest side ms <= 24: one scale, window ms // 2, dilation 1, stride max((k + 1) // 4, 1) (2 or 3 from ms = 14 on); ms = 10 gives window 5
# at stride 1, the marching form with LNCCLoss's eps
LNCC_MS = st.fixed_dictionaries(dict(
    ms=st.sampled_from([6, 9, 10, 12, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24]), axis=st.integers(0, 2), e1=st.integers(0, 6), e2=st.integers(0, 8),
    n=st.integers(1, 2), grads=st.sampled_from(['I', 'J', 'IJ']), sd=st.integers(0, 999)))
LNCC_MS_PINNED = [dict(ms=ms, axis=i % 3, e1=_cyc([0, 3, 6], i), e2=_cyc([5, 0, 8], i), n=1 + i % 2, grads=_cyc(['IJ', 'I', 'J'], i), sd=i)
                  for i, ms in enumerate([6, 10, 14, 16, 19, 23, 24])]      # window 3 (stride 1), 5 (marching), 7 / 8 / 9 (stride 2), 11 / 12 (stride 3)


def lncc_class(case):
    if 'F' in case:
        return 'march F=%d' % case['F'] if case['F'] in (5, 9) else 'separable F=%d' % case['F']
    k = case['ms'] // 2
    s = max((k + 1) // 4, 1)
    return 'multi-scale strided' if s > 1 else ('multi-scale march' if k == 5 else 'multi-scale stride 1')


def build_lncc(case):
    if 'F' in case:
        dims = (case['F'] + case['ed'], case['F'] + case['eh'], case['F'] + case['ew'])        # from exactly the window span upward
    else:
        dims = [case['ms'] + case['e1'], case['ms'] + case['e2']]
        dims.insert(case['axis'], case['ms'])
    shape = (case['n'], 1) + tuple(dims)
    # two images in [0, 1] that are correlated (J = 0.6 I + 0.4 noise): the window cross term, which the loss squares, stays well away from zero --
    # between independent images it is a sum that cancels to noise, and with the few windows of a volume near the span the gradient is that noise
    I = rnd(shape, case['sd']) * 0.5 + 0.5
    return dict(I=I, J=0.6 * I + 0.4 * (rnd(shape, case['sd'] + 1) * 0.5 + 0.5), F=case.get('F'), grads=case['grads'])


def ref_lncc(inp, dtype):
    I = _leaf(inp['I'], dtype, 'I' in inp['grads'])
    J = _leaf(inp['J'], dtype, 'J' in inp['grads'])
    l = losses.lncc_loss(I, J, inp['F']) if inp['F'] else losses.lncc_multiscale_loss(I, J)
    l.backward()
    return float(l.detach().double()), (_f64(I.grad) if I.grad is not None else None), (_f64(J.grad) if J.grad is not None else None)


def lncc_eref(inp, r64):
    """The fp32 CPU oracle's distance from float64 on this example: (loss, worst gradient)."""
    r32 = ref_lncc(inp, torch.float32)
    return scalar_err(r32[0], r64[0], 'rel1'), max(dist(a, b) for a, b in zip(r32[1:], r64[1:]) if b is not None)


# ---- label kernels (integer: numpy is the reference) ------------------------------------------------------------------------------
_lab_vol = st.tuples(st.integers(1, 5), st.integers(1, 7), st.integers(1, 19))
ONE_HOT = st.fixed_dictionaries(dict(C=st.sampled_from([1, 2, 5, 32, 200, 256]), n=st.integers(1, 2), vol=_lab_vol, wide=st.booleans(), sd=st.integers(0, 999)))
ARGMAX = st.fixed_dictionaries(dict(C=st.sampled_from(DICE_C), n=st.integers(1, 2), vol=_lab_vol, wide=st.booleans(), levels=st.sampled_from([1, 2, 4]),
                                    sd=st.integers(0, 999)))
OVERLAP = st.fixed_dictionaries(dict(C=st.sampled_from([1, 2, 5, 32, 200, 255, 256, 1024]), n=st.integers(1, 3),
                                     V=st.one_of(st.integers(1, 3000), st.sampled_from([15, 16, 17, 16005])), pw=st.booleans(), tw=st.booleans(),
                                     runs=st.booleans(), sd=st.integers(0, 999)))
ONE_HOT_PINNED = [dict(C=C, n=1 + i % 2, vol=_cyc([(3, 5, 7), (1, 2, 19), (4, 7, 9)], i), wide=i % 2 == 0, sd=i) for i, C in enumerate([1, 2, 5, 32, 200, 256, 256])]
# the four label-width combinations at C = 1024 (labels outside [0, C) on the int64 side), and at C = 255 / 256 where uint8 can / cannot hold one
OVERLAP_PINNED = [dict(C=C, n=1 + i % 3, V=_cyc([16005, 17, 2999, 1000], i), pw=pw, tw=tw, runs=i % 2 == 0, sd=i)
                  for i, (C, pw, tw) in enumerate((C, pw, tw) for C in (1024, 255, 256) for pw in (False, True) for tw in (False, True))]
ARGMAX_PINNED = [dict(C=C, n=1 + i % 2, vol=_cyc([(3, 5, 7), (1, 2, 19), (4, 7, 9)], i), wide=i % 2 == 0, levels=_cyc([2, 4, 1], i), sd=i) for i, C in enumerate(DICE_C)]
LNCC_PINNED = [dict(F=F, n=1 + i % 2, ed=e[0], eh=e[1], ew=e[2], grads=_cyc(['IJ', 'I', 'J'], i), sd=i)
               for i, (F, e) in enumerate((F, e) for F in (3, 5, 7, 9) for e in ((0, 0, 0), (3, 8, 25)))]      # exactly the window span, and partial tiles


def build_one_hot(case):
    n, (d, h, w) = case['n'], case['vol']
    return labels_for('iid', (n, d, h, w), case['C'], case['sd'], case['wide']).reshape(n, 1, d, h, w)


def ref_one_hot(mask, C):
    m = mask.numpy().astype(np.int64)[:, 0]
    return np.moveaxis((m[..., None] == np.arange(C)).astype(np.float32), -1, 1)


def build_argmax(case):
    """Logits on `levels` integer values: exact ties in (nearly) every voxel, the first maximum has to win."""
    n, C, (d, h, w) = case['n'], case['C'], case['vol']
    g = torch.Generator().manual_seed(case['sd'])
    logits = torch.randint(0, case['levels'], (n, C, d, h, w), generator=g).float()
    return logits, labels_for('iid', (n, d, h, w), C, case['sd'], case['wide'])


def ref_counts(p, t, C):
    """counts[n][c] = (|p == c|, |t == c|, |p == c and t == c|) over labels inside [0, C); p, t: (n, V) integer arrays."""
    out = np.zeros((p.shape[0], C, 3), dtype=np.int64)
    for n in range(p.shape[0]):
        a, b = p[n], t[n]
        ina, inb = (a >= 0) & (a < C), (b >= 0) & (b < C)
        out[n, :, 0] = np.bincount(a[ina], minlength=C)
        out[n, :, 1] = np.bincount(b[inb], minlength=C)
        out[n, :, 2] = np.bincount(a[ina & (a == b)], minlength=C)
    return out


def ref_argmax(logits, truth):
    n, C = logits.shape[0], logits.shape[1]
    pred = np.argmax(logits.numpy(), axis=1)                                      # numpy: the first maximum, as torch.max
    return ref_counts(pred.reshape(n, -1).astype(np.int64), truth.numpy().reshape(n, -1).astype(np.int64), C), pred


def build_overlap(case):
    """Two label maps with values outside [0, C) present wherever the label width can hold one (negative ones too for int64)."""
    g = torch.Generator().manual_seed(case['sd'])
    C, shape = case['C'], (case['n'], case['V'])

    def one(wide):
        lo, hi = (-3, C + 20) if wide else (0, min(C + 20, 256))
        lab = torch.randint(lo, hi, shape, generator=g)
        if case['runs']:                                   # long runs of one pair (merged in registers by the kernel)
            lab[:, case['V'] // 4: case['V'] // 2] = C // 2
        return lab if wide else lab.to(torch.uint8)
    return one(case['pw']), one(case['tw'])
