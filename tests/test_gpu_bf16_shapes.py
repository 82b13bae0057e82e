"""Randomised float64 parity for the bf16 activation-storage twins that had no test of their own: the seven `_bf16` entries of norm_act.hip, the six of pool.hip, the two of
headdice.hip and the six masked 3x3x3 convolution twins of conv3d.hip, entry by entry through the C ABI and ops.call_act.  (The nine of deconv.hip are family 4 of
tests/test_gpu_pointwise_shapes.py; whole networks are tests/test_gpu_bf16_storage.py.)

Inputs are drawn in fp32, rounded to bf16 and handed over as bf16; the float64 reference takes the widened values.  Conv weights are bf16-representable, so the operand
rounding of the bf16 matrix mode is a no-op (one pinned matrix and one pinned stride-2 example use unrounded weights, their reference rounds them to nearest even).
Where an entry applies a deferred BatchNorm + activation to a matrix operand, the tensor da_bn_act_fwd_bf16 stores is held to float64 and then is the reference's
input.  Kinks decided on a recomputed z take block_cases' guard band (caps 0.1 % and 64; the oracle of the CPU file entered it at 16 elements of a tensor at most); decisions on a given bf16 tensor
(act_bwd on y, the pool's arg-max) are exact.  Every output buffer is prefilled with NaN.  Cases, builders, references, the restated launcher decisions and the bounds
are in tests/bf16_cases.py; tests/test_bf16_reference.py runs the same examples through an fp32 torch-CPU oracle that rounds where the product stores.

Bounds.  fp32 results: the tolerance of the quantity's fp32 family.  Stored bf16 tensors: |got - ref| <= 2^-8 |ref| + tol max|ref| (pointwise_cases.bf16_close), and,
wherever the reference is farther than tol max|ref| from a rounding midpoint, got == round-to-nearest-even(ref) exactly (bf16_cases.rne_check; at most 20 % of a tensor
may be left out: the worst was 12.5 %, the act of da_maxpool2_fwd_pro and the stride-2 dx; the exact zeros a ReLU leaves are always among them).  Bit equality: da_maxpool2_fwd / _bwd / _bwd_add (against (gskip.float() + routed.float()).bfloat16()),
da_upsample_nearest_fwd, da_act_bwd and da_act_bwd_add wherever the factor is 1 or 0 -- a sum of two bf16 values very often IS a rounding midpoint, so ties-to-even is
asserted there bit for bit.  The train-mode BatchNorm backward is a difference of terms of size scale dz (zero in exact arithmetic at M = 1): below 128 rows the absolute
part of its bounds is in units of max(max|ref|, max|scale dz|), from 128 rows on the plain formula holds.

Launcher branch <- value
  family `stream` (norm_act.hip; bf16_cases.plan_rows restates plan_rows): every entry on every example, slopes -1 / 0 / 0.01
      fixed channel quad, dxsum fused into the apply pass <- C = 8, 16, 32, 64;  no fixed quad, stand-alone column sum over the stored dx <- C = 12, 24, 48;
      VEC == 1, single 2-byte stores <- C = 3, 5, 6 (pinned only; the product never sends them, the C ABI exports them)
      rows <- M = 1; rpi 16 - 1 and + 1 (one workgroup / two); 2 rpi + 1 and rpi + 3 (the two-rows-in-flight loop of the backward sums clamps its second row)
      the 1024-workgroup cap <- C = 64, M = 262 221: 257 rows per workgroup, workgroups 1021 ... 1023 start past M (a workgroup that starts at or past M exists ONLY
      when the cap binds: below it rows_per_block <= rpi 16, test_bf16_reference.py proves it), four grid strides of bn_act_fwd (4096 x 256 quads each), sixteen of the fused backward
      (1024 x 256 quads, two in flight)
      bn_act_fwd above one grid stride with a quad that changes per iteration <- C = 12, M = 349 537;  act_bwd <- numel = 1, 3, 4 ... 7, 1021 ... 1024, one above a grid stride
      da_bn_act_bwd_dbias train 1 / 0 x dxsum given / null (the same dx, dgamma, dbeta bit for bit); da_act_bwd_add_dbias g2 given / null (null: da_act_bwd's bits), y null
      at slope -1, dbias given / null; da_act_bwd_add_partial + da_colsum_finish (*nparts = the grid, accumulate 0 / 1)
  family `pool` (pool.hip): D, H, W 2 ... 7 in all eight parity combinations (memset / memcpy of the trailing planes sized by the element), C = 4, 8, 12, 32 and pinned 3, 5,
      N 1 ... 2; inputs on a grid of 0.5 (37.7 % of the windows hold a tied maximum; torch-CPU's float64 max_pool3d backward is checked to route to the first maximum in
      (d, h, w) order on the same inputs); da_maxpool2_fwd_pro on even sizes with a negative scale channel (its maximum is bit-equal to the pool of its own stored act),
      declines odd sizes, C % 4 != 0 and slope >= 1 with both outputs untouched; nearest up-sampling by 2 and to (d + 3, 2 h - 1, w)
  family `head` (headdice.hip): (Cin, C) in {16, 64} x {16, 32}, V = 1, 105, 256, 257, 512, 693, 1025, N 1 ... 3, uint8 / int64 labels, prologue none / ReLU / LeakyReLU;
      other channel counts decline with every output untouched
  family `conv3` (conv3d.hip, bf16 matrix mode; shapes below / exactly / one past the 4 x 8 x 16 tile in every axis, N = 2; bf16_cases.c3_route restates the three launchers,
      every pinned example carries its routes written by hand): each entry through the C ABI with the hand-written mask, through ops.call_act (the same bits, no conversion
      pass; one pass where the twin declines) and through the forced conversion route
      all-bf16 matrix route <- (16, 0), (32, 16), (16, 16), (64, 32), (8, 0), (8, 16), (24, 0) x Cout 8, 16, 32, 12: fwd at three slopes, fwd_bnstats (partials against the
      float64 sums of the UNROUNDED result, *stats_nparts by the tile count), fwd_pro with the prologue on in1 / on both / with statistics, wgrad_pro, dgrad with a split
      output, wgrad (a given dbias declines).  The data gradient declines at Cout = 12 (pick_ck(12, 0) = 0) and for the split (8, 16) (first part not a multiple of 16)
      thin VALU fp32 -> bf16 <- (1, 0), (1, 1) -> 8, 12, 16 (Cout = 4 declines); its bf16 dy -> fp32 dx <- Cout 8, 16; few-Cin weight gradient (fp32 inputs, bf16 dy) <- Cout 4 ... 16
      thin bf16 -> fp32 <- (8, 16), (16, 16), (16, 0), (16, 8) -> 1 ... 3; fp32 dy -> bf16 dx1, dx2 <- also (4, 12), (12, 0); flow weight gradient (bf16 inputs, fp32 dy) <- all
      seven, (4, 0) included; stride 2 with act_bf16 <- C1 16, 32 x Cout 8 ... 64 at odd D, H, W (its data gradient declines at Cout = 8); *stats_nparts = 0 on both
      declines (test_conv3_declines): all seven partial masks with two inputs, every mask but the two complete ones with one; one bf16 and one fp32 input on a thin
      shape; stride 2 at C1 = 8, 48 and Cout = 6; the complete mask in matrix modes 'fp32' and 'fp32_split' -- always DA_ERR_UNSUPPORTED, *stats_nparts = 0, outputs untouched

The two dxsum routes sum DIFFERENT tensors, as read from bn_act_bwd_impl: the fused route (bn_act_bwd_apply_kernel's colacc) sums the fp32 dx BEFORE the store, the
stand-alone route (colsum_t<da_bf16>) the STORED bf16 dx.  Each is asserted against the float64 sum of what it sums; the two float64 sums differ by up to 3.6e-3 of
sum |scale dz| on these examples (the rounding errors of the stored tensor do not cancel).  The rounding oracle of tests/test_gpu_bf16_storage.py sums the stored tensor and
states that the device's pre-store sum is the more accurate of the two; neither route contradicts it at its 5e-3, so no kernel is changed.  da_act_bwd_add_dbias sums
before the store as well.

Worst case over all examples on an MI355X (from the DA_BF16_SHAPES_REPORT of that run), the fp32 CPU oracle's worst case on the same examples, the ceiling and what is
asserted (rule: max(4 x device, 8 x oracle) rounded up to two digits where that is more than 10 x below the ceiling, else the ceiling).  fp32 quantities: distance from
float64 (sums: largest per-channel error / sum |term|).  Stored tensors: "tol needed", the smallest tol at which both checks hold, never asserted below 8 x 2^-24 = 4.8e-7.
  family / quantity                          device worst   fp32 oracle worst   ceiling   asserted
  stream  mean | rstd | scale | shift           1.3e-7         2.3e-7            4.8e-7    4.8e-7   (stays)
  stream  running statistics                    1.3e-7         2.4e-7            4.8e-7    4.8e-7   (stays)
  stream  d_gamma / d_beta                      2.0e-7 / 6.7e-8   2.7e-7 / 2.1e-7   9.9e-6 / 5.8e-6   9.9e-6 / 5.8e-6   (8 x oracle = 2.2e-6 / 1.7e-6: stay)
  stream  colsum, dbias, dxsum fused / alone    5.8e-8, 6.0e-8, 5.2e-8 / 1.4e-8   1.1e-7   1e-6   1e-6   (8.4e-7: stays)
  stream  y (stored)                            0              1.7e-8            2e-5      4.8e-7
  stream  dx train / eval (stored)              5.0e-8 / 0     3.4e-8 / 0        7.2e-6    4.8e-7
  stream  act_bwd, act_bwd_add dx (stored)      0              0                 4.8e-7    4.8e-7   (derived: one or two fp32 operations on bf16 operands)
  pool    act of fwd_pro (stored)               0              0                 4.8e-7    4.8e-7   (derived)
  pool    nearest up-sampling dx (stored)       0              0                 1e-6      1e-6     (stays)
  head    loss                                  3.9e-8         3.0e-8            1e-4      2.4e-7
  head    coef                                  3.4e-7         3.2e-7            1e-4      2.6e-6
  head    dW / db                               7.6e-7 / 6.2e-7   5.5e-7 / 5.3e-7   1e-4   4.4e-6 / 4.3e-6
  head    dx (stored)                           5.5e-8         4.6e-8            1e-4      4.8e-7
  conv3   matrix y (stored)                     1.3e-7         7.0e-8            9.1e-6    5.6e-7
  conv3   matrix dx (stored)                    4.0e-8         1.1e-7            6.3e-6    6.3e-6   (8.5e-7: stays)
  conv3   matrix dW (plain / prologue)          1.6e-7 / 2.1e-7   6.9e-7 / 6.8e-7   5.6e-6   5.6e-6   (5.5e-6: stays)
  conv3   sum y / sum y^2                       6.4e-8 / 1.2e-7   8.0e-8           1e-6      1e-6     (stays)
  conv3   thin, few-Cin, flow, stride 2         5.8e-7 (flow y), 3.7e-7 (first dx), dW 1.3e-7 ... 2.1e-7; stored 4.5e-8   4.5e-7   1e-5   1e-5   (3.6e-6: stays)
The stored tensors sit at 0.985 ... 0.996 of their one-spacing bound, as round-to-nearest must.

Twin against the conversion route (ops.BF16_FORCE_BRIDGE, same arguments; every entry of the file, the two prologue entries of conv3d.hip included).  Bit-equal and asserted:
every stored tensor and every fp32 result of families `stream` and `pool` -- except, by construction, the stand-alone dxsum, which on the conversion route sums the still
unrounded fp32 dx and is held to the float64 sum of the unrounded dx there (5.1e-8 of sum |term|).  Matrix-core entries, measured, both sides asserted against float64 only:
head (no prologue) loss, dx, dW 0 elements differ; behind a prologue the conversion route keeps the head's activation in fp32 and is held to the reference on the unrounded
activation.  conv3 y (fwd, fwd_bnstats, fwd_pro) and dx of every route: 0 elements differ, and the partial sums of the conversion route meet the same 1e-6 (6.4e-8 / 1.2e-7;
behind a prologue 4.9e-8 / 8.9e-8).  conv3 dW differs in 68 % (few-Cin), 71 % (flow), 70 % (matrix route) and 75 % (wgrad_pro) of its elements by at most 1.2e-7, 1.2e-7,
2.0e-7 and 2.1e-7 of max|dW| (the fp32 entry takes another kernel variant), stride-2 dW 0.  The fp32 prologue entries of conv3d.hip round their activated operand to bf16
when they stage it, as the bf16 matrix mode does with every operand: that operand is the tensor da_bn_act_fwd_bf16 stores, so the conversion route of fwd_pro / wgrad_pro is
held to the same float64 reference as the twin (dW 2.1e-7).  The prologue entries on the raw tensors and the plain entries on the stored activated tensors: 0 elements of y
and dW differ.

No defect found in the kernels.  Two routes worth knowing: the all-bf16 data gradient declines for Cout = 12 and for a split (8, 16), and ops.call_act converts there;
the first layers' data gradient (bf16 dy -> fp32 dx) has a native thin route.

Scratch mutants (one change each, built outside the tree and loaded through DA_LIB; every address stays inside its tensor; each run once):
  (a) da_pack_bf16x2 truncates                       test_stream_random_shapes y 1.075 of the bound; test_act_bwd_sizes 1.273; test_head_random_shapes act 1.875;
                                                     test_pool_random_shapes dx add: 6 of 192 elements differ in their bits
  (b) `>=` for `>` in maxpool2_bwd_kernel's arg-max  test_pool_random_shapes dx: 28 of 192 elements differ (every pinned example)
  (c) act_bwd_kernel without its scalar tail         test_act_bwd_sizes numel = 1 (the NaN prefill stays); test_stream_random_shapes C = 3 at M = 1 and M = 1359
  (d) the odd-size memset / memcpy of half the bytes test_pool_random_shapes 3 x 2 x 2 (C = 8) and 5 x 7 x 2 (C = 3): non-finite dx
  (e) bits 1 and 2 of ops.call_act's mask exchanged  family conv3 on all 14 pinned one-input examples of the matrix and stride-2 kinds (the twin declines, a conversion pass is
                                                     counted where none may be); the 11 two-input examples pass, as they must (mask 7 is its own image).  Not run on the thin
                                                     kinds: there the wrong mask names another element size
"""
import ctypes

import pytest
import torch

import bf16_cases as bx
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float('nan')


def _bf(t):
    """a CPU tensor of bf16-representable values -> the device, as bf16"""
    d = t.to(dev()).to(BF)
    return d


def _nan(shape, dtype=torch.float32):
    """an output buffer prefilled with NaN: an element the kernel does not write fails the finiteness assertion of every comparison"""
    return torch.full(tuple(shape), NAN, device=dev()).to(dtype)


def _cpu(t):
    return t.detach().float().cpu() if t.dtype == BF else t.detach().cpu()


class _Route(object):
    """ops.call_act on the twin (bridge=False: ops.bridged_calls must not move) or through the conversion route (ops.BF16_FORCE_BRIDGE: it must count)"""

    def __init__(self, bridge):
        self.bridge = bridge

    def __call__(self, name, *args):
        from deepatlas_amd import ops
        prev, before = ops.BF16_FORCE_BRIDGE, ops.bridged_calls.get(name, 0)
        ops.BF16_FORCE_BRIDGE = self.bridge
        try:
            ops.call_act(name, *args)
        finally:
            ops.BF16_FORCE_BRIDGE = prev
        assert ops.bridged_calls.get(name, 0) - before == int(self.bridge), (name, self.bridge)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF else torch.int32), b.contiguous().view(torch.int16 if b.dtype == BF else torch.int32))


# ---- family `stream` -----------------------------------------------------------------------------------------------------------------
def _run_stream(inp, bridge):
    from deepatlas_amd import _native as nat
    from deepatlas_amd.ops import A, O
    ptr, st, call = nat.ptr, nat.stream(), _Route(bridge)
    M, C, slope = inp['M'], inp['C'], inp['slope']
    x, dy, g2, y = (_bf(inp[k]) for k in ('x', 'dy', 'g2', 'y'))
    gamma, beta, rm, rv = (inp[k].clone().to(dev()) for k in ('gamma', 'beta', 'rm', 'rv'))
    mu, rs, sc, sf = (t.contiguous() for t in inp['stats'].to(dev()))
    wp, wn = nat.workspace.get(nat.lib().da_bn_ws_bytes(M, C), dev())
    o = {}
    o['stats'] = _nan((4, C))
    call('da_bn_train_stats', A(x), M, C, ptr(gamma), ptr(beta), bx.EPS, bx.MOMENTUM, ptr(rm), ptr(rv), *[ptr(o['stats'][i]) for i in range(4)], wp, wn, st)
    o['rm'], o['rv'] = rm, rv
    o['y'] = _nan((M, C), BF)
    call('da_bn_act_fwd', A(x), ptr(sc), ptr(sf), slope, O(o['y']), M, C, st)
    for train in (1, 0):
        for with_sum in (True, False):
            k = ('train' if train else 'eval') + ('' if with_sum else '_nosum')
            o['dx_' + k], o['dgamma_' + k], o['dbeta_' + k] = _nan((M, C), BF), _nan((C,)), _nan((C,))
            o['dxsum_' + k] = _nan((C,)) if with_sum else None
            call('da_bn_act_bwd_dbias', A(dy), A(x), ptr(mu), ptr(rs), ptr(sc), ptr(sf), slope, train, O(o['dx_' + k]), ptr(o['dgamma_' + k]), ptr(o['dbeta_' + k]),
                 ptr(o['dxsum_' + k]), M, C, wp, wn, st)
    o['act_dx'] = _nan((M, C), BF)
    call('da_act_bwd', A(dy), A(y), slope, O(o['act_dx']), M * C, st)
    yy = None if slope < 0 else y                                # (no activation: y may be null)
    o['add_dx'], o['dbias'] = _nan((M, C), BF), _nan((C,))
    call('da_act_bwd_add_dbias', A(dy), A(g2), A(yy), slope, O(o['add_dx']), ptr(o['dbias']), M, C, wp, wn, st)
    o['add1_dx'] = _nan((M, C), BF)
    call('da_act_bwd_add_dbias', A(dy), A(None), A(y), slope, O(o['add1_dx']), None, M, C, wp, wn, st)
    o['part_dx'], o['part_dbias'] = _nan((M, C), BF), _nan((C,))
    pbytes = int(nat.lib().da_bn_ws_bytes(M, C))
    pbuf, n = torch.empty(pbytes, dtype=torch.uint8, device=dev()), ctypes.c_int(-1)
    call('da_act_bwd_add_partial', A(dy), A(g2), A(yy), slope, O(o['part_dx']), M, C, ptr(pbuf), ctypes.c_size_t(pbytes), ctypes.byref(n), st)
    nat.call('da_colsum_finish', ptr(pbuf), n.value, C, ptr(o['part_dbias']), 0, st)
    o['part_dbias2'] = o['part_dbias'].clone()
    nat.call('da_colsum_finish', ptr(pbuf), n.value, C, ptr(o['part_dbias2']), 1, st)
    o['nparts'] = n.value
    o['colsum'] = _nan((C,))
    call('da_colsum', A(x), M, C, ptr(o['colsum']), wp, wn, st)
    torch.cuda.synchronize()
    return o


STREAM_STORED = ('y', 'dx_train', 'dx_train_nosum', 'dx_eval', 'dx_eval_nosum', 'act_dx', 'add_dx', 'add1_dx', 'part_dx')
STREAM_F32 = ('stats', 'rm', 'rv', 'dgamma_train', 'dbeta_train', 'dgamma_eval', 'dbeta_eval', 'dgamma_train_nosum', 'dbeta_eval_nosum', 'dbias', 'part_dbias', 'part_dbias2', 'colsum')


def _stream_body(case):
    """Every entry of norm_act.hip on one example: the twin against float64, and the twin against the conversion route, bit for bit."""
    tol = bx.TOL['stream']
    inp = bx.build_stream(case)
    M, C, slope = inp['M'], inp['C'], inp['slope']
    got, via = _run_stream(inp, False), _run_stream(inp, True)
    fused = bx.fused_dxsum(C)
    # the conversion route runs the fp32 instantiation of the same template between two casts: the same per-element arithmetic and the same order of every sum.
    # One exception, by construction: the stand-alone dxsum sums the STORED dx, which on the conversion route is still the unrounded fp32 tensor
    for k in STREAM_STORED + STREAM_F32 + (('dxsum_train', 'dxsum_eval') if fused else ()):
        assert _same_bits(got[k], via[k]), (case, k, 'twin and conversion route differ')
    r = bx.ref_stream(inp, torch.float64, decided=dict(y=_cpu(got['y'])))
    bx.check_band(r['band'])
    bx.close('stream', 'stats', got['stats'], r['stats'], tol['stats'])
    bx.close('stream', 'run', got['rm'], r['rm'], tol['run'])
    bx.close('stream', 'run', got['rv'], r['rv'], tol['run'])
    bx.stored_close('stream y', _cpu(got['y']), r['y'], tol['out'])
    for k in ('train', 'eval'):
        bx.close('stream', 'dgamma', got['dgamma_' + k], r['dgamma'], tol['dgamma'])
        bx.close('stream', 'dbeta', got['dbeta_' + k], r['dbeta'], tol['dbeta'])
        dx = _cpu(got['dx_' + k])
        bx.stored_close('stream dx ' + k, dx, r['dx_' + k], tol['dx'], unit=r['dx_unit'] if k == 'train' else None)
        assert _same_bits(got['dx_' + k], got['dx_%s_nosum' % k]) and _same_bits(got['dgamma_' + k], got['dgamma_%s_nosum' % k]), (case, k)
        # dxsum.  Fused (a thread keeps its channel quad): the sums of the fp32 dx BEFORE the store.  Stand-alone: da_colsum over the stored bf16 dx.
        pre, stored = r['dx_' + k], dx.double()
        bx.sum_close('stream', 'dxsum fused' if fused else 'dxsum stand-alone', got['dxsum_' + k], pre if fused else stored, tol['sum'], units=r['dx_units'] if k == 'train' else None)
        if not fused:      # the conversion route's stand-alone sum runs over its still unrounded fp32 dx
            bx.sum_close('stream bridge', 'dxsum stand-alone', via['dxsum_' + k], pre, tol['sum'], units=r['dx_units'] if k == 'train' else None)
        bx.note('stream', 'dxsum: |sum of the stored dx - sum of the unrounded dx| / sum |scale dz|', float(((stored.sum(0) - pre.sum(0)).abs() / r['dx_terms'].abs().sum(0).clamp_min(1e-300)).max()))
    bx.check_act_dx('stream act_bwd dx', _cpu(got['act_dx']), r['act_dx'], r['af'], slope, tol['act'])
    bx.check_act_dx('stream act_bwd_add dx', _cpu(got['add_dx']), r['add_dx'], r['af'], slope, tol['act'])
    assert _same_bits(got['add1_dx'], got['act_dx']) and _same_bits(got['part_dx'], got['add_dx']), case      # g2 null: act_bwd itself;  the two-call form: the same pass
    bx.sum_close('stream', 'dbias', got['dbias'], r['add_dx'], tol['sum'])                                    # (sums of the fp32 result before the store, as the kernel reads)
    assert got['nparts'] == bx.plan_rows(M, C)['grid'] and _same_bits(got['part_dbias'], got['dbias']), (case, got['nparts'])
    assert torch.equal(got['part_dbias2'], got['dbias'] + got['dbias']), case                                 # accumulate = 1
    bx.sum_close('stream', 'colsum', got['colsum'], inp['x'], tol['sum'])


def test_stream_random_shapes():
    """da_bn_train_stats_bf16, da_bn_act_fwd_bf16, da_bn_act_bwd_dbias_bf16 (train 1 / 0, dxsum given / null), da_act_bwd_bf16, da_act_bwd_add_dbias_bf16 (g2, y, dbias given /
    null), da_act_bwd_add_partial_bf16 + da_colsum_finish, da_colsum_bf16 at every class of bf16_cases.plan_rows."""
    bx.run_cases(bx.STREAM, _stream_body, pinned=bx.STREAM_PINNED)


@pytest.mark.parametrize('case', bx.STREAM_LARGE, ids=lambda c: '%dx%d' % (c['m'], c['c']))
def test_stream_large(case):
    """262 221 x 64: the 1024-workgroup cap binds (257 rows per workgroup, the last three workgroups start past M; four grid strides of bn_act_fwd, sixteen of the fused
    backward).  349 537 x 12: bn_act_fwd above one grid stride with a channel quad that changes per iteration."""
    p = bx.plan_rows(case['m'], case['c'])
    if case['c'] == 64:
        assert p['grid'] == 1024 and p['rows_per_block'] == 257 and bx.idle_workgroups(case['m'], 64) == 3
    else:
        assert case['m'] * 3 > 4096 * 256 and (4096 * 256) % 3 != 0
    bx.lc._state['case'] = case
    _stream_body(case)
    bx.write_report()


def test_act_bwd_sizes():
    """da_act_bwd_bf16 at numel % 4 = 0 ... 3, numel = 1 and 3 (the scalar 2-byte tail alone) and one size above a grid stride: bit equality at slopes -1 and 0 and
    wherever y > 0, the rounding of the float64 product elsewhere; the twin against the conversion route bit for bit."""
    from deepatlas_amd import _native as nat
    from deepatlas_amd.ops import A, O
    for i, numel in enumerate(bx.ACT_NUMEL):
        g = bx.to_bf16(bx.nrm((numel,), 70 + i))
        y = bx.to_bf16(bx.nrm((numel,), 71 + i) + 1.0)
        y[::7] = 0.0
        gd, yd = _bf(g), _bf(y)
        for slope in bx.SLOPES:
            bx.lc._state['case'] = (numel, slope)
            af = torch.ones_like(y) if slope < 0 else torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
            outs = []
            for bridge in (False, True):
                dx = _nan((numel + 8,), BF)                      # eight elements behind the end: they keep their NaN
                _Route(bridge)('da_act_bwd', A(gd), A(yd), slope, O(dx[:numel]), numel, nat.stream())
                torch.cuda.synchronize()
                assert bool(torch.isnan(dx[numel:]).all()), (numel, slope)
                outs.append(dx[:numel])
            assert _same_bits(outs[0], outs[1]), (numel, slope)
            bx.check_act_dx('stream act_bwd dx', _cpu(outs[0]), g.double() * af.double(), af, slope, bx.TOL['stream']['act'])
    bx.write_report()


# ---- family `pool` -------------------------------------------------------------------------------------------------------------------
def _run_pool(inp, bridge):
    from deepatlas_amd import _native as nat
    from deepatlas_amd.ops import A, O
    ptr, st, call = nat.ptr, nat.stream(), _Route(bridge)
    (N, D, H, W), C = inp['dims'], inp['c']
    x, dy, gskip, raw = (_bf(inp[k]) for k in ('x', 'dy', 'gskip', 'raw'))
    o = dict(y=_nan(dy.shape, BF), dx=_nan(x.shape, BF), dx_add=_nan(x.shape, BF))
    call('da_maxpool2_fwd', A(x), O(o['y']), N, D, H, W, C, st)
    call('da_maxpool2_bwd', A(dy), A(x), O(o['dx']), N, D, H, W, C, st)
    call('da_maxpool2_bwd_add', A(dy), A(x), A(gskip), O(o['dx_add']), N, D, H, W, C, st)
    if not ((D | H | W) & 1) and C % 4 == 0:
        sc, sf = inp['scale'].to(dev()), inp['shift'].to(dev())
        o['act'], o['pro_y'] = _nan(x.shape, BF), _nan(dy.shape, BF)
        call('da_maxpool2_fwd_pro', A(raw), ptr(sc), ptr(sf), inp['slope'], O(o['act']), O(o['pro_y']), N, D, H, W, C, st)
    for k in (0, 1):
        Do, Ho, Wo = bx.up_size(D, H, W, k)
        g = _bf(inp['up_dy%d' % k])
        o['up%d' % k], o['up_dx%d' % k] = _nan(g.shape, BF), _nan(x.shape, BF)
        call('da_upsample_nearest_fwd', A(x), O(o['up%d' % k]), N, D, H, W, C, Do, Ho, Wo, st)
        call('da_upsample_nearest_bwd', A(g), O(o['up_dx%d' % k]), N, D, H, W, C, Do, Ho, Wo, st)
    torch.cuda.synchronize()
    return o


def _pool_body(case):
    tol = bx.TOL['pool']
    inp = bx.build_pool(case)
    got, via = _run_pool(inp, False), _run_pool(inp, True)
    for k in got:
        assert _same_bits(got[k], via[k]), (case, k, 'twin and conversion route differ')
    r = bx.ref_pool(inp, torch.float64)
    bx.bits_equal('pool y', got['y'], r['y'])
    bx.bits_equal('pool dx', got['dx'], r['routed'])                      # the first maximum in (d, h, w) order; the odd trailing planes zero
    bx.bits_equal('pool dx add', got['dx_add'], (inp['gskip'].float() + r['routed'].float()).bfloat16())
    if 'act' in got:
        act = _cpu(got['act'])
        bx.stored_close('pool act', act, r['act'], tol['act'])
        bx.bits_equal('pool pro y', got['pro_y'], bx.ref_pool(dict(inp, x=act), torch.float64)['y'])      # the maximum over the STORED values
    for k in (0, 1):
        bx.bits_equal('pool up', got['up%d' % k], r['up%d' % k])
        bx.stored_bound('pool up dx', _cpu(got['up_dx%d' % k]), r['up_dx%d' % k], tol['up_dx'])


def test_pool_random_shapes():
    """da_maxpool2_{fwd, fwd_pro, bwd, bwd_add}_bf16 and da_upsample_nearest_{fwd, bwd}_bf16: D, H, W 2 ... 7 in every parity combination (the floor-mode trailing
    planes are cleared / copied by the byte, sized by the element type), inputs on a coarse grid (a tied maximum in every third window), C % 4 != 0 pinned."""
    bx.run_cases(bx.POOL, _pool_body, pinned=bx.POOL_PINNED)


def test_pool_prologue_declines():
    """da_maxpool2_fwd_pro_bf16: odd sizes, C % 4 != 0 and slope >= 1 return DA_ERR_UNSUPPORTED and leave both outputs untouched"""
    from deepatlas_amd import _native as nat
    for (D, H, W), C, slope in (((3, 4, 4), 8, 0.01), ((4, 5, 4), 8, 0.01), ((4, 4, 7), 8, 0.0), ((4, 4, 4), 6, 0.01), ((4, 4, 4), 8, 1.0), ((4, 4, 4), 8, 1.5)):
        x = _bf(bx.to_bf16(bx.nrm((1, D, H, W, C), 3)))
        sc, sf = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
        act, y = _nan(x.shape, BF), _nan((1, D // 2, H // 2, W // 2, C), BF)
        assert not nat.call_supported('da_maxpool2_fwd_pro_bf16', nat.ptr(x), nat.ptr(sc), nat.ptr(sf), slope, nat.ptr(act), nat.ptr(y), 1, D, H, W, C, nat.stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(act).all()) and bool(torch.isnan(y).all()), (D, H, W, C, slope)


# ---- family `head` -------------------------------------------------------------------------------------------------------------------
def _run_head(inp, bridge):
    from deepatlas_amd import _native as nat, ops
    from deepatlas_amd.ops import A, O
    ptr, st, call = nat.ptr, nat.stream(), _Route(bridge)
    N, V, cin, c = inp['N'], inp['V'], inp['cin'], inp['c']
    x, w, b, lab = _bf(inp['x']), inp['w'].to(dev()), inp['b'].to(dev()), inp['labels'].to(dev())
    lb = 8 if lab.dtype == torch.int64 else 1
    ps, pt, slope = (inp['scale'].to(dev()), inp['shift'].to(dev()), inp['pro']) if inp['pro'] is not None else (None, None, -1.0)
    wp, wn = nat.workspace.get(nat.lib().da_head_dice_ws_bytes(N, V, cin, c), dev())
    o = dict(loss=_nan((1,)), coef=_nan((2, N, c)), dx=_nan((N, V, cin), BF), dw=_nan((cin, c)), db=_nan((c,)))
    if ps is not None:          # the activated input as a stored tensor: what the prologue forms in registers
        o['act'] = _nan((N, V, cin), BF)
        nat.call('da_bn_act_fwd_bf16', ptr(x), ptr(ps), ptr(pt), slope, ptr(o['act']), N * V, cin, st)
    call('da_head_dice_fwd', A(x), ptr(ps), ptr(pt), slope, ptr(w), ptr(b), ptr(lab), lb, N, V, cin, c, ops._WEIGHT_TYPES['Uniform'], 0, bx.HEAD_EPS, ptr(o['loss']), ptr(o['coef']),
         wp, wn, st)
    gl = torch.ones(1, device=dev())
    call('da_head_dice_bwd', A(x), ptr(ps), ptr(pt), slope, ptr(w), ptr(b), ptr(lab), lb, ptr(o['coef']), ptr(gl), O(o['dx']), ptr(o['dw']), ptr(o['db']), N, V, cin, c, wp, wn, st)
    torch.cuda.synchronize()
    return o


def _head_compare(family, o, r, tol):
    e = bx.scalar_err(float(o['loss']), r['loss'], 'rel1')
    bx.note(family, 'loss', e)
    assert e < tol['loss'], (family, e)
    for k in ('coef', 'dw', 'db'):
        bx.close(family, k, o[k], r[k], tol[k])
    bx.stored_close(family + ' dx', _cpu(o['dx']), r['dx'], tol['dx'])


def _head_body(case):
    tol = bx.TOL['head']
    inp = bx.build_head(case)
    got, via = _run_head(inp, False), _run_head(inp, True)
    act = None
    if inp['pro'] is not None:
        act = _cpu(got['act'])
        bx.stored_close('head act', act, bx.head_act(inp, torch.float64), bx.F32_FLOOR)
    r = bx.ref_head(inp, torch.float64, act)
    _head_compare('head', got, r, tol)
    # The conversion route hands the fp32 entry the widened x: without a prologue the same numbers in the same kernel; with one, its activation stays fp32 where the
    # twin rounds it to bf16, so it is held to the float64 evaluation on the UNROUNDED activation.  Nobody has measured whether the routes are bit-equal: recorded.
    _head_compare('head bridge', via, r if act is None else bx.ref_head(inp, torch.float64, bx.head_act(inp, torch.float64)), tol)
    if act is None:
        a, b = _cpu(got['dx']).double(), _cpu(via['dx']).double()
        bx.note('head', 'twin vs bridge: share of dx elements that differ', float((a != b).double().mean()))
        bx.note('head', 'twin vs bridge: largest |dx difference| / max|dx|', float((a - b).abs().max() / a.abs().max()))
        bx.note('head', 'twin vs bridge: dW distance', bx.dist(got['dw'], via['dw'].double()))


def test_head_random_shapes():
    """da_head_dice_{fwd, bwd}_bf16: (Cin, C) in {16, 64} x {16, 32}, V below / at / above one and two 256-voxel chunks, N 1 ... 3, uint8 and int64 labels, with and without
    the prologue.  Loss, coef, dW, db fp32; dx stored bf16."""
    bx.run_cases(bx.HEAD, _head_body, pinned=bx.HEAD_PINNED)


def test_head_declines():
    """other channel counts: DA_ERR_UNSUPPORTED, outputs untouched"""
    from deepatlas_amd import _native as nat, ops
    ptr, st = nat.ptr, nat.stream()
    N, V = 2, 300
    for cin, c in bx.HEAD_DECLINED:
        x, w, b = _bf(bx.to_bf16(bx.nrm((N, V, cin), 1))), bx.nrm((cin, c), 2).to(dev()), bx.nrm((c,), 3).to(dev())
        lab = torch.zeros((N, V), dtype=torch.uint8, device=dev())
        wp, wn = nat.workspace.get(nat.lib().da_head_dice_ws_bytes(N, V, cin, c), dev())
        loss, coef, dx, dw, db = _nan((1,)), _nan((2, N, c)), _nan((N, V, cin), BF), _nan((cin, c)), _nan((c,))
        assert not nat.call_supported('da_head_dice_fwd_bf16', ptr(x), None, None, -1.0, ptr(w), ptr(b), ptr(lab), 1, N, V, cin, c, ops._WEIGHT_TYPES['Uniform'], 0, bx.HEAD_EPS,
                                      ptr(loss), ptr(coef), wp, wn, st)
        c0, gl = torch.zeros((2, N, c), device=dev()), torch.ones(1, device=dev())
        assert not nat.call_supported('da_head_dice_bwd_bf16', ptr(x), None, None, -1.0, ptr(w), ptr(b), ptr(lab), 1, ptr(c0), ptr(gl), ptr(dx), ptr(dw), ptr(db), N, V, cin, c, wp, wn, st)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (loss, coef, dx, dw, db)), (cin, c)


# ---- family `conv3` ------------------------------------------------------------------------------------------------------------------
def _nd(t, dtype):
    """NCDHW CPU tensor -> the kernels' NDHWC on the device"""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(dev()).to(dtype) if t is not None else None


def _nc(t):
    """a device NDHWC tensor -> NCDHW float on the CPU"""
    return _cpu(t).permute(0, 4, 1, 2, 3) if t is not None else None


def _c3_call(via, name, args, mask):
    """One entry through the C ABI (`abi`: the twin with `mask`), ops.call_act (`act`) or ops.call_act with BF16_FORCE_BRIDGE (`bridge`).
    Returns (ran, conversion passes counted)."""
    from deepatlas_amd import _native as nat, ops
    if via == 'abi':
        return nat.call_supported(name + '_bf16', *([(nat.ptr(a.t) if isinstance(a, ops.A) else a) for a in args] + [mask])), 0
    prev, before = ops.BF16_FORCE_BRIDGE, ops.bridged_calls.get(name, 0)
    ops.BF16_FORCE_BRIDGE = via == 'bridge'
    try:
        ok = ops.call_act(name, *args, may_decline=True)
    finally:
        ops.BF16_FORCE_BRIDGE = prev
    return ok, ops.bridged_calls.get(name, 0) - before


class _C3(object):
    """the device tensors of one family-`conv3` example and its entries"""

    def __init__(self, case, inp):
        from deepatlas_amd import _native as nat
        self.case, self.inp, self.nat = case, inp, nat
        kind = case['kind']
        self.tx, self.ty, self.tdx = (torch.float32 if kind == 'first' else BF), (torch.float32 if kind == 'flow' else BF), (torch.float32 if kind == 'first' else BF)
        self.x1, self.x2, self.dy = _nd(inp['x1'], self.tx), _nd(inp['x2'], self.tx), _nd(inp['dy'], self.ty)
        self.w = inp['w'].permute(2, 3, 4, 1, 0).reshape(27, inp['c1'] + inp['c2'], inp['cout']).contiguous().to(dev())
        self.b = inp['b'].to(dev())
        self.dims, self.c1, self.c2, self.cout, self.stride = inp['dims'], inp['c1'], inp['c2'], inp['cout'], inp['stride']
        N, D, H, W = self.dims
        self.yshape, self.xshape = (N,) + tuple(inp['odims']) + (self.cout,), (N, D, H, W)
        self.ws = nat.workspace.get(nat.lib().da_conv3d_k3_ws_bytes(N, D, H, W, self.c1 + self.c2, self.cout, self.stride), dev())
        self.masks = bx.c3_masks(case)

    def fwd(self, via, slope, x1=None, x2=None):
        from deepatlas_amd.ops import A, O
        y = _nan(self.yshape, self.ty)
        ok, nb = _c3_call(via, 'da_conv3d_k3_fwd', [A(self.x1 if x1 is None else x1), self.c1, A(self.x2 if x2 is None else x2), self.c2, self.nat.ptr(self.w), self.nat.ptr(self.b), O(y)] +
                          list(self.dims) + [self.cout, self.stride, float(slope), self.ws[0], self.ws[1], self.nat.stream()], self.masks[0])
        return ok, nb, y

    def bnstats(self, via):
        from deepatlas_amd.ops import A, O
        y, pbuf, n = _nan(self.yshape, self.ty), _nan((512, 2, self.cout), torch.float64), ctypes.c_int(-1)
        ok, nb = _c3_call(via, 'da_conv3d_k3_fwd_bnstats', [A(self.x1), self.c1, A(self.x2), self.c2, self.nat.ptr(self.w), self.nat.ptr(self.b), O(y)] + list(self.dims) +
                          [self.cout, self.stride, self.nat.ptr(pbuf), 512, ctypes.byref(n), self.ws[0], self.ws[1], self.nat.stream()], self.masks[0])
        return ok, nb, y, pbuf, n.value

    def dgrad(self, via):
        from deepatlas_amd.ops import A, O
        dx1 = _nan(self.xshape + (self.c1,), self.tdx)
        dx2 = _nan(self.xshape + (self.c2,), self.tdx) if self.c2 else None
        ok, nb = _c3_call(via, 'da_conv3d_k3_dgrad', [A(self.dy), self.nat.ptr(self.w), O(dx1), self.c1, O(dx2), self.c2] + list(self.dims) +
                          [self.cout, self.stride, self.ws[0], self.ws[1], self.nat.stream()], self.masks[1])
        return ok, nb, dx1, dx2

    def wgrad(self, via, dbias=None, x1=None, x2=None):
        from deepatlas_amd.ops import A
        dw = _nan((27, self.c1 + self.c2, self.cout))
        ok, nb = _c3_call(via, 'da_conv3d_k3_wgrad', [A(self.x1 if x1 is None else x1), self.c1, A(self.x2 if x2 is None else x2), self.c2, A(self.dy), self.nat.ptr(dw), self.nat.ptr(dbias)] +
                          list(self.dims) + [self.cout, self.stride, self.ws[0], self.ws[1], self.nat.stream()], self.masks[2])
        return ok, nb, dw

    def pro_args(self, both):
        ptr, inp = self.nat.ptr, self.inp
        self.pro_keep = [inp['scale1'].to(dev()), inp['shift1'].to(dev())] + ([inp['scale2'].to(dev()), inp['shift2'].to(dev())] if both else [])
        k = self.pro_keep
        return (ptr(k[0]), ptr(k[1]), 0.01), ((ptr(k[2]), ptr(k[3]), 0.01) if both else (None, None, -1.0))

    def acts(self, both):
        """the stored activated tensors the prologue stands for (da_bn_act_fwd_bf16)"""
        out = []
        for i, raw in ((1, self.x1), (2, self.x2)) if both else ((1, self.x1),):
            k, a = self.pro_keep[2 * (i - 1): 2 * i], _nan(raw.shape, BF)
            self.nat.call('da_bn_act_fwd_bf16', self.nat.ptr(raw), self.nat.ptr(k[0]), self.nat.ptr(k[1]), 0.01, self.nat.ptr(a), raw.numel() // raw.shape[-1], raw.shape[-1], self.nat.stream())
            out.append(a)
        return out + [None] * (2 - len(out))

    def fwd_pro(self, via, both, stats):
        from deepatlas_amd.ops import A, O
        p1, p2 = self.pro_args(both)
        y, pbuf, n = _nan(self.yshape, self.ty), _nan((512, 2, self.cout), torch.float64), ctypes.c_int(-1)
        ok, nb = _c3_call(via, 'da_conv3d_k3_fwd_pro', [A(self.x1), self.c1, p1[0], p1[1], p1[2], A(self.x2), self.c2, p2[0], p2[1], p2[2], self.nat.ptr(self.w), self.nat.ptr(self.b), O(y)] +
                          list(self.dims) + [self.cout, -1.0, self.nat.ptr(pbuf) if stats else None, 512 if stats else 0, ctypes.byref(n), self.ws[0], self.ws[1], self.nat.stream()], self.masks[0])
        return ok, nb, y, pbuf, n.value

    def wgrad_pro(self, via, both):
        from deepatlas_amd.ops import A
        p1, p2 = self.pro_args(both)
        dw = _nan((27, self.c1 + self.c2, self.cout))
        ok, nb = _c3_call(via, 'da_conv3d_k3_wgrad_pro', [A(self.x1), self.c1, p1[0], p1[1], p1[2], A(self.x2), self.c2, p2[0], p2[1], p2[2], A(self.dy), self.nat.ptr(dw)] + list(self.dims) +
                          [self.cout, self.ws[0], self.ws[1], self.nat.stream()], self.masks[2])
        return ok, nb, dw


def _dw(dw):
    """[27][Cin][Cout] -> [Cout][Cin][3, 3, 3]"""
    return dw.detach().cpu().reshape(3, 3, 3, dw.shape[1], dw.shape[2]).permute(4, 3, 0, 1, 2)


def _c3_check(case, q, got, ref, family='conv3'):
    """one result against float64: a stored tensor by stored_close, an fp32 one by close"""
    kind, tol = case['kind'], bx.c3_tol(case['kind'])
    if q != 'dw' and got.dtype == BF:
        bx.stored_close('%s %s %s' % (family, kind, q), _nc(got), ref, tol[q])
    else:
        bx.close(family, '%s %s' % (kind, q), _dw(got) if q == 'dw' else _nc(got), ref, tol[q])


def _twin_vs_bridge(case, q, a, b):
    a, b = _cpu(a).double(), _cpu(b).double()
    bx.note('conv3', 'twin vs bridge, %s %s: share of elements that differ' % (case['kind'], q), float((a != b).double().mean()))
    bx.note('conv3', 'twin vs bridge, %s %s: largest |difference| / max|value|' % (case['kind'], q), float((a - b).abs().max() / a.abs().max().clamp_min(1e-300)))


def _three_ways(case, run, route, outs):
    """run(via) -> (ran, conversion passes, *tensors).  The C-ABI twin with the mask written down in bf16_cases.c3_masks runs exactly when `route` says so and leaves its outputs
    untouched otherwise; ops.call_act reaches the same route with the mask it builds itself (no conversion pass, the same bits) or converts when the twin declines;
    the forced conversion route is returned too.  Returns (the call_act result, the forced-conversion result)."""
    abi, act, via = run('abi'), run('act'), run('bridge')
    torch.cuda.synchronize()
    assert abi[0] == (route is not None), (case, route, abi[0])
    assert act[0] and act[1] == int(route is None) and via[0] and via[1] == 1, (case, route, act[:2], via[:2])
    for k in outs:
        if abi[k] is None:
            continue
        if route is None:
            assert bool(torch.isnan(abi[k]).all()), (case, 'a declined call wrote its output')
        else:
            assert _same_bits(abi[k], act[k]), (case, 'ops.call_act and the C ABI differ')
    return act, via


def _conv3_body(case):
    inp = bx.build_conv3(case)
    kind, (c1, c2), cout = case['kind'], case['ch'], case['cout']
    rf, rd, rw = bx.c3_routes(case)
    t = _C3(case, inp)
    N, D, H, W = inp['dims']
    # forward + activation
    act, via = _three_ways(case, lambda v: t.fwd(v, inp['slope']), rf, (2,))
    r = bx.ref_conv3(inp, torch.float64, decided=_nc(act[2]))
    bx.check_band(r['band'])
    _c3_check(case, 'y', act[2], r['y'])
    rb = r if torch.equal(_nc(via[2]) > 0, _nc(act[2]) > 0) else bx.ref_conv3(inp, torch.float64, decided=_nc(via[2]))
    _c3_check(case, 'y', via[2], rb['y'], 'conv3 bridge')
    if rf is not None:
        _twin_vs_bridge(case, 'y', act[2], via[2])
    # forward + statistics: the partial sums are taken from the accumulators, before the store; none on the thin and stride-2 routes
    act, via = _three_ways(case, t.bnstats, rf, (2,))
    zr = r['z'].movedim(1, -1).reshape(-1, cout)
    for res, fam, native in ((act, 'conv3', rf), (via, 'conv3 bridge', 'mfma' if kind == 'mfma' else 'other')):
        _c3_check(case, 'y', res[2], r['z'], fam)
        if native == 'mfma':
            tiles, n = bx.bc.ntiles(N, D, H, W), res[4]
            assert 0 < n <= min(512, tiles) and (n == tiles or n % 8 == 0) and bool(torch.isnan(res[3][n:]).all()), (case, fam, n, tiles)
            bx.sum_close(fam, 'sum y', res[3][:n, 0].sum(0), zr, bx.TOL['conv3']['sum'])
            bx.sum_close(fam, 'sum y^2', res[3][:n, 1].sum(0), zr * zr, bx.TOL['conv3']['sum'])
        elif native is not None:
            assert res[4] == 0 and bool(torch.isnan(res[3]).all()), (case, fam, res[4])
    if rf is not None:
        _twin_vs_bridge(case, 'y of fwd_bnstats', act[2], via[2])
    # data gradient
    act, via = _three_ways(case, t.dgrad, rd, (2, 3))
    for res, fam in ((act, 'conv3'), (via, 'conv3 bridge')):
        _c3_check(case, 'dx', res[2], r['dx1'], fam)
        if c2:
            _c3_check(case, 'dx', res[3], r['dx2'], fam)
    if rd is not None:
        _twin_vs_bridge(case, 'dx', act[2], via[2])
    # weight gradient; a bias gradient is not the twin's to give
    act, via = _three_ways(case, t.wgrad, rw, (2,))
    _c3_check(case, 'dw', act[2], r['dw'])
    _c3_check(case, 'dw', via[2], r['dw'], 'conv3 bridge')
    if rw is not None:
        _twin_vs_bridge(case, 'dw', act[2], via[2])
    db = _nan((cout,))
    ok, _, dw = t.wgrad('abi', dbias=db)
    torch.cuda.synchronize()
    assert not ok and bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()), case
    if kind != 'mfma':
        return
    # the prologue entries: the stored activated tensor (da_bn_act_fwd_bf16) is held to float64, then it is the reference's input
    both, stats = case['pro'] != 'in1' and c2 > 0, case['pro'] == 'stats'
    p1, p2 = t.pro_args(both)
    a1, a2 = t.acts(both)
    torch.cuda.synchronize()
    for i, a in ((1, a1), (2, a2)):
        if a is not None:
            bx.stored_close('conv3 act', _nc(a), bx.pro_act(inp, i, 0.01, torch.float64), bx.TOL['conv3']['act'])
    rp = bx.ref_conv3(inp, torch.float64, slope=-1.0, x1=_nc(a1), x2=_nc(a2) if a2 is not None else None)
    ok, _, y, pbuf, n = t.fwd_pro('abi', both, stats)
    ok2, nb, y2, _, n2 = t.fwd_pro('act', both, stats)
    torch.cuda.synchronize()
    assert ok and ok2 and nb == 0 and _same_bits(y, y2) and n == n2, (case, ok, ok2, nb)
    _c3_check(case, 'y', y, rp['z'], 'conv3 pro')
    if stats:
        assert 0 < n <= 512 and bool(torch.isnan(pbuf[n:]).all()), (case, n)
        zr = rp['z'].movedim(1, -1).reshape(-1, cout)
        bx.sum_close('conv3', 'sum y', pbuf[:n, 0].sum(0), zr, bx.TOL['conv3']['sum'])
        bx.sum_close('conv3', 'sum y^2', pbuf[:n, 1].sum(0), zr * zr, bx.TOL['conv3']['sum'])
    else:
        assert n == 0
    ok, _, dw = t.wgrad_pro('abi', both)
    ok2, nb, dw2 = t.wgrad_pro('act', both)
    torch.cuda.synchronize()
    assert ok and ok2 and nb == 0 and _same_bits(dw, dw2), (case, ok, ok2, nb)
    _c3_check(case, 'dw', dw, rp['dw'], 'conv3 pro')
    # The conversion route hands the fp32 prologue entries the widened raw tensors.  Their activation is formed in fp32 and, in the bf16 matrix mode, rounded to bf16 as
    # every matrix operand is when it is staged: the operand is the tensor da_bn_act_fwd_bf16 stores, so this side is held to the same float64 reference
    okb, nbb, yb, pbufb, n_b = t.fwd_pro('bridge', both, stats)
    okw, nbw, dwb = t.wgrad_pro('bridge', both)
    torch.cuda.synchronize()
    assert okb and okw and nbb == 1 and nbw == 1 and n_b == n, (case, okb, okw, nbb, nbw, n_b, n)
    _c3_check(case, 'y', yb, rp['z'], 'conv3 pro bridge')
    _c3_check(case, 'dw', dwb, rp['dw'], 'conv3 pro bridge')
    if stats:
        bx.sum_close('conv3 pro bridge', 'sum y', pbufb[:n_b, 0].sum(0), zr, bx.TOL['conv3']['sum'])
        bx.sum_close('conv3 pro bridge', 'sum y^2', pbufb[:n_b, 1].sum(0), zr * zr, bx.TOL['conv3']['sum'])
    _twin_vs_bridge(case, 'y of fwd_pro', y, yb)
    _twin_vs_bridge(case, 'dw of wgrad_pro', dw, dwb)
    # ... and the plain entries on the stored activated tensors give the same bits as the prologue entries on the raw ones
    okf, _, y3 = t.fwd('abi', -1.0, x1=a1, x2=a2)
    okw, _, dw3 = t.wgrad('abi', x1=a1, x2=a2)
    torch.cuda.synchronize()
    assert okf and okw
    bx.note('conv3', 'prologue vs materialised: share of y elements that differ', float((_cpu(y) != _cpu(y3)).double().mean()))
    bx.note('conv3', 'prologue vs materialised: dW distance', bx.dist(dw, dw3.double()))


def test_conv3_random_shapes():
    """da_conv3d_k3_{fwd, fwd_bnstats, fwd_pro, wgrad_pro, dgrad, wgrad}_bf16 in the bf16 matrix mode: the all-bf16 matrix route at every channel class of pick_ck with and
    without a second input, the mixed thin routes (fp32 -> bf16 first layers, bf16 -> fp32 flow conv, the few-Cin and flow weight gradients) and stride 2, each through
    the C ABI with the mask written down by hand, through ops.call_act with the mask it builds, and through the conversion route."""
    from test_gpu_block_shapes import _mode
    bx.check_c3_pinned()
    with _mode('bf16'):
        bx.run_cases(bx.C3, _conv3_body, pinned=bx.C3_PINNED)


def _every_entry(t, masks, both):
    """(entry, ran, outputs) of the six entries through the C ABI with the (forward, data-gradient, weight-gradient) masks"""
    t.masks = masks
    r = []
    ok, _, y = t.fwd('abi', -1.0)
    r.append(('fwd', ok, [y]))
    ok, _, y, pbuf, n = t.bnstats('abi')
    r.append(('fwd_bnstats', ok, [y]))
    assert n == 0 or (ok and n > 0)
    ok, _, dx1, dx2 = t.dgrad('abi')
    r.append(('dgrad', ok, [dx1, dx2]))
    ok, _, dw = t.wgrad('abi')
    r.append(('wgrad', ok, [dw]))
    if t.case['kind'] == 'mfma':
        ok, _, y, pbuf, n = t.fwd_pro('abi', both, True)
        r.append(('fwd_pro', ok, [y, pbuf]))
        assert n == 0 or (ok and n > 0)
        ok, _, dw = t.wgrad_pro('abi', both)
        r.append(('wgrad_pro', ok, [dw]))
    torch.cuda.synchronize()
    return r


def _expect(t, masks, why, mode1=True):
    """every entry runs exactly when bf16_cases.c3_route names a route for its mask (never outside the bf16 matrix mode, the VALU kernels apart), and a declined call
    leaves its outputs untouched"""
    (c1, c2), cout, s = t.case['ch'], t.case['cout'], t.case['stride']
    both = c2 > 0
    for entry, ok, outs in _every_entry(t, masks, both):
        base = {'fwd_bnstats': 'fwd', 'fwd_pro': 'fwd', 'wgrad_pro': 'wgrad'}.get(entry, entry)
        route = bx.c3_route(base, c1, c2, cout, s, masks[{'fwd': 0, 'dgrad': 1, 'wgrad': 2}[base]], pro=entry.endswith('_pro'))
        want = route is not None and (mode1 or route in ('thin', 'fewcin', 'flow'))
        assert ok == want, (why, entry, masks, route, ok)
        if not ok:
            assert all(bool(torch.isnan(o).all()) for o in outs if o is not None), (why, entry, masks, 'a declined call wrote its output')


def test_conv3_declines():
    """DA_ERR_UNSUPPORTED with the outputs untouched: every partial mask of a matrix-shaped layer in the bf16 matrix mode, with one and with two inputs; the full mask
    while the matrix mode is not 1 (matrix and stride-2 routes); one bf16 and one fp32 input on a thin shape; stride 2 at channel counts its kernels do not take."""
    from test_gpu_block_shapes import _mode
    base = dict(slope=-1.0, pro='both', raw_w=False, sd=77, stride=1)
    mfma, single = dict(base, kind='mfma', ch=(16, 16), cout=16, dims=(1, 4, 8, 16)), dict(base, kind='mfma', ch=(16, 0), cout=16, dims=(1, 4, 8, 16))
    s2 = dict(base, kind='s2', ch=(16, 0), cout=16, dims=(1, 5, 9, 17), stride=2)
    with _mode('bf16'):
        for case in (mfma, single):
            t = _C3(case, bx.build_conv3(case))
            for m in range(8):
                _expect(t, (m, m, m), 'partial mask')
        # a thin shape with one bf16 and one fp32 input (masks as ops.call_act would build them)
        flow = dict(base, kind='flow', ch=(8, 16), cout=3, dims=(1, 4, 8, 16))
        t = _C3(flow, bx.build_conv3(flow))
        t.x2 = t.x2.float()
        assert bx.c3_route('fwd', 8, 16, 3, 1, 1) is None and bx.c3_route('dgrad', 8, 16, 3, 1, 2) is None and bx.c3_route('wgrad', 8, 16, 3, 1, 1) is None
        _expect(t, (1, 2, 1), 'mixed inputs')
        # stride 2 outside da_conv3_s2_supported
        for ch, cout in (((8, 0), 16), ((48, 0), 16), ((16, 0), 6)):
            c = dict(s2, ch=ch, cout=cout)
            assert bx.c3_routes(c) == (None, None, None)
            _expect(_C3(c, bx.build_conv3(c)), (5, 3, 5), 'stride 2')
    for mode in ('fp32', 'fp32_split'):
        with _mode(mode):
            for case, masks in ((mfma, (7, 7, 7)), (s2, (5, 3, 5))):
                _expect(_C3(case, bx.build_conv3(case)), masks, 'matrix mode ' + mode, mode1=False)
