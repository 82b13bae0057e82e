"""Shared by tests/test_gpu_bf16_shapes.py (the `_bf16` activation-storage twins of norm_act.hip, pool.hip, headdice.hip and the six masked 3x3x3 convolution twins of
conv3d.hip, entry by entry through the C ABI and ops.call_act, against float64) and tests/test_bf16_reference.py (an fp32 torch-CPU oracle that rounds to bf16 where the
product stores, against float64 on the same examples, no GPU): strategies, pinned examples (one per launcher branch, reached by construction), builders, the float64
references, the launcher decisions the pinned sizes are built on (restated), and the bounds.

Conventions are those of tests/pointwise_cases.py: every family runs `run_cases` (loss_cases.run_cases: seed 160950, the pinned examples first, then 60 derandomised
examples, at least 90 % compared to the end); distances by `close` / `dist` / `note`; activation kinks that a kernel decides on a RECOMPUTED z = x scale + shift by
block_cases.activate (guard band |z| < G max|z|, capped per tensor at 0.1 % of its elements and 64); stored tensors by pointwise_cases.bf16_close.  With
DA_BF16_SHAPES_REPORT=<path> set, run_cases writes the worst figure per family and quantity to that JSON file.

Inputs are drawn in fp32, rounded to bf16 (to_bf16) and handed to the device as bf16 tensors; the float64 reference takes the widened values.  What a kernel decides on
a GIVEN bf16 tensor (act_bwd on y, the pool's arg-max) is exact and gets no band.

Bounds.
  fp32 results       the tolerance the same quantity's fp32 family asserts (TOL below names the source of each), lowered by the project's rule where the measurement allows.
  stored bf16, all   bf16_close: |got - ref| <= 2^-8 |ref| + tol max|ref|.
  stored bf16, mode  rne_check: wherever the float64 reference is farther than tol max|ref| from a bf16 rounding midpoint the stored value IS round-to-nearest-even of
                     the reference; the elements nearer than that are left out, at most LEFT_OUT_MAX of a tensor.
  bit equality       selections, copies and single correctly rounded fp32 operations (bits_equal).

Plain module, no fixtures, no pytest settings."""
import json
import os

import torch
import torch.nn.functional as F
from hypothesis import strategies as st

import block_cases as bc
import loss_cases as lc
import regconv_cases as rc
from block_cases import BAND_ELEMS, EPS, MOMENTUM, activate, check_band, col_err, nrm        # noqa: F401  (re-exported for the two test files)
from loss_cases import _cyc, _f64, close, dist, note, scalar_err                             # noqa: F401
from pointwise_cases import BF16_EPS, bf16_close, to_bf16                                    # noqa: F401

FAMILIES = ('stream', 'pool', 'conv3', 'head')
LEFT_OUT_MAX = 0.20        # rne_check: the largest share of a tensor that may lie within tol max|ref| of a rounding midpoint
TIE_MIN = 0.30             # family `pool`: share of the pooling windows (per channel) that hold a tied maximum, over a run
F32_FLOOR = 8 * 2.0 ** -24   # eight roundings of an fp32 value (4.8e-7): block_cases' floor for one short fp32 expression


def run_cases(strategy, body, pinned=()):
    ran = lc.run_cases(strategy, body, pinned)
    write_report()
    return ran


def write_report():
    path = os.environ.get('DA_BF16_SHAPES_REPORT')
    if path:
        def mine(k):
            fam, what = k.split('/', 1)
            return any(w in FAMILIES for w in fam.split()) or (fam == 'bf16' and what.split()[0] in FAMILIES)
        with open(path, 'w') as f:
            json.dump({k: v for k, v in lc.WORST.items() if mine(k)}, f, indent=1, sort_keys=True)


# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# CEIL: what the fp32 family of the same quantity asserts today.
#   stream  stats, run: block_cases.TOL['sums'] (mean | rstd | scale | shift and the running statistics of da_bn_train_stats_from_partials); out, dx, dgamma, dbeta:
#           block_cases.TOL['block'] (ops.ConvBNActFn's BatchNorm quantities); sum: 1e-6 of sum |term| (block_cases' epilogue sums; here the column sums da_colsum, the
#           bias gradient dxsum / dbias); act: F32_FLOOR -- act_bwd and act_bwd_add are one or two fp32 operations per element on bf16 operands, nothing the fp32 suite
#           bounds looser than check()'s 1e-4 would be a bound on them, so the number format gives it: at most two roundings of 2^-24 each, asserted at eight
#   pool    act: F32_FLOOR (da_maxpool2_fwd_pro: one multiply-add and one multiply per element); up_dx: 1e-6, test_pool_and_upsample_random_shapes' 'nearest bwd'
#   head    block_cases.TOL['sums']['head'] (test_fused_head_softmax_dice_vs_torch_cpu) for the loss, coef, dx, dW, db
#   conv3   regconv_cases.TOL[...]['fp32_split'] = 1e-5 for out, dx, dw of every registration-net route and block_cases.TOL['sums'] for the matrix route's y, dx and sums;
#           dw of the matrix route: block_cases.TOL['block']['dw']
# TOL: what both files assert, never above CEIL.  Rule (tests/loss_cases.py): where max(4 x device worst, 8 x fp32-oracle worst) is more than 10 x below the ceiling, that
# value rounded up to two digits; otherwise the ceiling.  The figures are in the table of tests/test_gpu_bf16_shapes.py.
CEIL = {
    'stream': {'stats': bc.TOL['sums']['stats'], 'run': bc.TOL['sums']['run'], 'out': bc.TOL['block']['out'], 'dx': bc.TOL['block']['dx'], 'dgamma': bc.TOL['block']['dgamma'],
               'dbeta': bc.TOL['block']['dbeta'], 'sum': 1e-6, 'act': F32_FLOOR},
    'pool': {'act': F32_FLOOR, 'up_dx': 1e-6},
    'head': dict.fromkeys(('loss', 'coef', 'dx', 'dw', 'db'), bc.TOL['sums']['head']),
    'conv3': {'y': bc.TOL['sums']['y'], 'dx': bc.TOL['sums']['dx'], 'dw': bc.TOL['block']['dw'], 'sum': bc.TOL['sums']['sum'], 'thin': 1e-5, 'act': F32_FLOOR},
}
# A stored tensor's `tol` is measured as the smallest tol at which its two checks hold ("tol needed" in the report) and is never taken below F32_FLOOR.
TOL = {
    # out, dx: device 0 / 5.0e-8, oracle 1.7e-8 / 3.4e-8 needed -> the floor;  stats, run, dgamma, dbeta, sum: max(4 x device, 8 x oracle) = 1.9e-6, 1.9e-6, 2.2e-6, 1.7e-6,
    # 8.4e-7 are less than 10 x below their ceilings: stay
    'stream': dict(CEIL['stream'], out=F32_FLOOR, dx=F32_FLOOR),
    'pool': dict(CEIL['pool']),                   # up_dx: nothing needed on either side; the floor is less than 10 x below 1e-6: stays
    # loss 8 x 3.0e-8 (oracle), coef 8 x 3.2e-7, dW 8 x 5.5e-7, db 8 x 5.3e-7 (4 x device: 1.6e-7, 1.4e-6, 3.1e-6, 2.5e-6);  dx: device 5.5e-8, oracle 4.6e-8 needed -> the floor
    'head': {'loss': 2.4e-7, 'coef': 2.6e-6, 'dx': F32_FLOOR, 'dw': 4.4e-6, 'db': 4.3e-6},
    # y: device 1.3e-7, oracle 7.0e-8 needed -> 5.6e-7;  dx: 8 x the oracle's 1.1e-7 = 8.5e-7 is less than 10 x below 6.3e-6: stays;  dw 8 x 6.9e-7 = 5.5e-6, sum 6.4e-7,
    # thin 8 x 4.5e-7 = 3.6e-6: stay
    'conv3': dict(CEIL['conv3'], y=5.6e-7),
}
assert all(TOL[f][k] <= CEIL[f][k] for f in CEIL for k in CEIL[f])


def quarter_of(v):
    """a quarter of a tolerance (the project's margin for the fp32 oracle), but not below the floor of eight fp32 roundings: a quarter of the floor is two roundings, fewer
    than the expressions have operations"""
    return min(v, max(v / 4, F32_FLOOR))


def quarter(family):
    """what the fp32 oracle is held to, fp32 results and the `tol` of stored tensors alike"""
    return {k: quarter_of(v) for k, v in TOL[family].items()}


# ---- comparisons of stored tensors -------------------------------------------------------------------------------------------------
def rne(ref):
    """round-to-nearest-even of a float64 tensor to bf16, widened to float64 (through fp32: the double rounding can only matter within 2^-24 |ref| of a midpoint,
    which rne_check leaves out)"""
    return ref.detach().double().float().bfloat16().double()


def trunc_bf16(t):
    """the WRONG store: the upper 16 bits of the fp32 value"""
    return (t.detach().float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def midpoint_distance(ref):
    """|ref - m|, m the midpoint of the two bf16 neighbours of ref"""
    ref = ref.detach().double().cpu().contiguous()
    lo_bits = ref.float().view(torch.int32) & -65536
    lo, hi = lo_bits.view(torch.float32).double(), (lo_bits + 65536).view(torch.float32).double()
    return (ref - 0.5 * (lo + hi)).abs()


def rne_check(what, got, ref, tol, unit=0.0, cap_tol=None):
    """The rounding mode of a stored tensor.  Returns the left-out share (recorded; asserted <= LEFT_OUT_MAX).  unit: see stored_close.
    cap_tol: the (larger) tol at which the left-out share is measured and capped -- the CPU file holds its oracle to a quarter of the device's tol and proves the cap at
    the device's own."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(float(ref.abs().max()), unit)
    far = midpoint_distance(ref) > tol * scale
    out = ~(midpoint_distance(ref) > (cap_tol or tol) * scale)
    share = float(out.double().mean()) if ref.numel() else 0.0
    note('bf16', what + ' (rounding mode: left-out share)', share)
    assert share <= LEFT_OUT_MAX, 'bf16 %s: %.3f of the tensor lies within tol max|ref| of a rounding midpoint' % (what, share)
    miss = got != rne(ref)
    # measured: the smallest tol at which every mismatch would have been left out (0 when the stored tensor is the rounding of the reference everywhere)
    note('bf16', what + ' (rounding mode: tol needed)', float((midpoint_distance(ref)[miss] / max(float(ref.abs().max()), unit, 1e-300)).max()) if bool(miss.any()) else 0.0)
    bad = far & miss
    assert not bool(bad.any()), 'bf16 %s: %d of %d elements are not the round-to-nearest-even of the reference' % (what, int(bad.sum()), ref.numel())
    return share


def stored_bound(what, got, ref, tol):
    """bf16_close alone, for a stored tensor whose exact value often IS a rounding midpoint (sums of bf16 values): no mode check"""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    note('bf16', what + ' (stored bf16: tol needed)', float((((g - r).abs() - BF16_EPS * r.abs()).clamp_min(0.0) / max(float(r.abs().max()), 1e-300)).max()) if r.numel() else 0.0)
    bf16_close(what, got, ref, tol)


def stored_close(what, got, ref, tol, unit=None, cap_tol=None):
    """a stored bf16 tensor against float64: every element within one spacing (bf16_close) and the rounding mode (rne_check).
    unit (None: the plain formula): the largest magnitude among the TERMS of the expression, for a result that is a difference of larger terms (the train-mode BatchNorm backward: at M = 1 it
    is zero in exact arithmetic and a few fp32 roundings of scale dz on any machine) -- the absolute part of both bounds is then tol max(max|ref|, unit)."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), what
    # measured: the smallest tol at which the one-spacing bound holds
    note('bf16', what + ' (stored bf16: tol needed)', float((((g - r).abs() - BF16_EPS * r.abs()).clamp_min(0.0) / max(float(r.abs().max()), unit or 0.0, 1e-300)).max()) if r.numel() else 0.0)
    if unit is None:
        bf16_close(what, got, ref, tol)
        return rne_check(what, got, ref, tol, cap_tol=cap_tol)
    e = float(((g - r).abs() / (BF16_EPS * r.abs() + tol * max(float(r.abs().max()), unit))).max())
    note('bf16', what + ' (stored bf16, fraction of its bound)', e)
    assert e <= 1.0, 'bf16 %s: %.3f of the bound' % (what, e)
    if float(r.abs().max()) == 0.0:       # (identically zero: nothing is rounded)
        return 0.0
    return rne_check(what, got, ref, tol, unit, cap_tol)


def check_act_dx(what, got, ref, af, slope, tol):
    """dx of act_bwd / act_bwd_add: where the factor is 1 (every element at slopes -1 and 0, where 0 selects a signed zero) the fp32 result is exact -- a copy, or a sum
    of two bf16 values, which very often lies EXACTLY on a rounding midpoint: ties-to-even is asserted there by bit equality -- and where it is the slope the stored
    value is one spacing from, and the rounding of, the float64 product"""
    got, ref, af = got.detach().double().cpu(), ref.detach().double().cpu(), af.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), what
    one = (af == 1) | (af == 0)
    bits_equal(what, got[one], rne(ref[one]))
    if slope > 0 and int((~one).sum()):
        stored_close(what, got[~one], ref[~one], tol)


def bits_equal(what, got, ref):
    """bit equality of two bf16 tensors (ref: a tensor of exactly representable values in any float dtype, or a bf16 tensor)"""
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    if ref.dtype != torch.bfloat16:
        rb = ref.to(torch.bfloat16)
        assert torch.equal(rb.double(), ref.double()), what + ': the reference is not bf16-representable'
        ref = rb
    if got.dtype != torch.bfloat16:
        gb = got.to(torch.bfloat16)
        assert bool(torch.isnan(got).any()) or torch.equal(gb.double(), got.double()), what
        got = gb
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    n = int((got.view(torch.int16) != ref.view(torch.int16)).sum())
    assert n == 0, 'bf16 %s: %d of %d elements differ in their bits' % (what, n, ref.numel())


def sum_close(family, what, got, terms, tol, units=None):
    """column sums `got` [C] against the float64 sum of `terms` [rows, C], in units of sum |term| per channel.  units [rows, C]: what stands for |term| where the terms
    themselves are differences of larger quantities (the train-mode BatchNorm backward, zero in exact arithmetic at M = 1): sum |units| is then the yardstick"""
    assert bool(torch.isfinite(got.detach().double()).all()), what
    t = terms.detach().double().cpu().reshape(-1, terms.shape[-1])
    u = t if units is None else units.detach().double().cpu().reshape(-1, terms.shape[-1])
    e = float(((got.detach().double().cpu() - t.sum(0)).abs() / torch.maximum(t.abs().sum(0), u.abs().sum(0)).clamp_min(1e-300)).max())
    note(family, what, e)
    assert e < tol, '%s %s: %.3e of sum |term| (tolerance %.1e)' % (family, what, e, tol)
    return e


# ---- family `stream`: norm_act.hip -------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


K_MAX_BLOCKS = 1024


def plan_rows(M, C):
    """norm_act.hip plan_rows: channel group width, groups per row, rows in flight per workgroup, workgroup size, grid, rows per workgroup"""
    vec = 4 if C % 4 == 0 else 1
    cq = C // vec
    rpi = max(256 // cq, 1)
    grid = max(1, min(_cdiv(M, rpi * 16), K_MAX_BLOCKS))
    return dict(vec=vec, cq=cq, rpi=rpi, block=cq * rpi, grid=grid, rows_per_block=_cdiv(M, grid))


def da_grid(work, block=256, cap=256 * 16):
    """common.h da_grid"""
    return max(1, min(_cdiv(work, block), cap))


def fused_dxsum(C):
    """bn_act_bwd_impl: dxsum comes out of bn_act_bwd_apply_kernel (sums of the fp32 dx BEFORE the store) when a thread keeps its channel quad; otherwise the
    stand-alone colsum_t over the STORED dx"""
    return C % 4 == 0 and 256 % (C // 4) == 0


def idle_workgroups(M, C):
    """workgroups of the row-blocked kernels whose row range starts at or past M"""
    p = plan_rows(M, C)
    return sum(1 for b in range(p['grid']) if b * p['rows_per_block'] >= M)


STREAM_FUSED, STREAM_ALONE, STREAM_VEC1 = [8, 16, 32, 64], [12, 24, 48], [3, 5, 6]
SLOPES = [-1.0, 0.0, 0.01]
STREAM_CAP = dict(c=64, m=262144 + 77)         # the 1024-workgroup cap binds: 257 rows per workgroup, workgroups 1021 ... 1023 start past M
STREAM_STRIDE = dict(c=12, m=349537)           # bn_act_fwd above one grid stride (4096 x 256 quads) with a quad that changes per iteration (stride % 3 != 0)


def stream_rows(C):
    """1 | one below and one above rpi * 16 (one workgroup / two) | 2 rpi + 1: odd, the two-rows-in-flight loop of the BatchNorm-backward sums runs once in full and
    once with its second row clamped | rpi + 3: the second row clamped for all but three row slots"""
    rpi = plan_rows(1, C)['rpi']
    return [1, rpi * 16 - 1, rpi * 16 + 1, 2 * rpi + 1, rpi + 3]


STREAM = st.fixed_dictionaries(dict(c=st.sampled_from(STREAM_FUSED + STREAM_ALONE), m=st.one_of(st.integers(1, 900), st.sampled_from([255, 257, 511, 1025, 2047, 2049])),
                                    slope=st.sampled_from(SLOPES), sd=st.integers(0, 999)))
STREAM_PINNED = [dict(c=c, m=m, slope=_cyc(SLOPES, i + j), sd=600 + 10 * i + j, fixed=True)
                 for i, c in enumerate(STREAM_FUSED + STREAM_ALONE + STREAM_VEC1) for j, m in enumerate(stream_rows(c))]
STREAM_LARGE = [dict(STREAM_CAP, slope=0.01, sd=790, fixed=True), dict(STREAM_STRIDE, slope=0.0, sd=791, fixed=True)]
# act_bwd: numel % 4 = 0 ... 3 and numel = 1, 3 (rows x channels of the pinned examples do not give these: its own list), one size above a grid stride of the quads
ACT_NUMEL = [1, 3, 4, 5, 6, 7, 1021, 1022, 1023, 1024, 4 * 256 * 4096 + 4 * 77 + 2]
UNIT_ROWS = bc.M_MIN       # (128: block_cases' fewest voxels per channel in train mode)
STREAM_BETA0 = 1.5         # beta is centred here: about 7 % of z = gamma xhat + beta is negative.  A LeakyReLU'd negative is 100 x nearer to zero than its spacing-relative
                           # neighbours and lies inside tol max|ref| of a rounding midpoint; centred at 0, half of every tensor would be left out of rne_check


def build_stream(case):
    C, M = case['c'], case['m']
    if not case.get('fixed'):
        while M * C < BAND_ELEMS:
            M += 37
    sd = 100 * case['sd']
    x = to_bf16(nrm((M, C), sd + 1) + nrm((C,), sd + 2))
    gamma = 1.0 + 0.3 * nrm((C,), sd + 3)
    gamma[1 % C] = -0.8
    beta = STREAM_BETA0 + nrm((C,), sd + 4, 0.2)
    # the statistics rows the backward is handed: those of x itself, formed in float64 and rounded to fp32 once (device and reference read the same numbers)
    x64 = x.double()
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.double() * rstd
    stats = torch.stack((mean, rstd, scale, beta.double() - mean * scale)).float()
    y = to_bf16(nrm((M, C), sd + 8) + 1.0)
    y.view(-1)[::7] = 0.0                                     # exact zeros: `y > 0` is false there
    return dict(x=x, dy=to_bf16(nrm((M, C), sd + 5)), g2=to_bf16(nrm((M, C), sd + 6)), y=y, gamma=gamma, beta=beta, rm=nrm((C,), sd + 9, 0.1),
                rv=nrm((C,), sd + 10).abs() * 0.5 + 0.5, stats=stats, slope=case['slope'], M=M, C=C)


def ref_stream(inp, dtype, decided=None):
    """Every quantity of the family in `dtype`, nothing rounded.  decided: {'y': the tested side's da_bn_act_fwd output} (None: own decisions)."""
    counts = []
    M, slope = inp['M'], inp['slope']
    x, dy, g2, yin = (inp[k].to(dtype) for k in ('x', 'dy', 'g2', 'y'))
    gamma, beta, rm, rv = (inp[k].to(dtype) for k in ('gamma', 'beta', 'rm', 'rv'))
    r = {}
    # da_bn_train_stats: batch statistics (biased variance), the affine form, running statistics with the unbiased variance (the biased one at M = 1)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma * rstd
    r['stats'] = torch.stack((mean, rstd, scale, beta - mean * scale))
    r['rm'] = (1 - MOMENTUM) * rm + MOMENTUM * mean
    r['rv'] = (1 - MOMENTUM) * rv + MOMENTUM * (var * (M / (M - 1.0)) if M > 1 else var)
    # da_bn_act_fwd / da_bn_act_bwd_dbias on the statistics rows of `inp`
    mu, rs, sc, sf = (t.to(dtype) for t in inp['stats'])
    z = x * sc + sf
    if slope < 0:
        r['y'], fac = z, torch.ones_like(z)
    else:
        # block_cases.activate's constant mask (its own z > 0 outside the guard band, the tested side's decision inside), read back from a ReLU of z
        mask = activate(z, 0.0, decided['y'].to(dtype) if decided else None, counts) != 0
        fac = torch.where(mask, torch.ones_like(z), torch.full_like(z, slope))
        r['y'] = z * fac
    dz = dy * fac
    xhat = (x - mu) * rs
    s1, s2 = dz.sum(0), (dz * xhat).sum(0)
    r['dbeta'], r['dgamma'] = s1, s2
    r['dx_train'] = sc * (dz - s1 / M - xhat * (s2 / M))
    r['dx_terms'] = sc * dz
    # the yardstick of the terms only where few rows make the result small against them (M = 1: zero); from UNIT_ROWS on the plain bounds
    small = M < UNIT_ROWS
    r['dx_unit'], r['dx_units'] = (float(r['dx_terms'].abs().max()) if small else None), (r['dx_terms'] if small else None)
    r['dx_eval'] = sc * dz
    # da_act_bwd / da_act_bwd_add_*: decided on the GIVEN tensor y, exactly
    af = torch.ones_like(yin) if slope < 0 else torch.where(yin > 0, torch.ones_like(yin), torch.full_like(yin, slope))
    r['act_dx'], r['af'] = dy * af, af
    r['add_dx'] = (dy + g2) * af
    r['band'] = counts
    return r


def oracle_colsum(t):
    """column sums the way the product forms them: fp32 over a few rows (16 here; a thread of the row-blocked kernels adds up to 17), double beyond"""
    n16 = t.shape[0] // 16 * 16
    return t[:n16].reshape(-1, 16, t.shape[1]).sum(1).double().sum(0) + t[n16:].sum(0).double()


def stream_oracle(inp):
    """the fp32 oracle that rounds where the product stores: y, dx_*, act_dx, add_dx as bf16 values; the sums from its own fp32 tensors BEFORE the store"""
    r = ref_stream(inp, torch.float32)
    out = dict(r)
    for k in ('y', 'dx_train', 'dx_eval', 'act_dx', 'add_dx'):
        out[k] = to_bf16(r[k])
        out[k + '_f32'] = r[k]
    return out


# ---- family `pool`: pool.hip --------------------------------------------------------------------------------------------------------
POOL_C, POOL_C_VEC1 = [4, 8, 12, 32], [3, 5]
POOL = st.fixed_dictionaries(dict(c=st.sampled_from(POOL_C), n=st.integers(1, 2), d=st.integers(2, 7), h=st.integers(2, 7), w=st.integers(2, 7), sd=st.integers(0, 999)))
# every parity combination of (D, H, W) at 2 ... 7, the VEC == 1 channel counts, 2 x 2 x 2 and 7 x 7 x 7
POOL_PINNED = ([dict(c=_cyc(POOL_C, i), n=1 + i % 2, d=d, h=h, w=w, sd=800 + i) for i, (d, h, w) in enumerate(
                   [(2, 2, 2), (3, 2, 2), (2, 3, 2), (2, 2, 3), (3, 5, 2), (5, 2, 7), (2, 7, 3), (7, 7, 7), (4, 6, 4), (6, 4, 6), (3, 3, 3), (4, 5, 6)])] +
               [dict(c=c, n=1 + i % 2, d=d, h=h, w=w, sd=820 + i) for i, (c, (d, h, w)) in enumerate([(3, (4, 4, 4)), (5, (3, 4, 5)), (3, (5, 7, 2)), (5, (6, 2, 4))])])


def _windows(t):
    """[N, D, H, W, C] (even sizes) -> [N, D/2, H/2, W/2, C, 8], the last axis in the kernels' scan order t = 4 dd + 2 hh + ww"""
    N, D, H, W, C = t.shape
    return t.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, D // 2, H // 2, W // 2, C, 8)


def _unwindows(w):
    N, Do, Ho, Wo, C, _ = w.shape
    return w.reshape(N, Do, Ho, Wo, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(N, 2 * Do, 2 * Ho, 2 * Wo, C)


def pool_route(x, dy, last=False):
    """MaxPool3d(2) backward on NDHWC tensors, floor mode: the window's gradient goes to its FIRST maximum in (d, h, w) order (last=True: the wrong rule), the odd
    trailing planes get zero"""
    N, D, H, W, C = x.shape
    De, He, We = D // 2 * 2, H // 2 * 2, W // 2 * 2
    win = _windows(x[:, :De, :He, :We])
    eq = win == win.max(-1, keepdim=True).values
    if last:
        pick = eq & (eq.flip(-1).cumsum(-1).flip(-1) == 1)
    else:
        pick = eq & (eq.cumsum(-1) == 1)
    dx = torch.zeros_like(x)
    dx[:, :De, :He, :We] = _unwindows(torch.where(pick, dy.unsqueeze(-1), torch.zeros((), dtype=x.dtype)))      # (+0 elsewhere, as the kernel selects it)
    return dx


def tie_counts(x):
    """(windows whose maximum occurs more than once, windows) per channel, over the even part of x [N, D, H, W, C]"""
    N, D, H, W, C = x.shape
    win = _windows(x[:, :D // 2 * 2, :H // 2 * 2, :W // 2 * 2])
    eq = win == win.max(-1, keepdim=True).values
    return int((eq.sum(-1) > 1).sum()), eq[..., 0].numel()


def up_size(d, h, w, k):
    """k = 0: factor 2;  k = 1: the non-integer factors of test_pool_and_upsample_random_shapes"""
    return (2 * d, 2 * h, 2 * w) if k == 0 else (d + 3, 2 * h - 1, w)


def build_pool(case):
    n, d, h, w, c = case['n'], case['d'], case['h'], case['w'], case['c']
    sd = 100 * case['sd']
    shape, pooled = (n, d, h, w, c), (n, d // 2, h // 2, w // 2, c)
    x = to_bf16(torch.round(1.5 * nrm(shape, sd + 1)) / 2.0)           # a coarse grid: ties inside the 2 x 2 x 2 windows
    scale = 1.0 + 0.3 * nrm((c,), sd + 5)
    scale[1 % c] = -0.8
    inp = dict(x=x, dy=to_bf16(nrm(pooled, sd + 2)), gskip=to_bf16(nrm(shape, sd + 3)), raw=to_bf16(nrm(shape, sd + 4)), scale=scale, shift=STREAM_BETA0 + nrm((c,), sd + 6, 0.2),
               slope=_cyc([0.01, 0.0, -1.0], case['sd']), dims=(n, d, h, w), c=c)
    for k in (0, 1):
        inp['up_dy%d' % k] = to_bf16(nrm((n,) + up_size(d, h, w, k) + (c,), sd + 7 + k))
    return inp


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1)


def ref_pool(inp, dtype):
    x, dy, gskip = (inp[k].to(dtype) for k in ('x', 'dy', 'gskip'))
    r = dict(y=_ndhwc(F.max_pool3d(_ncdhw(x), 2)), routed=pool_route(x, dy))
    r['dx_add'] = gskip + r['routed']
    z = inp['raw'].to(dtype) * inp['scale'].to(dtype) + inp['shift'].to(dtype)
    s = 1.0 if inp['slope'] < 0 else inp['slope']
    r['act'] = torch.maximum(z, z * s)                               # (continuous in z: no decision, no band)
    n, d, h, w = inp['dims']
    for k in (0, 1):
        leaf = x.clone().requires_grad_(True)
        up = F.interpolate(_ncdhw(leaf), size=up_size(d, h, w, k))
        up.backward(_ncdhw(inp['up_dy%d' % k].to(dtype)))
        r['up%d' % k], r['up_dx%d' % k] = _ndhwc(up.detach()), leaf.grad
    return r


# ---- family `head`: headdice.hip ------------------------------------------------------------------------------------------------------
HEAD_CH = [(16, 16), (16, 32), (64, 16), (64, 32)]
HEAD_V = [1, 105, 256, 257, 512, 693, 1025]            # below, at and just above one and two 256-voxel chunks; two chunks per workgroup of the forward at 1025
HEAD_DECLINED = [(32, 16), (16, 8), (16, 48), (48, 32)]
HEAD = st.fixed_dictionaries(dict(ch=st.sampled_from(HEAD_CH), v=st.sampled_from(HEAD_V), n=st.integers(1, 3), wide=st.booleans(), pro=st.sampled_from([None, 0.0, 0.01]),
                                  sd=st.integers(0, 999)))
HEAD_PINNED = [dict(ch=ch, v=v, n=1 + (i + j) % 3, wide=(i + j) % 2 == 0, pro=_cyc([None, 0.01, 0.0], i + j), sd=900 + 10 * i + j) for i, ch in enumerate(HEAD_CH)
               for j, v in enumerate(HEAD_V)]
HEAD_EPS = 1e-6


def build_head(case):
    """weights x 0.2 / sqrt(Cin): logits of spread about 0.4 (1 behind the prologue).  dx of a voxel scales with the probability of its label, which is log-normal in the
    logits' spread: with test_gpu_ops' x 0.5 the softmax saturates, the few undecided voxels carry a dx hundreds of times the typical one, and nearly every element
    then lies within tol max|ref| of a rounding midpoint (measured: 87 % at 1e-4, 50 % at 1e-5)"""
    (cin, c), V, N = case['ch'], case['v'], case['n']
    sd = 100 * case['sd']
    lab = torch.randint(0, c, (N, V), generator=torch.Generator().manual_seed(sd + 7))
    scale = 1.0 + 0.3 * nrm((cin,), sd + 4)
    scale[1] = -0.8
    return dict(x=to_bf16(nrm((N, V, cin), sd + 1, 2.0)), w=nrm((cin, c), sd + 2, 0.2 / cin ** 0.5), b=nrm((c,), sd + 3, 0.2), labels=lab if case['wide'] else lab.to(torch.uint8),
                scale=scale, shift=2 * STREAM_BETA0 + nrm((cin,), sd + 5, 0.2), pro=case['pro'], N=N, V=V, cin=cin, c=c)


def head_act(inp, dtype):
    """the activated input the prologue forms, unrounded: max(z, z s) (continuous: no band)"""
    z = inp['x'].to(dtype) * inp['scale'].to(dtype) + inp['shift'].to(dtype)
    return torch.maximum(z, z * inp['pro'])


def ref_head(inp, dtype, act=None):
    """loss, coef [2][N][C] (d loss / d p = coef0 [label == c] + coef1), dx (with respect to the ACTIVATED input), dW [Cin][C], db of Dice(softmax(a W + b), labels) with
    uniform class weights.  act: the stored activated input [N][V][Cin] when there is a prologue (the tested side's), else the input itself."""
    a = (act if act is not None else inp['x']).detach().to(dtype).clone().requires_grad_(True)
    w, b = inp['w'].to(dtype).clone().requires_grad_(True), inp['b'].to(dtype).clone().requires_grad_(True)
    N, V, C = inp['N'], inp['V'], inp['c']
    p = torch.softmax(a @ w + b, -1)                                               # [N][V][C]
    onehot = F.one_hot(inp['labels'].long(), C).to(dtype)
    inter, sv, tv = (p * onehot).sum(1), p.sum(1), onehot.sum(1)                   # [N][C]
    den = sv + tv + 2 * HEAD_EPS
    loss = 1 - ((2 * inter + HEAD_EPS) / den).sum() / (N * C)
    loss.backward()
    coef = torch.stack((-2.0 / den / (N * C), (2 * inter + HEAD_EPS) / den ** 2 / (N * C))).detach()
    return dict(loss=float(loss.detach().double()), coef=_f64(coef), dx=_f64(a.grad), dw=_f64(w.grad), db=_f64(b.grad))


# ---- family `conv3`: the six masked twins of conv3d.hip --------------------------------------------------------------------------------
# bf16_mask: one bit per activation argument in signature order, an absent in2 / dx2 included (ops.call_act counts every A(...) it is handed):
#   fwd, fwd_bnstats, fwd_pro: in1 1, in2 2, out 4;   dgrad: dy 1, dx1 2, dx2 4;   wgrad, wgrad_pro: in1 1, in2 2, dy 4
def c3_want(entry, c2):
    """the mask of "every tensor bf16" """
    return (1 | 2 | (4 if c2 else 0)) if entry == 'dgrad' else (1 | (2 if c2 else 0) | 4)


def c3_route(entry, c1, c2, cout, stride, mask, dbias=False, pro=False):
    """conv3d.hip da_conv3d_k3_{fwd, dgrad, wgrad}_bf16 in matrix mode 1, restated: 'thin' | 'fewcin' | 'flow' | 's2' | 'mfma' | None (DA_ERR_UNSUPPORTED)"""
    cin, want = c1 + c2, c3_want(entry, c2)
    if entry == 'fwd':
        inm = 1 | (2 if c2 else 0)
        if not pro and stride == 1 and (mask & inm) in (0, inm) and not rc.mfma_fwd_supported(c1, c2, cout, 1) and rc.thin_supported(c1, c2, cout, 1):
            return 'thin'
        if mask & want != want:
            return None
        if stride == 2:
            return 's2' if rc.s2_supported(c1, c2, cout) and not pro else None
        return 'mfma' if rc.mfma_fwd_supported(c1, c2, cout, 1) else None
    if entry == 'dgrad':
        outm = 2 | (4 if c2 else 0)
        if stride == 1 and (mask & outm) in (0, outm) and not rc.mfma_fwd_supported(cout, 0, cin, 1, c1, c2) and rc.thin_supported(cout, 0, cin, 1):
            return 'thin'
        if mask & want != want:
            return None
        if stride == 2:      # (da_conv3_s2_dgrad stages dY in 16-channel chunks)
            return 's2' if rc.s2_supported(c1, c2, cout) and cout % 16 == 0 else None
        return 'mfma' if rc.mfma_fwd_supported(cout, 0, cin, 1, c1, c2) else None
    inm = 1 | (2 if c2 else 0)
    if dbias:
        return None
    if not pro and stride == 1 and mask & inm == 0 and mask & 4 and rc.fewcin_wgrad_supported(c1, c2, cout, 1):
        return 'fewcin'
    if not pro and stride == 1 and mask & inm == inm and not mask & 4 and rc.flow_wgrad_supported(c1, c2, cout, 1):
        return 'flow'
    if mask & want != want:
        return None
    if stride == 2:
        return 's2' if rc.s2_supported(c1, c2, cout) and not pro else None
    # da_conv3_mfma_wgrad on bf16 tensors: the matrix kernels proper
    ok = rc.mfma_wgrad_supported(c1, c2, cout, 1) and rc.pick_ck(c1, c2) != 0 and cout % 4 == 0 and cout > 4 and not rc.smallcin_ok(c1, c2, cout, 1)
    return 'mfma' if ok and not rc.fewcin_wgrad_supported(c1, c2, cout, 1) else None


# smaller than the 4 x 8 x 16 output tile in every axis | exactly one tile | one past a tile in each axis | N = 2
C3_SHAPES = [(1, 3, 5, 9), (1, 4, 8, 16), (1, 5, 9, 17), (2, 4, 8, 16)]
C3_CH = bc.CH16 + bc.CH8                    # pick_ck = 16 | 8, with and without a second input
C3_COUTS = [8, 16, 32, 12]
C3_PRO = ['in1', 'both', 'stats']
C3_S2_CH, C3_S2_COUT = [16, 32], [8, 16, 32, 64]
C3_S2_SHAPES = [(1, 3, 5, 9), (1, 5, 9, 17), (2, 7, 7, 11), (1, 9, 15, 31)]
C3_FIRST_CH, C3_FLOW_CH = [(1, 0), (1, 1), (2, 0)], [(8, 16), (16, 16), (16, 0), (4, 12), (12, 0), (4, 0), (16, 8)]


def _c3(kind, ch, cout, dims, i, stride=1, **kw):
    return dict(dict(kind=kind, ch=ch, cout=cout, dims=dims, stride=stride, slope=_cyc(SLOPES, i), pro=_cyc(C3_PRO, i), raw_w=False, sd=1000 + i), **kw)


C3 = st.one_of(
    st.fixed_dictionaries(dict(kind=st.just('mfma'), ch=st.sampled_from(C3_CH), cout=st.sampled_from(C3_COUTS), dims=st.sampled_from(C3_SHAPES), stride=st.just(1),
                               slope=st.sampled_from(SLOPES), pro=st.sampled_from(C3_PRO), raw_w=st.just(False), sd=st.integers(0, 999))),
    st.fixed_dictionaries(dict(kind=st.just('s2'), ch=st.sampled_from([(c, 0) for c in C3_S2_CH]), cout=st.sampled_from(C3_S2_COUT), dims=st.sampled_from(C3_S2_SHAPES),
                               stride=st.just(2), slope=st.sampled_from(SLOPES), pro=st.none(), raw_w=st.just(False), sd=st.integers(0, 999))),
    st.fixed_dictionaries(dict(kind=st.just('first'), ch=st.sampled_from(C3_FIRST_CH), cout=st.sampled_from([4, 8, 12, 16]), dims=st.sampled_from(C3_SHAPES), stride=st.just(1),
                               slope=st.sampled_from(SLOPES), pro=st.none(), raw_w=st.just(False), sd=st.integers(0, 999))),
    st.fixed_dictionaries(dict(kind=st.just('flow'), ch=st.sampled_from(C3_FLOW_CH), cout=st.sampled_from([1, 2, 3]), dims=st.sampled_from(C3_SHAPES), stride=st.just(1),
                               slope=st.just(-1.0), pro=st.none(), raw_w=st.just(False), sd=st.integers(0, 999))))
# `want`: the routes (fwd, dgrad, wgrad) each pinned example is there for, written down by hand; check_c3_pinned compares them with c3_route
def _m3(ch, cout):
    """the all-bf16 matrix route; its data gradient declines at Cout = 12 (dY, its input, has no 8- or 16-channel chunking) and for the split (8, 16) (the first part of a
    split output has to be a multiple of 16)"""
    return ('mfma', None if cout == 12 or ch == (8, 16) else 'mfma', 'mfma')


C3_PINNED = ([_c3('mfma', ch, _cyc(C3_COUTS, i), _cyc(C3_SHAPES, i), i, want=_m3(ch, _cyc(C3_COUTS, i))) for i, ch in enumerate(C3_CH)] +
             [_c3('mfma', _cyc(C3_CH, i + 2), co, _cyc(C3_SHAPES, i + 1), 10 + i, want=_m3(_cyc(C3_CH, i + 2), co)) for i, co in enumerate(C3_COUTS)] +
             [_c3('mfma', (16, 16), 16, s, 20 + i, want=_m3((16, 16), 16)) for i, s in enumerate(C3_SHAPES)] +
             # unrounded weights: the reference rounds them to nearest even, as the bf16 matrix mode does with every operand
             [_c3('mfma', (16, 0), 16, (1, 5, 9, 17), 30, raw_w=True, want=_m3((16, 0), 16)), _c3('s2', (16, 0), 16, (1, 5, 9, 17), 31, stride=2, raw_w=True, want=('s2', 's2', 's2'))] +
             [_c3('s2', (c, 0), co, _cyc(C3_S2_SHAPES, i + j), 40 + 4 * i + j, stride=2, want=('s2', 's2' if co % 16 == 0 else None, 's2'))
              for i, c in enumerate(C3_S2_CH) for j, co in enumerate(C3_S2_COUT)] +
             [_c3('first', ch, co, _cyc(C3_SHAPES, i + j), 60 + 4 * i + j, want=('thin' if co >= 8 else None, 'thin' if co in (8, 16) else None, 'fewcin'))
              for i, ch in enumerate(C3_FIRST_CH[:2]) for j, co in enumerate([4, 8, 12, 16])] +
             [_c3('flow', ch, _cyc([3, 1, 2], i), _cyc(C3_SHAPES, i), 80 + i, slope=-1.0, want=('thin' if ch[0] % 8 == 0 and ch[1] % 8 == 0 else None, 'thin' if sum(ch) >= 8 else None, 'flow'))
              for i, ch in enumerate(C3_FLOW_CH)])


def c3_masks(case):
    """the masks the product sends for this kind: (fwd, dgrad, wgrad)"""
    c2 = case['ch'][1]
    inm = 1 | (2 if c2 else 0)
    if case['kind'] == 'first':      # fp32 network inputs -> bf16
        return 4, 1, 4
    if case['kind'] == 'flow':       # bf16 -> the fp32 displacement field
        return inm, 2 | (4 if c2 else 0), inm
    return c3_want('fwd', c2), c3_want('dgrad', c2), c3_want('wgrad', c2)


def c3_routes(case):
    (c1, c2), cout, s = case['ch'], case['cout'], case['stride']
    mf, md, mw = c3_masks(case)
    return c3_route('fwd', c1, c2, cout, s, mf), c3_route('dgrad', c1, c2, cout, s, md), c3_route('wgrad', c1, c2, cout, s, mw)


def check_c3_pinned():
    for c in C3_PINNED:
        assert c3_routes(c) == c['want'], (c, c3_routes(c))


def build_conv3(case):
    (c1, c2), cout, (n, d, h, w), s = case['ch'], case['cout'], case['dims'], case['stride']
    sd, cin = 100 * case['sd'], c1 + c2
    od = tuple((v - 1) // s + 1 for v in (d, h, w))
    wt = nrm((cout, cin, 3, 3, 3), sd, 0.2)
    sigma = 0.2 * (27 * cin) ** 0.5
    # an activated output is centred 1.5 standard deviations above its kink (see STREAM_BETA0)
    b = nrm((cout,), sd + 1, 0.1) + (1.5 * sigma if case['slope'] >= 0 else 0.0)
    inp = dict(x1=to_bf16(nrm((n, c1, d, h, w), sd + 10)), x2=to_bf16(nrm((n, c2, d, h, w), sd + 11)) if c2 else None, w=wt if case['raw_w'] else to_bf16(wt), b=b,
               dy=to_bf16(nrm((n, cout) + od, sd + 12)), slope=case['slope'], stride=s, dims=(n, d, h, w), odims=od, c1=c1, c2=c2, cout=cout, sigma=sigma)
    for i, c in ((1, c1), (2, c2)):
        if c:
            scale = 1.0 + 0.3 * nrm((c,), sd + 20 + i)
            scale[1 % c] = -0.8
            inp['scale%d' % i], inp['shift%d' % i] = scale, STREAM_BETA0 + nrm((c,), sd + 30 + i, 0.2)
    return inp


def ref_conv3(inp, dtype, decided=None, x1=None, x2=None, slope=None):
    """z (the conv result, nothing rounded), y = act(z), and the gradients of the LINEAR convolution for the output gradient dy: dx1, dx2, dw.
    x1 / x2: other inputs (the stored activated tensors behind a prologue).  decided: the tested side's activated output."""
    counts = []
    slope = inp['slope'] if slope is None else slope
    a1 = (inp['x1'] if x1 is None else x1).detach().to(dtype).clone().requires_grad_(True)
    a2 = (inp['x2'] if x2 is None else x2).detach().to(dtype).clone().requires_grad_(True) if inp['c2'] else None
    w = rne(inp['w']).to(dtype).requires_grad_(True)          # (the bf16 matrix mode rounds both operands; a no-op unless raw_w)
    z = F.conv3d(torch.cat((a1, a2), 1) if a2 is not None else a1, w, inp['b'].to(dtype), stride=inp['stride'], padding=1)
    z.backward(inp['dy'].to(dtype))
    zd = z.detach()
    y = zd if slope < 0 else activate(zd, slope, decided, counts)
    return dict(z=_f64(zd), y=_f64(y), dx1=_f64(a1.grad), dx2=_f64(a2.grad) if a2 is not None else None, dw=_f64(w.grad), band=counts)


def pro_act(inp, i, slope, dtype):
    """the activated input a prologue forms from raw input i, unrounded: max(z, z s), s = 1 for no activation"""
    x = inp['x%d' % i].to(dtype)
    z = x * inp['scale%d' % i].to(dtype).view(1, -1, 1, 1, 1) + inp['shift%d' % i].to(dtype).view(1, -1, 1, 1, 1)
    return torch.maximum(z, z * (1.0 if slope < 0 else slope))


def c3_tol(kind):
    """(y, dx, dw) tolerances: the matrix route's, or the registration-net routes' one figure"""
    t = TOL['conv3']
    return dict(y=t['y'], dx=t['dx'], dw=t['dw']) if kind == 'mfma' else dict(y=t['thin'], dx=t['thin'], dw=t['thin'])


def c3_stored(case):
    """which of (y, dx) the product stores as bf16 for this kind"""
    return dict(y=case['kind'] != 'flow', dx=case['kind'] != 'first')


def claimed():
    """the `_bf16` entry points this module's families test entry by entry (the ledger of tests/test_bf16_reference.py)"""
    return {'stream': ['da_bn_train_stats', 'da_bn_act_fwd', 'da_bn_act_bwd_dbias', 'da_act_bwd', 'da_act_bwd_add_dbias', 'da_act_bwd_add_partial', 'da_colsum'],
            'pool': ['da_maxpool2_fwd', 'da_maxpool2_fwd_pro', 'da_maxpool2_bwd', 'da_maxpool2_bwd_add', 'da_upsample_nearest_fwd', 'da_upsample_nearest_bwd'],
            'head': ['da_head_dice_fwd', 'da_head_dice_bwd'],
            'conv3': ['da_conv3d_k3_fwd', 'da_conv3d_k3_fwd_bnstats', 'da_conv3d_k3_fwd_pro', 'da_conv3d_k3_wgrad_pro', 'da_conv3d_k3_dgrad', 'da_conv3d_k3_wgrad']}


# family 4 of tests/pointwise_cases.py (test_gpu_pointwise_shapes.py test_bf16_twins)
POINTWISE_CLAIMED = ['da_deconv_k2s2_fwd', 'da_deconv_k2s2_fwd_bnstats', 'da_deconv_k2s2_dgrad', 'da_deconv_k2s2_wgrad', 'da_conv1x1_fwd', 'da_conv1x1_fwd_pro', 'da_conv1x1_dgrad',
                     'da_conv1x1_wgrad', 'da_conv1x1_wgrad_pro']
