"""Shared by tests/test_gpu_regconv_shapes.py (the registration net's convolution kernels -- conv3d_s2n.hip, conv3d_up2.hip, conv3d_flowmm.hip,
conv3d_flow.hip and the thin / small-Cin kernels of conv3d_mfma.hip -- through ops.Conv3dK3Fn against float64) and tests/test_regconv_reference.py (F.conv3d
in fp32 on torch-CPU against float64 on the same examples, no GPU): hypothesis strategies, pinned examples that reach every launcher branch by construction,
builders, the float64 reference, the launchers' route predicates restated in Python, CEIL and TOL.

Four families, each through loss_cases.run_cases (seed 160950: the pinned examples first, then 60 derandomised examples, at least 54 compared to the end):
  'stride2'  stride-2 conv + activation, one input          (voxel_morph.py encoder)
  'up2'      conv(nearest-x2(cat(a, b))) + activation       (decoder; the folded route, and UpsampleNearestFn + Conv3dK3Fn on the same inputs)
  'flow'     Cout 1 ... 4, stride 1                         (FlowConv 24 -> 3 and its neighbours)
  'first'    Cin 1 ... 4, stride 1                          (first layers; the data gradient is asked for although training never does)
Every example runs in matrix mode 'fp32_split' (the shipped route) and 'fp32', both against float64.

Reference: F.conv3d(cat(x1, x2), w, b, stride, padding=1) in float64 on the widened fp32 inputs, F.interpolate(scale_factor=2, mode='nearest') in front for
'up2', then the activation; gradients by autograd with a drawn output gradient (fork: one per alias, the reference adds the two).  The ReLU / LeakyReLU kink is
block_cases' rule: a constant mask from the float64 z outside the guard band G max|z|, the tested side's decision inside it, at most 0.1 % of a tensor and 64
elements there (check_band), the forward comparison unmasked.  Drawn examples with an activation are widened in W until the output has BAND_ELEMS elements and
narrowed until it has at most BAND_ELEMS_MAX.  Values: block_cases.nrm draws, weights x 0.2, bias x 0.1, the output gradient N(G_MEAN, 1) (see G_MEAN).

Routes.  The C ABI does not show which kernel ran, so the launchers' predicates are restated below, each under the name of the function it restates;
`reached(case, mode)` gives the route of the forward, the data gradient and the weight gradient and their tile / slab / grid counts, and every pinned example
carries in `want` what it is meant to reach (written down by hand, not computed): check_pinned() compares the two, so a pinned shape that stops reaching its
branch after a launcher change fails instead of silently testing something else.

Measuring: with DA_REGCONV_SHAPES_REPORT=<path> set, run_cases writes the worst distance so far per family, mode and quantity (and the case that gave it) to
that JSON file; the table in test_gpu_regconv_shapes.py was filled from it.

Plain module, no fixtures, no pytest settings."""
import json
import os

import torch
import torch.nn.functional as F
from hypothesis import strategies as st

import loss_cases as lc
from loss_cases import _cyc, _f64, _leaf, close, dist, note      # noqa: F401  (re-exported for the two test files)
from block_cases import activate, check_band, G, BAND_ELEMS, nrm  # noqa: F401  (the guard-band rule is block_cases', not re-implemented)

FAMILIES = ('stride2', 'up2', 'flow', 'first')
MODES = ('fp32_split', 'fp32')
QUANTITIES = ('out', 'dx', 'dw', 'db')


def run_cases(strategy, body, pinned=()):
    """loss_cases.run_cases (seed, example count, pinned examples first, the 90 % assertion) + this module's report."""
    ran = lc.run_cases(strategy, body, pinned)
    write_report()
    return ran


def write_report():
    path = os.environ.get('DA_REGCONV_SHAPES_REPORT')
    if path:
        with open(path, 'w') as f:
            json.dump({k: v for k, v in lc.WORST.items() if any(w in FAMILIES for w in k.split('/')[0].split())}, f, indent=1, sort_keys=True)


# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# CEIL: what the existing tests of these kernels assert -- 1e-5 on every tensor in split mode (test_native_stride2_split_kernels_are_fp32_accurate,
# test_folded_upsampling_conv_is_fp32_accurate, test_split_mode_is_fp32_accurate), 1e-4 in fp32 mode (check()'s TOL in tests/test_gpu_ops.py).
# TOL: what both new files assert, never above CEIL.  Rule (tests/loss_cases.py): where max(4 x device worst, 8 x fp32-CPU-oracle worst) is more than 10 x
# below the ceiling, that value rounded up to two digits; otherwise the ceiling.  The figures are in the table of tests/test_gpu_regconv_shapes.py.
CEIL = {f: {'fp32_split': dict.fromkeys(QUANTITIES, 1e-5), 'fp32': dict.fromkeys(QUANTITIES, 1e-4)} for f in FAMILIES}
# Split mode: every max(4 x device, 8 x oracle) is within 10 x of the 1e-5 ceiling (the fp32 oracle itself is 0.4 ... 2.1e-6 from float64 on these examples), so the
# ceiling stays throughout.  fp32 mode (ceiling 1e-4): the measured bound wherever it is below 1e-5.
_SPLIT = dict.fromkeys(QUANTITIES, 1e-5)
TOL = {
    'stride2': {'fp32_split': dict(_SPLIT), 'fp32': {'out': 6.3e-6, 'dx': 6.3e-6, 'dw': 1e-4, 'db': 1e-4}},
    # ('up2' fp32: the materialised route, UpsampleNearestFn + Conv3dK3Fn -- the folded kernels exist in split mode only)
    'up2': {'fp32_split': dict(_SPLIT), 'fp32': {'out': 7.8e-6, 'dx': 3.5e-6, 'dw': 1e-4, 'db': 1e-4}},
    'flow': {'fp32_split': dict(_SPLIT), 'fp32': {'out': 1e-4, 'dx': 3.3e-6, 'dw': 1e-4, 'db': 5.4e-6}},
    'first': {'fp32_split': dict(_SPLIT), 'fp32': {'out': 3.7e-6, 'dx': 6.8e-6, 'dw': 1e-4, 'db': 1e-4}},
}
assert all(TOL[f][m][q] <= CEIL[f][m][q] for f in FAMILIES for m in MODES for q in QUANTITIES)


# ---- the launchers' predicates, restated -----------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def pick_ck(c1, c2):
    """conv3d_mfma.hip pick_ck"""
    if (c1 + c2) % 16 == 0 and c1 % 16 == 0:
        return 16
    if (c1 + c2) % 8 == 0 and c1 % 8 == 0:
        return 8
    return 0


def smallcin_ok(c1, c2, cout, stride):
    """conv3d_mfma.hip smallcin_ok"""
    return stride == 1 and c1 + c2 <= 4 and cout <= 32


def thin_supported(c1, c2, cout, stride):
    """conv3d_mfma.hip da_conv3_thin_supported"""
    cin = c1 + c2
    if stride != 1:
        return False
    if cout <= 4 and 8 <= cin <= 64 and c1 % 8 == 0 and c2 % 8 == 0:
        return True
    return cin <= 4 and 8 <= cout <= 32


def mfma_fwd_supported(c1, c2, cout, stride, cs1=-1, cs2=0):
    """conv3d_mfma.hip da_conv3_mfma_fwd_supported"""
    if stride != 1 or pick_ck(c1, c2) == 0 or cout < 8 or cout % 4 != 0:
        return False
    if cs1 < 0:
        cs1, cs2 = cout, 0
    if cs2 > 0 and (cs1 % 16 != 0 or cs2 % 4 != 0):
        return False
    return cs1 % 4 == 0


def mfma_wgrad_supported(c1, c2, cout, stride):
    """conv3d_mfma.hip da_conv3_mfma_wgrad_supported"""
    if smallcin_ok(c1, c2, cout, stride):
        return True
    if stride != 1 or pick_ck(c1, c2) == 0:
        return False
    return not (cout % 4 != 0 and cout > 16)


def s2_supported(c1, c2, cout):
    """conv3d_s2.hip da_conv3_s2_supported"""
    return c2 == 0 and c1 % 16 == 0 and c1 <= 32 and cout >= 8 and cout % 4 == 0


def s2n_supported(cin, cout, n, d, h, w):
    """conv3d_s2n.hip da_conv3_s2n_supported"""
    if cin % 16 != 0 or cin > 32 or cout % 32 != 0 or cout > 64:
        return False
    return d * h * w * cin * 4 < (1 << 32) and n * d * h * w < (1 << 31)


def s2n_wgrad_slabs(ntiles, nchunks, ngroups):
    """conv3d_s2n.hip s2n_wgrad_slabs"""
    s = 256 // (nchunks * ngroups)
    s = max(s // 8 * 8, 8)
    return max(min(s, ntiles), 1)


def upconv_supported(c1, c2, cout, mode):
    """conv3d_up2.hip da_upconv3d_k3_supported"""
    if mode != 'fp32_split':
        return False
    if c1 <= 0 or c2 < 0 or c1 % 8 or c2 % 8 or (c2 > 0 and c1 % 16) or c1 + c2 > 64:
        return False
    return not (cout % 8 or cout <= 0 or cout > 32)


def up_wgrad_slabs(ntiles, nchunks):
    """conv3d_up2.hip up_wgrad_slabs"""
    s = 512 // (nchunks * 8)
    s = max(s // 8 * 8, 8)
    return max(min(s, ntiles), 1)


def up_dgrad_ntiles(cin):
    """conv3d_up2.hip da_upconv3d_k3_dgrad: N-tiles of the data gradient, three rounded to four"""
    ntn = _cdiv(cin, 16)
    return 4 if ntn == 3 else ntn


FLOWMM_CH = [(8, 16), (16, 16), (16, 0), (8, 8), (8, 0)]


def flowmm_supported(c1, c2, cout, mode):
    """conv3d_flowmm.hip da_conv3_flowmm_supported (the sizes of this file are far below its 32-bit limits)"""
    return mode == 'fp32_split' and 1 <= cout <= 3 and (c1, c2) in FLOWMM_CH


def flow_wgrad_supported(c1, c2, cout, stride):
    """conv3d_flow.hip da_conv3_flow_wgrad_supported"""
    return stride == 1 and 1 <= cout <= 3 and c1 % 4 == 0 and c2 % 4 == 0 and c1 <= 16 and c2 <= 16 and c1 + c2 >= 4


def fewcin_wgrad_supported(c1, c2, cout, stride):
    """conv3d_flow.hip da_conv3_fewcin_wgrad_supported"""
    return stride == 1 and c1 >= 1 and c2 >= 0 and c1 + c2 <= 2 and cout % 4 == 0 and 4 <= cout <= 16


def fewcin_valu(c1, c2, cout):
    """conv3d_flow.hip da_conv3_fewcin_wgrad: the condition under which fewcin_valu_launch runs (fp32 tensors; one input channel only)"""
    return cout in (8, 16) and (c2 == 0 or (c1 == 1 and c2 == 1)) and c1 + c2 == 1


def xcd_items(n, grid, b, sub=0, nsub=1):
    """common.h da_xcd_items: the items workgroup b of `grid` (wave `sub` of `nsub`) walks"""
    if grid % 8:
        return list(range(b * nsub + sub, n, grid * nsub))
    x, j, J = b % 8, b // 8, grid // 8
    return list(range(n * x // 8 + j * nsub + sub, n * (x + 1) // 8, J * nsub))


def tiles_of(n, d, h, w, tile):
    return n * _cdiv(d, tile[0]) * _cdiv(h, tile[1]) * _cdiv(w, tile[2])


def persistent(ntiles, cap=512, nsub=1):
    """grid = min(ntiles, cap) workgroups over da_xcd_items: (grid, most items one workgroup / wave walks)"""
    grid = min(_cdiv(ntiles, nsub), cap)
    return grid, max(len(xcd_items(ntiles, grid, b, s, nsub)) for b in range(grid) for s in range(nsub))


S2N_TILE = UP_TILE = (2, 4, 16)      # conv3d_s2n.hip TZ, TY, TX (output voxels); conv3d_up2.hip CTZ, CTY, CTX (coarse voxels)
FLOW_SPLIT_TILE, FLOW_FP32_TILE = (2, 8, 16), (4, 8, 16)      # conv3d_flowmm.hip / conv3d_flow.hip sp:: ; conv3d_flow.hip TZ, TY, TX
VALU_YR = 33                         # conv3d_flow.hip fewcin_valu_launch
# Drawn examples with an activation: the output has at most this many elements.  An element enters the guard band with probability about 4e-5 (|z| < 1e-5 max|z|,
# max|z| about 5 sigma), so at 1.5 M elements -- 2 x 32 x 9 x 40 x 68 of the 'first' family -- 60 are expected against the cap of 64; at 500 000 it is 20.
BAND_ELEMS_MAX = 500000
# The drawn output gradient is N(G_MEAN, 1), not N(0, 1): the bias gradient is its sum over the voxels, and with one to four output channels a zero-mean sum
# of V terms is a cancelling one, |sum| about sqrt(V) of sum |term| = 0.8 V, which the comparison divides by -- the fp32 oracle's own db was 2.7e-6 from float64
# on a Cout = 1 example of 4 000 voxels, above a quarter of the ceiling.  With the mean the sum is 0.5 V and db is as well conditioned as the other tensors.
G_MEAN = 0.5


def out_dims(fam, d, h, w):
    if fam == 'stride2':
        return (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return (2 * d, 2 * h, 2 * w) if fam == 'up2' else (d, h, w)


def reached(case, mode, dims=None):
    """Routes of the three passes of ops.Conv3dK3Fn for `case` in matrix mode `mode` (da_conv3d_k3_fwd / _dgrad / _wgrad, da_conv3_s2_*, da_conv3_mfma_wgrad
    and the da_upconv3d_k3_* entries, restated) and the counts of the kernels this file is about."""
    fam, (c1, c2), cout = case['fam'], case['ch'], case['cout']
    cin = c1 + c2
    n, d, h, w = dims or (case['n'], case['d'], case['h'], case['w'])
    r = {}
    if fam == 'up2':
        ok = upconv_supported(c1, c2, cout, mode)
        r['fwd'] = r['dgrad'] = r['wgrad'] = 'up2' if ok else 'declined'
        if ok:
            t = tiles_of(n, d, h, w, UP_TILE)
            s = up_wgrad_slabs(t, cin // 8)
            r.update(tiles=t, slabs=s, walk=_cdiv(t, s), ntn=up_dgrad_ntiles(cin), nt=_cdiv(cout, 16))
        return r
    if fam == 'stride2':
        if not s2_supported(c1, c2, cout):
            route = 'direct'
        elif mode == 'fp32_split' and s2n_supported(cin, cout, n, d, h, w):
            route = 's2n'
            t = tiles_of(n, *out_dims(fam, d, h, w), S2N_TILE)
            s = s2n_wgrad_slabs(t, cin // 8, cout // 32)
            r.update(tiles=t, slabs=s, walk=_cdiv(t, s))
        else:
            route = 's2d'
        r['fwd'] = r['dgrad'] = r['wgrad'] = route
        if route == 's2d' and cout % 16 != 0:
            r['dgrad'] = 'direct'                           # da_conv3_s2_dgrad: the masked kernels stage dY in 16-channel chunks
        return r
    # stride 1
    if mfma_fwd_supported(c1, c2, cout, 1):
        r['fwd'] = 'mfma'
    elif flowmm_supported(c1, c2, cout, mode):
        r['fwd'] = 'flowmm'
    else:
        r['fwd'] = 'thin' if thin_supported(c1, c2, cout, 1) else 'direct'
    if mfma_fwd_supported(cout, 0, cin, 1, c1, c2):
        r['dgrad'] = 'mfma'
    elif flowmm_supported(c1, c2, cout, mode):
        r['dgrad'] = 'flowmm'
    else:
        r['dgrad'] = 'thin' if thin_supported(cout, 0, cin, 1) else 'direct'
    if r['fwd'] == 'flowmm':
        t = tiles_of(n, d, h, w, FLOW_SPLIT_TILE)
        g, k = persistent(t)
        r.update(tiles=t, grid=g, walk=k)
    if not mfma_wgrad_supported(c1, c2, cout, 1):
        r['wgrad'] = 'direct'
    elif fewcin_wgrad_supported(c1, c2, cout, 1):
        if fewcin_valu(c1, c2, cout):
            r['wgrad'] = 'valu'
            xw = 64 // (cin * cout // 4)
            nxs, nys = _cdiv(w, xw), _cdiv(h, VALU_YR)
            strips = n * d * nxs * nys
            g, k = persistent(strips, nsub=4)
            r.update(xw=xw, nxs=nxs, nys=nys, strips=strips, wgrid=g, wwalk=k, ragged_x=w % xw != 0, tail=(h - (nys - 1) * VALU_YR) % 3)
        else:
            # (flow_launch: the split kernel in split mode unless two window tensors are read, C2 > 0)
            r['wgrad'] = 'exchanged'
            tile = FLOW_SPLIT_TILE if (mode == 'fp32_split' and c2 == 0) else FLOW_FP32_TILE
            t = tiles_of(n, d, h, w, tile)
            g, k = persistent(t)
            r.update(wtiles=t, wgrid=g, wwalk=k)
    elif smallcin_ok(c1, c2, cout, 1):
        r['wgrad'] = 'smallcin'
    elif flow_wgrad_supported(c1, c2, cout, 1):
        r['wgrad'] = 'flow_split' if mode == 'fp32_split' else 'flow_fp32'
        t = tiles_of(n, d, h, w, FLOW_SPLIT_TILE if mode == 'fp32_split' else FLOW_FP32_TILE)
        g, k = persistent(t)
        r.update(wtiles=t, wgrid=g, wwalk=k, template=(6, c2 > 0, 16 if (c2 > 0 and c1 > 8) else 8))
    elif cout <= 4 and cin <= 32:
        r['wgrad'] = 'swapped'
    else:
        r['wgrad'] = 'generic'
    return r


def check_pinned(case):
    """Every entry of the pinned example's `want` is what the restated launchers give, in both modes."""
    dims = build_dims(case)
    for mode in MODES:
        got = reached(case, mode, dims)
        for k, v in case['want'].get(mode, {}).items():
            assert got.get(k) == v, 'pinned example no longer reaches what it names: %s %s = %r, wanted %r (%r)' % (mode, k, got.get(k), v, case)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def build_dims(case):
    """(n, d, h, w) of the input(s).  Drawn examples with an activation: W widened until the output tensor, on which the activation is decided, has BAND_ELEMS
    elements (block_cases.fit's rule), and narrowed until it has at most BAND_ELEMS_MAX; the pinned examples keep their shapes."""
    n, d, h, w = case['n'], case['d'], case['h'], case['w']
    if not case.get('fixed') and case['slope'] >= 0:
        def elems(w_):
            od = out_dims(case['fam'], d, h, w_)
            return n * case['cout'] * od[0] * od[1] * od[2]
        while elems(w) < BAND_ELEMS:
            w += 1
        while elems(w) > BAND_ELEMS_MAX and w > 1:
            w -= 1
    return n, d, h, w


# Structured values on a slab-walk shape whose tiles lie along x (tile index = x tile): slab 0 walks tile 0 and then the last tile.
#   'zero_first' / 'zero_last': the input (with the tile's halo) and the output gradient are exactly zero over that tile
#   'jump_dn' / 'jump_up': the first tile's input and output-gradient values x 2^-30 / 2^+30 (E of the staged tile 60 above / below the others':
#       'jump_up' takes the `Emin + 40` clamp on the second tile, 'jump_dn' the accumulator rescale by 2^-60)
JUMP = 30
_IN_TILE_W = {'stride2': 32, 'up2': 16}      # input voxels along x under one tile
_OUT_TILE_W = {'stride2': 16, 'up2': 32}


def _structure(case, x, g, ntx):
    kind, fam = case.get('kind'), case['fam']
    wi, wo = _IN_TILE_W[fam], _OUT_TILE_W[fam]
    if kind == 'zero_first':
        for t in x:
            t[..., :wi + (1 if fam == 'up2' else 0)] = 0.0
        for t in g:
            t[..., :wo] = 0.0
    elif kind == 'zero_last':
        for t in x:
            t[..., (ntx - 1) * wi - 1:] = 0.0
        for t in g:
            t[..., (ntx - 1) * wo:] = 0.0
    elif kind in ('jump_dn', 'jump_up'):
        f = 2.0 ** (JUMP if kind == 'jump_up' else -JUMP)
        for t in x:
            t[..., :wi] *= f
        for t in g:
            t[..., :wo] *= f


def build(case):
    """Well-conditioned fp32 CPU inputs (block_cases.nrm draws: N(0, 1) activations, N(G_MEAN, 1) output gradients, weights x 0.2, bias x 0.1)."""
    fam, (c1, c2), cout = case['fam'], case['ch'], case['cout']
    n, d, h, w = dims = build_dims(case)
    od = out_dims(fam, d, h, w)
    sd = 100 * case['sd']
    x1 = nrm((n, c1, d, h, w), sd + 10)
    x2 = nrm((n, c2, d, h, w), sd + 11) if c2 else None
    g1 = nrm((n, cout) + od, sd + 12) + G_MEAN
    g2 = nrm((n, cout) + od, sd + 13) + G_MEAN if case['fork'] else None
    if case.get('kind'):
        _structure(case, [t for t in (x1, x2) if t is not None], [t for t in (g1, g2) if t is not None], _cdiv(od[2], _OUT_TILE_W[fam]))
    return dict(fam=fam, x1=x1, x2=x2, w=nrm((cout, c1 + c2, 3, 3, 3), sd, 0.2), b=nrm((cout,), sd + 1, 0.1), g1=g1, g2=g2, stride=2 if fam == 'stride2' else 1,
                up2=fam == 'up2', slope=case['slope'], fork=case['fork'], dims=dims, kind=case.get('kind'))


def ref(inp, dtype, decided=None):
    """dict of out, dx1, dx2, dw, db in float64 (computed in `dtype`); decided: the activated output of the tested side (None: own decisions)."""
    counts = []
    x1, x2 = _leaf(inp['x1'], dtype), (_leaf(inp['x2'], dtype) if inp['x2'] is not None else None)
    w, b = _leaf(inp['w'], dtype), _leaf(inp['b'], dtype)
    x = torch.cat((x1, x2), 1) if x2 is not None else x1
    if inp['up2']:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    z = F.conv3d(x, w, b, stride=inp['stride'], padding=1)
    out = activate(z, inp['slope'], decided, counts) if inp['slope'] >= 0 else z
    g = inp['g1'].to(dtype) + (inp['g2'].to(dtype) if inp['g2'] is not None else 0)
    out.backward(g)
    zd = z.detach()
    return dict(out=_f64(out), dx1=_f64(x1.grad), dx2=_f64(x2.grad) if x2 is not None else None, dw=_f64(w.grad), db=_f64(b.grad), band=counts,
                bandmask=(zd.abs() < G * zd.abs().max()) if inp['slope'] >= 0 else None)


def same_decisions(r, out_a, out_b):
    """Do two tested sides decide alike inside the guard band of reference `r`?  (then `r` serves both)"""
    m = r['bandmask']
    return m is None or torch.equal((out_a > 0)[m], (out_b > 0)[m])


def compare(family, got, r, tol):
    for k in ('out', 'dx1', 'dx2', 'dw', 'db'):
        if r[k] is not None:
            close(family, 'dx' if k.startswith('dx') else k, got[k], r[k], tol['dx' if k.startswith('dx') else k])


def compare_jump(family, inp, got, r, tol):
    """'jump_dn' / 'jump_up' examples (no activation).  dw and db are sums over every tile: compared whole, relative to their largest entry, which the tiles
    holding the large values dominate -- the ordinary tiles for 'jump_dn'.  out and dx are local.  Beyond the reach of every staged box that can hold a voxel of
    the scaled tile (two tiles along x) they are compared as always.  Up to there the staged box mixes the two magnitudes, and what split_f16.h states for an
    element 2^15 or more below its box's largest magnitude M is an ABSOLUTE error, <= 2^-36 M per product where a kernel keeps the previous item's unit (as
    tests/test_gpu_split.py::test_split_mode_one_outlier_in_a_staged_box asserts it): |error| <= 2^-36 M sum|w| + 2^-20 sum|w||x|."""
    for k in ('dw', 'db'):
        close(family, k, got[k], r[k], tol[k])
    fam = inp['fam']
    far_o, far_i = 2 * _OUT_TILE_W[fam] + 2, 2 * _IN_TILE_W[fam] + 2
    close(family, 'out', got['out'][..., far_o:], r['out'][..., far_o:], tol['out'])
    x = torch.cat((inp['x1'], inp['x2']), 1) if inp['x2'] is not None else inp['x1']
    g = inp['g1'] + (inp['g2'] if inp['g2'] is not None else 0)
    aw = inp['w'].double().abs()
    xa, ga = x.double().abs().requires_grad_(True), g.double().abs()
    xu = F.interpolate(xa, scale_factor=2, mode='nearest') if inp['up2'] else xa
    A = F.conv3d(xu, aw, inp['b'].double().abs(), stride=inp['stride'], padding=1)
    A.backward(ga)
    Ad = xa.grad                                            # sum |w| |dy| per input element
    M = 2.0 ** JUMP * 8.0                                   # the scaled tile's largest magnitude: N(0, 1) draws stay below 8
    Mx, Mg = (M, M) if inp['kind'] == 'jump_up' else (8.0, 8.0)
    e = (got['out'].double() - r['out']).abs()[..., :far_o]
    bound = (2.0 ** -36 * Mx * aw.sum((1, 2, 3, 4)).reshape(1, -1, 1, 1, 1) + 2.0 ** -20 * A.detach())[..., :far_o]
    assert bool((e <= bound).all()), '%s out, near the scaled tile: %.3e of the bound' % (family, float((e / bound).max()))
    dx = torch.cat((got['dx1'], got['dx2']), 1) if inp['x2'] is not None else got['dx1']
    rdx = torch.cat((r['dx1'], r['dx2']), 1) if inp['x2'] is not None else r['dx1']
    for k in ('dx1', 'dx2'):
        if r[k] is not None:
            close(family, 'dx', got[k][..., far_i:], r[k][..., far_i:], tol['dx'])
    e = (dx.double() - rdx).abs()[..., :far_i]
    up = 8.0 if inp['up2'] else 1.0                         # (a coarse element collects 8 fine voxels' taps)
    bound = (2.0 ** -36 * Mg * up * aw.sum((0, 2, 3, 4)).reshape(1, -1, 1, 1, 1) + 2.0 ** -20 * Ad)[..., :far_i]
    assert bool((e <= bound).all()), '%s dx, near the scaled tile: %.3e of the bound' % (family, float((e / bound).max()))


# ---- the pinned examples ----------------------------------------------------------------------------------------------------------
def _pin(fam, ch, cout, shape, i, want, slope=None, fork=False, kind=None):
    n, d, h, w = shape
    return dict(fam=fam, ch=ch, cout=cout, n=n, d=d, h=h, w=w, slope=_cyc([0.0, 0.01, -1.0], i) if slope is None else slope, fork=fork, sd=i, kind=kind,
                fixed=True, want=want)


def _all3(route, **counts):
    return dict(fwd=route, dgrad=route, wgrad=route, **counts)


# ---- family 1, stride2 ----
S2_NATIVE, S2_MASKED = [(16, 32), (16, 64), (32, 32), (32, 64)], [(16, 8), (16, 16), (32, 24), (32, 48)]
S2_DIRECT = [(8, 16), (24, 32), (48, 8), (16, 3), (32, 5)]


def _s2n(tiles, slabs, walk):
    return {'fp32_split': _all3('s2n', tiles=tiles, slabs=slabs, walk=walk), 'fp32': _all3('s2d')}


_S2DIR = {m: _all3('direct') for m in MODES}


def _s2d(cout):
    return {m: dict(fwd='s2d', dgrad='s2d' if cout % 16 == 0 else 'direct', wgrad='s2d') for m in MODES}

STRIDE2_PINNED = [
    # a single output voxel
    _pin('stride2', (16, 0), 32, (1, 1, 1, 1), 0, _s2n(1, 1, 1)), _pin('stride2', (32, 0), 64, (1, 2, 2, 2), 1, _s2n(1, 1, 1)),
    # exactly one 2 x 4 x 16 output tile from odd and from even sizes, and one voxel over a tile on every axis
    _pin('stride2', (32, 0), 32, (1, 3, 7, 31), 2, _s2n(1, 1, 1)), _pin('stride2', (16, 0), 64, (1, 4, 8, 32), 3, _s2n(1, 1, 1)),
    _pin('stride2', (16, 0), 32, (1, 5, 9, 33), 4, _s2n(8, 8, 1), fork=True),
    # thin axes: W = 1; D = 1 with H and W large
    _pin('stride2', (32, 0), 32, (1, 9, 13, 1), 5, _s2n(6, 6, 1)), _pin('stride2', (16, 0), 32, (1, 1, 37, 70), 6, _s2n(15, 15, 1)),
    # slab walks of the native weight gradient: 36 tiles over 32 slabs; 129 and 257 tiles over 128 (a ragged x edge on the last tile); 65 over 64; N = 2 with 66
    # over 64 (65 is odd: no two equal samples give it)
    _pin('stride2', (32, 0), 64, (1, 11, 23, 127), 7, _s2n(36, 32, 2), fork=True),
    _pin('stride2', (16, 0), 32, (1, 3, 7, 16 * 2 * 129 - 1), 8, _s2n(129, 128, 2)), _pin('stride2', (16, 0), 32, (1, 3, 7, 16 * 2 * 257 - 1), 9, _s2n(257, 128, 3)),
    _pin('stride2', (32, 0), 32, (1, 3, 7, 16 * 2 * 65 - 1), 10, _s2n(65, 64, 2)), _pin('stride2', (16, 0), 64, (2, 3, 7, 16 * 2 * 33 - 1), 11, _s2n(66, 64, 2)),
    _pin('stride2', (32, 0), 32, (2, 4, 7, 16 * 2 * 33 - 3), 12, _s2n(66, 64, 2)),
] + [
    # scale bookkeeping across the two tiles slab 0 walks (tiles 0 and 128)
    _pin('stride2', (16, 0), 32, (1, 3, 7, 16 * 2 * 129 - 1), 13 + i, _s2n(129, 128, 2), slope=-1.0 if k.startswith('jump') else 0.01, kind=k)
    for i, k in enumerate(['zero_first', 'zero_last', 'jump_dn', 'jump_up'])
] + [
    # the masked space-to-depth and the direct classes, one example each
    _pin('stride2', (ci, 0), co, _cyc([(1, 5, 9, 33), (2, 4, 7, 10)], i), 20 + i, _s2d(co)) for i, (ci, co) in enumerate(S2_MASKED)
] + [
    _pin('stride2', (ci, 0), co, _cyc([(1, 5, 9, 33), (2, 4, 7, 10)], i), 30 + i, _S2DIR) for i, (ci, co) in enumerate(S2_DIRECT)
]
_S2_DRAW = [(c, 'n') for c in S2_NATIVE] * 9 + [(c, 'o') for c in S2_MASKED + S2_DIRECT] * 4      # 36 : 36 -- half of the drawn examples native
STRIDE2 = st.fixed_dictionaries(dict(cc=st.sampled_from(_S2_DRAW), n=st.integers(1, 2), d=st.integers(1, 11), h=st.integers(1, 19), w=st.integers(1, 67),
                                     slope=st.sampled_from([-1.0, 0.0, 0.01]), fork=st.booleans(), sd=st.integers(0, 999))).map(
    lambda c: dict({k: v for k, v in c.items() if k != 'cc'}, fam='stride2', ch=(c['cc'][0][0], 0), cout=c['cc'][0][1]))

# ---- family 2, up2 ----
# (C1, C2) -> N-tiles of the data gradient (da_upconv3d_k3_dgrad; three rounded to four)
UP_CLASSES = {(8, 0): 1, (16, 0): 1, (24, 0): 2, (16, 8): 2, (32, 0): 2, (16, 16): 2, (40, 0): 4, (32, 8): 4, (16, 24): 4, (32, 16): 4, (48, 0): 4,
              (56, 0): 4, (48, 8): 4, (48, 16): 4, (32, 32): 4, (64, 0): 4}
UP_COUTS = [8, 16, 24, 32]
# declined by da_upconv3d_k3_supported: asserted through the C ABI (DA_ERR_UNSUPPORTED, output untouched) and ops.upconv_supported
UP_DECLINED = [(8, 8, 16), (12, 0, 16), (64, 8, 16), (16, 0, 40), (16, 0, 12)]


def _up(tiles, slabs, walk, ntn=None, nt=None):
    d = _all3('up2', tiles=tiles, slabs=slabs, walk=walk)
    if ntn:
        d.update(ntn=ntn, nt=nt)
    return {'fp32_split': d, 'fp32': _all3('declined')}


_UP_SMALL = [((1, 3, 5, 17), 8), ((2, 2, 3, 9), 2), ((1, 1, 6, 20), 4)]      # (coarse shape, tiles)
UP2_PINNED = [
    # one example per channel class, Cout cycling over one N-tile, a half-empty second and a full second
    _pin('up2', ch, _cyc(UP_COUTS, i), _cyc(_UP_SMALL, i)[0], 100 + i,
         _up(_cyc(_UP_SMALL, i)[1], min(_cyc(_UP_SMALL, i)[1], 8 if sum(ch) >= 40 else {8: 64, 16: 32, 24: 16, 32: 16}[sum(ch)]), 1, ntn, _cyc([1, 1, 2, 2], i)))
    for i, (ch, ntn) in enumerate(UP_CLASSES.items())
] + [
    # coarse shapes: one voxel; exactly one 2 x 4 x 16 tile; one over on every axis; W = 1; N = 2 with three tiles per sample -> nslabs 1, 1, 8, 4, 6
    _pin('up2', (32, 32), 32, (1, 1, 1, 1), 120, _up(1, 1, 1)), _pin('up2', (16, 0), 16, (1, 2, 4, 16), 121, _up(1, 1, 1), fork=True),
    _pin('up2', (16, 16), 24, (1, 3, 5, 17), 122, _up(8, 8, 1)), _pin('up2', (32, 16), 16, (1, 4, 7, 1), 123, _up(4, 4, 1)),
    _pin('up2', (8, 0), 8, (2, 2, 4, 48), 124, _up(6, 6, 1)),
    # nslabs 3, 5 (up_wgrad_reduce_kernel: the tail alone, the four-at-a-time body + one)
    _pin('up2', (24, 0), 16, (1, 2, 4, 48), 125, _up(3, 3, 1)), _pin('up2', (40, 0), 32, (1, 2, 4, 80), 126, _up(5, 5, 1)),
    # slab walks: Cin = 64 with 9 and 17 tiles over 8 slabs, 48 with 9, 32 with 17 over 16, 8 with 65 over 64
    _pin('up2', (32, 32), 32, (1, 2, 4, 16 * 9 - 3), 127, _up(9, 8, 2), fork=True), _pin('up2', (64, 0), 16, (1, 2, 3, 16 * 17 - 1), 128, _up(17, 8, 3)),
    _pin('up2', (32, 16), 24, (1, 1, 4, 16 * 9), 129, _up(9, 8, 2)), _pin('up2', (16, 16), 8, (1, 2, 4, 16 * 17 - 5), 130, _up(17, 16, 2)),
    _pin('up2', (8, 0), 8, (1, 1, 2, 16 * 65 - 2), 131, _up(65, 64, 2)),
] + [
    _pin('up2', (32, 32), 16, (1, 2, 4, 16 * 9 - 3), 132 + i, _up(9, 8, 2), slope=-1.0 if k.startswith('jump') else 0.0, kind=k)
    for i, k in enumerate(['zero_first', 'zero_last', 'jump_dn', 'jump_up'])
]
UP2 = st.fixed_dictionaries(dict(ch=st.sampled_from(sorted(UP_CLASSES)), cout=st.sampled_from(UP_COUTS), n=st.integers(1, 2), d=st.integers(1, 6), h=st.integers(1, 10),
                                 w=st.integers(1, 35), slope=st.sampled_from([-1.0, 0.0, 0.01]), fork=st.booleans(), sd=st.integers(0, 999))).map(
    lambda c: dict(c, fam='up2'))

# ---- family 3, flow ----
FLOW_WGRAD_CH = [(8, 0), (16, 0), (8, 8), (16, 16), (8, 16), (16, 8)]
FLOW_CH = FLOWMM_CH + [(16, 8), (24, 0), (32, 0), (32, 32), (12, 0)]
_FLOW_SHAPE = (1, 5, 9, 18)                                  # split tile 2 x 8 x 16: 3 x 2 x 2 = 12 tiles; fp32 tile 4 x 8 x 16: 8
_FLOW_TEMPLATE = {(8, 0): (6, False, 8), (16, 0): (6, False, 8), (8, 8): (6, True, 8), (8, 16): (6, True, 8), (16, 16): (6, True, 16), (16, 8): (6, True, 16)}


def _flow(ch, cout, split_tiles=None, fp32_tiles=None, walk=(None, None)):
    """the flow family's table: forward / data gradient flowmm (split mode, the five classes, Cout <= 3) else thin; the weight gradient's kernel per mode"""
    mm, wg = ch in FLOWMM_CH and cout <= 3, ch in FLOW_WGRAD_CH and cout <= 3
    w = {}
    for mode, t, k in (('fp32_split', split_tiles, walk[0]), ('fp32', fp32_tiles, walk[1])):
        sp = mode == 'fp32_split'
        # (the data gradient of 32 + 32 -> Cout is a thin conv Cout -> 64: da_conv3_thin_supported stops at 32 outputs, the direct kernel runs)
        d = dict(fwd='flowmm' if (mm and sp) else 'thin', dgrad='flowmm' if (mm and sp) else ('thin' if sum(ch) <= 32 else 'direct'))
        d['wgrad'] = ('flow_split' if sp else 'flow_fp32') if wg else ('generic' if sum(ch) > 32 else 'swapped')
        if wg:
            d['template'] = _FLOW_TEMPLATE[ch]
        if t is not None:
            if mm and sp:
                d.update(tiles=t, grid=min(t, 512), walk=k)
            if wg:
                d.update(wtiles=t, wgrid=min(t, 512), wwalk=k)
        w[mode] = d
    return w


# split-tile count -> (shape, fp32-tile count, most tiles one workgroup walks: split, fp32)
FLOW_TILE_SHAPES = {1: ((1, 2, 8, 16), 1, 1, 1), 7: ((1, 2, 8, 109), 7, 1, 1), 8: ((1, 4, 15, 31), 4, 1, 1), 9: ((1, 2, 17, 33), 9, 1, 1), 16: ((2, 4, 16, 32), 8, 1, 1),
                    17: ((1, 2, 8, 267), 17, 1, 1), 49: ((1, 13, 49, 15), 28, 1, 1), 64: ((1, 8, 32, 64), 32, 1, 1), 65: ((1, 10, 100, 13), 39, 1, 1),
                    513: ((1, 6, 24, 905), 342, 2, 1), 1025: ((1, 9, 2, 3273), 615, 3, 2)}
FLOW_PINNED = [
    # all fifteen flowmm classes and all eighteen flow-wgrad classes at 5 x 9 x 18 (Cout 1 ... 3 over the six weight-gradient classes covers both)
    _pin('flow', ch, co, _FLOW_SHAPE, 200 + 3 * i + co, _flow(ch, co, 12, 8, (1, 1)), slope=_cyc([-1.0, 0.0], i + co), fork=(i + co) % 5 == 0)
    for i, ch in enumerate(FLOW_WGRAD_CH) for co in (1, 2, 3)
] + [
    # the thin / swapped / generic / direct neighbours
    _pin('flow', (8, 16), 4, _FLOW_SHAPE, 230, _flow((8, 16), 4), slope=-1.0), _pin('flow', (24, 0), 3, _FLOW_SHAPE, 231, _flow((24, 0), 3), slope=0.0),
    _pin('flow', (32, 0), 2, _FLOW_SHAPE, 232, _flow((32, 0), 2), slope=-1.0), _pin('flow', (32, 32), 3, _FLOW_SHAPE, 233, _flow((32, 32), 3), slope=-1.0),
    _pin('flow', (12, 0), 3, _FLOW_SHAPE, 234, {m: dict(fwd='direct', dgrad='thin', wgrad='direct') for m in MODES}, slope=-1.0),
] + [
    # tile counts of the persistent grids on 8 + 16 -> 3
    _pin('flow', (8, 16), 3, shape, 240 + i, _flow((8, 16), 3, t, tf, (ks, kf)), slope=_cyc([-1.0, 0.0], i))
    for i, (t, (shape, tf, ks, kf)) in enumerate(FLOW_TILE_SHAPES.items())
]
FLOW = st.fixed_dictionaries(dict(ch=st.sampled_from(FLOW_CH), cout=st.integers(1, 4), n=st.integers(1, 2), d=st.integers(1, 9), h=st.integers(1, 19), w=st.integers(1, 35),
                                  slope=st.sampled_from([-1.0, 0.0]), fork=st.booleans(), sd=st.integers(0, 999))).map(lambda c: dict(c, fam='flow'))

# ---- family 4, first ----
FIRST_CH = [(1, 0), (2, 0), (1, 1), (3, 0), (4, 0), (2, 2)]
FIRST_COUTS = [4, 8, 12, 16, 24, 32]


def _valu(cout, **counts):
    return {m: dict(fwd='thin', dgrad='thin', wgrad='valu', xw=256 // cout, **counts) for m in MODES}


def _exch(ch, cout, split_tiles, fp32_tiles, walk=(1, 1)):
    w = {}
    for mode, t, k in (('fp32_split', split_tiles if ch[1] == 0 else fp32_tiles, walk[0] if ch[1] == 0 else walk[1]), ('fp32', fp32_tiles, walk[1])):
        w[mode] = dict(fwd='thin' if cout >= 8 else 'direct', wgrad='exchanged', wtiles=t, wgrid=min(t, 512), wwalk=k)
    return w


FIRST_PINNED = [
    # the VALU kernel (1 -> 8: XW = 32; 1 -> 16: XW = 16).  H = 33, 34, 66, 67: one strip exactly; a second of 1 row; two strips; a third of 1 row -- and the
    # `yb += 3` rotation's tail of 0, 1, 0, 1 rows; 35 and 68: a tail of 2
    _pin('first', (1, 0), co, (1, 2, hh, 5), 300 + i, _valu(co, nys=nys, tail=tail, nxs=1, strips=2 * nys))
    for i, (co, (hh, nys, tail)) in enumerate((co, t) for co in (8, 16) for t in ((33, 1, 0), (34, 2, 1), (66, 2, 0), (67, 3, 1), (35, 2, 2), (68, 3, 2)))
] + [
    # ragged last x-strip (xin false on some lanes): W = XW - 1, XW, XW + 1, together with a ragged last y-strip
    _pin('first', (1, 0), co, (1, 2, 35, ww), 320 + i, _valu(co, nxs=nxs, ragged_x=rag, nys=2, tail=2))
    for i, (co, (ww, nxs, rag)) in enumerate([(8, (31, 1, True)), (8, (32, 1, False)), (8, (33, 2, True)), (16, (15, 1, True)), (16, (16, 1, False)), (16, (17, 2, True))])
] + [
    # D = 1; N = 2; more than 2048 strips (a wave walks a second strip, its accumulators persist): 137 x 3 x 5 = 2055 strips over 512 x 4 waves
    _pin('first', (1, 0), 8, (1, 1, 40, 37), 330, _valu(8, strips=4, wgrid=1, wwalk=1)), _pin('first', (1, 0), 16, (2, 3, 34, 20), 331, _valu(16, strips=24, wgrid=6, wwalk=1)),
    _pin('first', (1, 0), 16, (1, 137, 67, 65), 332, _valu(16, strips=2055, wgrid=512, wwalk=2, nxs=5, nys=3, ragged_x=True, tail=1), slope=-1.0),
] + [
    # the operand-exchanged matrix form at the flow family's tile counts 1, 8, 9, 513 (split tile; the fp32 tile: 1, 4, 9, 342)
    _pin('first', ch, co, FLOW_TILE_SHAPES[t][0], 340 + i, _exch(ch, co, t, FLOW_TILE_SHAPES[t][1], FLOW_TILE_SHAPES[t][2:]), slope=-1.0 if t == 513 else None)
    for i, (t, ch, co) in enumerate([(1, (1, 1), 16), (8, (2, 0), 16), (9, (1, 0), 12), (513, (2, 0), 8), (9, (1, 1), 4), (513, (1, 1), 12)])
] + [
    # smallcin: the remaining classes
    _pin('first', ch, co, _cyc([(1, 5, 9, 18), (2, 3, 35, 7)], i), 350 + i, {m: dict(fwd='thin', wgrad='smallcin') for m in MODES})
    for i, (ch, co) in enumerate([((3, 0), 8), ((4, 0), 16), ((2, 2), 24), ((1, 0), 32), ((2, 0), 24), ((1, 1), 32), ((3, 0), 12)])
]
FIRST = st.fixed_dictionaries(dict(ch=st.sampled_from(FIRST_CH), cout=st.sampled_from(FIRST_COUTS), n=st.integers(1, 2), d=st.integers(1, 9), h=st.integers(1, 40),
                                   w=st.integers(1, 70), slope=st.sampled_from([-1.0, 0.0, 0.01]), fork=st.booleans(), sd=st.integers(0, 999))).map(
    lambda c: dict(c, fam='first'))

FAMILY = {'stride2': (STRIDE2, STRIDE2_PINNED), 'up2': (UP2, UP2_PINNED), 'flow': (FLOW, FLOW_PINNED), 'first': (FIRST, FIRST_PINNED)}
