"""Shared by tests/test_gpu_block_shapes.py (the fused conv + BatchNorm + activation block kernels against float64) and tests/test_block_reference.py
(the same composition in fp32 on torch-CPU against float64, no GPU): hypothesis strategies and pinned examples that name every launcher branch of the
block, builders that turn a drawn case into well-conditioned fp32 CPU inputs, the float64 references, the distances and the tolerances.

Both files run their families through `run_cases` (loss_cases.run_cases: seed 160950, the pinned examples first, then 60 derandomised examples, at
least 90 % of them compared to the end), so the CPU companion sees exactly the examples the device test sees.

Measuring: with DA_BLOCK_SHAPES_REPORT=<path> set, run_cases writes the worst distance recorded so far per family and quantity (and the case that
gave it) to that JSON file when it returns; the table in test_gpu_block_shapes.py was filled from it.

Kinks.  LeakyReLU / ReLU and the pool's arg-max are decided on values fp32 and fp64 compute differently; one flipped voxel moves the data gradient at
27 Cin voxels by far more than any tolerance here.  The float64 reference therefore takes its activation as z * where(mask, 1, slope) with a CONSTANT
mask: its own z > 0 wherever |z| >= G max|z|, and inside that guard band the decision of the side under test, read from the activated tensor that side
returned (`activate`).  The pool routes a window's gradient to its own arg-max unless the float64 top-two gap is below G max|a|, then to the arg-max of
the tested side's activated tensor (`pool`).  How often the band is entered is capped per tensor (`check_band`): 0.1 % of the elements and 64.  Outside
the band a wrong decision of the tested side stays visible: the forward comparison is unmasked.

Plain module, no fixtures, no pytest settings."""
import json
import os

import torch
import torch.nn.functional as F
from hypothesis import strategies as st

import loss_cases as lc
from loss_cases import _cyc, _f64, _leaf, close, dist, note      # noqa: F401  (re-exported for the two test files)

G = 1e-5                   # guard band, in units of the tensor's largest magnitude
BAND_FRAC, BAND_MAX = 1e-3, 64
MOMENTUM, EPS = 0.1, 1e-5  # nn.BatchNorm3d defaults (modules.SegBlock)
M_MIN = 128                # train mode: voxels per channel
# Drawn examples: every tensor an activation is decided on has at least this many elements.  The cap allows 0.1 % of a tensor, so a tensor of fewer than 1000
# elements may not enter the band once, and an element enters it with probability about 3e-5: which of the drawn small tensors does is chance.  At 4000
# elements the cap is 4 against an expectation of 0.1.  The pinned examples keep their shapes.
BAND_ELEMS = 4000
WORK_MAX = 4e6             # per conv: M Cin Cout
TD, TH, TW = 4, 8, 16      # output tile of the matrix forward / data gradient (the weight gradient: two z planes)
FAMILIES = ('block', 'chain', 'chain_pool', 'sums')


def run_cases(strategy, body, pinned=()):
    """loss_cases.run_cases (seed, example count, pinned examples first, the 90 % assertion) + this module's report."""
    ran = lc.run_cases(strategy, body, pinned)
    write_report()
    return ran


def write_report():
    path = os.environ.get('DA_BLOCK_SHAPES_REPORT')
    if path:
        with open(path, 'w') as f:
            json.dump({k: v for k, v in lc.WORST.items() if any(w in FAMILIES for w in k.split('/')[0].split())}, f, indent=1, sort_keys=True)


# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# CEIL: what the existing fp32 comparisons assert (tests/test_gpu_ops.py check(): 1e-4 for convolution tensors; test_bn_act_random_shapes: 2e-5 for the
# BatchNorm forward and d_beta, 2e-4 for dx and d_gamma, 1e-5 for running statistics; test_deconv_fused_batchnorm_statistics: 1e-6 of sum |term| for
# epilogue sums).  'db_zero': the conv bias gradient in front of a train-mode BatchNorm is zero in exact arithmetic; what a run holds is the rounding of
# sum dz, asserted as max |db| <= tol sum_voxels |dz_ref| (largest channel).  Its ceiling is reasoning, not an existing test: dz = scale (g' - mean g' -
# xhat mean(g' xhat)), so a relative error e in the two means shifts every dz of a channel by e |mean g'| and their sum by e |sum g'| <= e sum |g'|; with
# e = a few fp32 roundings (6e-8 each) plus the fp32 sum of M <= 2^14 terms in blocks, 1e-5 is two orders above what correct fp32 code leaves.
# TOL: what both new files assert, never above CEIL.  Rule (tests/loss_cases.py): where max(4 x device worst, 8 x fp32-CPU-oracle worst) is more than 10 x
# below the ceiling, that value (rounded up to two digits); otherwise the ceiling.  The figures are in the table of tests/test_gpu_block_shapes.py.
# 'dbeta' shares d_gamma's ceiling, not the 2e-5 test_bn_act_random_shapes asserts at M <= 2268: behind a train-mode BatchNorm the gradient reaching a block sums
# to zero per channel, so d_beta = sum dA act'(z) is a cancelling sum like d_gamma, |sum| ~ sum |term| / (2 sqrt M).  The fp32 oracle's own d_beta is up to 1.2e-5 from
# float64 (the pooled block), and the quarter rule of the CPU companion needs 4 x that below the tolerance.
_Q = {'out': 2e-5, 'run': 1e-5, 'dx': 2e-4, 'dw': 1e-4, 'db': 1e-4, 'db_zero': 1e-5, 'dgamma': 2e-4, 'dbeta': 2e-4}
CEIL = {
    'block': dict(_Q), 'chain': dict(_Q), 'chain_pool': dict(_Q),
    'sums': {'y': 1e-4, 'dx': 1e-4, 'sum': 1e-6, 'stats': 2e-5, 'run': 1e-5, 'head': 1e-4},
}
TOL = {
    'block': {'out': 2e-5, 'run': 1e-5, 'dx': 7.2e-6, 'dw': 5.6e-6, 'db': 5.2e-6, 'db_zero': 4.4e-7, 'dgamma': 9.9e-6, 'dbeta': 5.8e-6},
    'chain': {'out': 2e-5, 'run': 1e-5, 'dx': 7.4e-6, 'dw': 1e-4, 'db': 2.5e-6, 'db_zero': 4.4e-7, 'dgamma': 1.5e-5, 'dbeta': 1.1e-5},
    # (chain_pool d_beta: max(4 x device, 8 x oracle) = 9.4e-5 is taken although it is less than 10 x below the 2e-4 ceiling -- that ceiling is this file's own, ten times
    # what the stand-alone BatchNorm test asserts, so the measured bound is kept instead of it)
    'chain_pool': {'out': 2e-5, 'run': 1e-5, 'dx': 7.6e-6, 'dw': 1e-4, 'db': 6.7e-6, 'db_zero': 3.4e-7, 'dgamma': 2e-4, 'dbeta': 9.4e-5},
    # 'stats' / 'run' (da_bn_train_stats_from_partials, double sums handed in): no fp32 oracle; 4 x the 9.3e-8 / 8.5e-8 measured is below what one fp32 result can be
    # asserted to, so the floor is 8 roundings of the stored fp32 value, 8 x 2^-24.  'head': the tolerance of test_fused_head_softmax_dice_vs_torch_cpu, as given.
    'sums': {'y': 9.1e-6, 'dx': 6.3e-6, 'sum': 1e-6, 'stats': 4.8e-7, 'run': 4.8e-7, 'head': 1e-4},
}
assert all(TOL[f][k] <= CEIL[f][k] for f in CEIL for k in CEIL[f])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def nrm(shape, sd, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(int(sd))) * scale


def ntiles(n, d, h, w):
    return n * ((d + TD - 1) // TD) * ((h + TH - 1) // TH) * ((w + TW - 1) // TW)


def fit(n, d, h, w, convs, train, step=1, m_min=M_MIN, fixed=False, per_voxel=1):
    """Train mode: widen W until every channel has m_min voxels; drawn examples (not `fixed`, the pinned ones) also until the thinnest BatchNorm'd tensor has
    BAND_ELEMS elements (`per_voxel`: 8 where that tensor is a pooled one).  Then shrink W, after it H, until the largest conv (cin, cout) of `convs` is within
    WORK_MAX, never below the first bound."""
    lo = m_min if train else 1
    if not fixed:
        lo = max(lo, -(-BAND_ELEMS * per_voxel // min(co for _, co in convs)))
    while n * d * h * w < lo:
        w += step
    work = max(ci * co for ci, co in convs)
    while n * d * h * w * work > WORK_MAX and w > step and n * d * h * (w - step) >= lo:
        w -= step
    while n * d * h * w * work > WORK_MAX and h > step and n * d * (h - step) * w >= lo:
        h -= step
    return d, h, w


def block_params(cin, cout, sd, transposed=False, neg_gamma=False, beta0=0.0):
    """weights x 0.2, conv bias x 0.1, gamma = 1 + 0.3 n, beta = beta0 + 0.2 n, drawn running statistics with variance >= 0.5."""
    gamma = 1.0 + 0.3 * nrm((cout,), sd + 2)
    if neg_gamma:
        gamma[1 % cout] = -0.8            # the raw order of that channel is the reverse of the activated order (da_maxpool2_bwd_bst)
    return dict(w=nrm((cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3), sd, 0.2), b=nrm((cout,), sd + 1, 0.1), gamma=gamma,
                beta=beta0 + nrm((cout,), sd + 3, 0.2), rm=nrm((cout,), sd + 4, 0.1), rv=nrm((cout,), sd + 5).abs() * 0.5 + 0.5, cin=cin, cout=cout)


# the shapes pinned by construction: (n, d, h, w) -> tiles of the matrix forward.  One tile; one voxel over a tile on every axis; 1 x 1 x 128; W = 1;
# N = 2 with three tiles per sample; 1, 7, 8, 9 and 17 tiles = the persistent grid's nblocks cases 1, 7, 8, 8 walking 9, 16 walking 17.
SHAPES_PINNED = [(1, 4, 8, 16), (1, 5, 9, 17), (1, 1, 1, 128), (1, 9, 19, 1), (2, 4, 8, 48), (1, 4, 8, 112), (1, 8, 16, 32), (1, 4, 24, 48), (1, 4, 8, 272)]
SHAPES_TILES = [1, 8, 8, 9, 6, 7, 8, 9, 17]
_shape = dict(n=st.integers(1, 2), d=st.integers(1, 9), h=st.integers(1, 19), w=st.integers(1, 35))


def launcher_nrep(tiles, cout, mode, pro=False):
    """N-tiles per workgroup that conv3_mfma_fwd_impl picks for a forward of `tiles` output tiles (restated: pick_nrep, the cap at 2 outside the plain fp32 matrix
    mode, and the makespan model that prefers one N-tile per workgroup while the grid has room).  At fewer than 129 tiles it is always 1."""
    nt = (cout + 15) // 16
    nrep = nt if nt <= 3 else (2 if nt % 2 == 0 else (3 if nt % 3 == 0 else 2))
    if (mode != 'fp32' or pro) and nrep > 2:
        nrep = 2
    if nrep > 1:
        def cost(r):
            nb = min(max(512 // -(-nt // r), 1), tiles)
            return -(-tiles // nb) * r * (1.08 if r == 1 else 1.0)
        if cost(1) < cost(nrep):
            nrep = 1
    return nrep


# The N-tile branches need a grid too full for one N-tile per workgroup: (shape, Cout) -> NREP = 2 for two (257 tiles), three (171) and four (129) N-tiles, and in
# the plain fp32 matrix mode NREP = 3 at 341 tiles (no statistics epilogue there: da_bn_train_stats runs).  Rows of 3 voxels: ragged tiles within WORK_MAX.
NREP_PINNED = [((1, 1, 3, 4112), 32), ((1, 1, 3, 2725), 48), ((1, 1, 3, 2050), 64), ((1, 1, 1, 5445), 48)]


# ---- the float64 / fp32 composition ----------------------------------------------------------------------------------------------
def check_band(counts):
    """The cap on decisions taken from the tested side: per tensor at most 0.1 % of its elements and at most 64."""
    for k, n in counts:
        assert k <= min(BAND_FRAC * n, BAND_MAX), 'guard band entered at %d of %d elements (%r)' % (k, n, counts)


def activate(z, slope, decided, counts):
    """z * where(mask, 1, slope), mask constant.  decided = None: the side's own z > 0 (the fp32 oracle, playing the device).  Else the activated tensor
    of the tested side, which decides inside the guard band."""
    zd = z.detach()
    mask = zd > 0
    if decided is not None:
        band = zd.abs() < G * zd.abs().max()
        counts.append((int(band.sum()), zd.numel()))
        mask = torch.where(band, decided.to(zd.device) > 0, mask)
    one = torch.ones((), dtype=z.dtype)
    return z * torch.where(mask, one, one * slope)


def _windows(t):
    N, C, D, H, W = t.shape
    return t.reshape(N, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, D // 2, H // 2, W // 2, 8)


def pool(a, decided, counts):
    """F.max_pool3d(a, 2) whose gradient is routed by a constant index: the window's own arg-max, or inside the guard band (top-two gap below G max|a|) the
    arg-max of the tested side's activated tensor.  A window whose maximum is exactly zero (ReLU, every voxel inactive) is no band case: whichever voxel
    receives the gradient has act' = 0, so the routing reaches nothing."""
    wa = _windows(a)
    wd = wa.detach()
    idx = wd.argmax(-1)
    if decided is not None:
        top = wd.topk(2, dim=-1).values
        band = ((top[..., 0] - top[..., 1]) < G * wd.abs().max()) & (top[..., 0] != 0)
        counts.append((int(band.sum()), band.numel()))
        idx = torch.where(band, _windows(decided).argmax(-1), idx)
    return wa.gather(-1, idx.unsqueeze(-1)).squeeze(-1)


class _Block(object):
    """One conv -> BatchNorm -> activation block of the reference, its leaves in `dtype`."""

    def __init__(self, p, dtype, train, slope, transposed=False):
        self.w, self.b, self.gamma, self.beta = (_leaf(p[k], dtype) for k in ('w', 'b', 'gamma', 'beta'))
        self.rm, self.rv = p['rm'].clone().to(dtype), p['rv'].clone().to(dtype)
        self.train, self.slope, self.transposed = train, slope, transposed

    def __call__(self, x, decided, counts):
        y = F.conv_transpose3d(x, self.w, self.b, padding=1) if self.transposed else F.conv3d(x, self.w, self.b, padding=1)
        y.retain_grad()
        self.y = y
        z = F.batch_norm(y, self.rm, self.rv, self.gamma, self.beta, self.train, MOMENTUM, EPS)
        self.act = activate(z, self.slope, decided, counts)
        return self.act

    def results(self, i, out):
        """After backward: this block's quantities into `out` under '<name><i>'."""
        dz = self.y.grad
        out['dw%d' % i], out['db%d' % i], out['dgamma%d' % i], out['dbeta%d' % i] = (_f64(t.grad) for t in (self.w, self.b, self.gamma, self.beta))
        out['rm%d' % i], out['rv%d' % i] = _f64(self.rm), _f64(self.rv)
        out['dzsum%d' % i] = float(dz.detach().double().abs().sum((0, 2, 3, 4)).max())
        out['train%d' % i] = self.train


def compare(family, got, ref, tol):
    """Every quantity of a run against the float64 reference, recorded under `family` and asserted at tol[quantity]: 'out*', 'dx*' tensors, per block i
    'dw<i>', 'dgamma<i>', 'dbeta<i>', 'rm<i>', 'rv<i>', and 'db<i>' -- an ordinary tensor in eval mode, in train mode max |db| in units of sum |dz_ref|."""
    for k in sorted(ref):
        if k.startswith(('dzsum', 'train', 'act', 'band')) or ref[k] is None:
            continue
        q = 'run' if k[:2] in ('rm', 'rv') else k.rstrip('0123456789')
        if q in ('outs', 'outp'):
            q = 'out'
        if q in ('dskip',):
            q = 'dx'
        if q == 'db' and ref['train' + k[2:]]:
            e = float(got[k].detach().double().abs().max()) / max(ref['dzsum' + k[2:]], 1e-30)
            assert e == e, 'non-finite bias gradient'
            note(family, 'db_zero', e)
            assert e <= tol['db_zero'], '%s %s: max|db| = %.3e of sum|dz| (tolerance %.1e)' % (family, k, e, tol['db_zero'])
            continue
        close(family, q, got[k], ref[k], tol[q])


# ---- family 1: one ConvBNActFn ----------------------------------------------------------------------------------------------------
# launcher branch <- channel class: pick_ck = 16 | pick_ck = 8 | pick_ck = 0 (direct kernels: *stats_nparts == 0, da_bn_train_stats runs)
CH16, CH8, CH0 = [(16, 0), (32, 16), (16, 16), (64, 32)], [(8, 0), (8, 16), (24, 0)], [(1, 0), (3, 0), (12, 4)]
CH_CLASSES = CH16 + CH8 + CH0
# Cout on the matrix path: 8, 16, 32 (one or two N-tiles), 12 (ragged N-tile), 48 (three N-tiles, two per workgroup), 64;  3, 5 leave it
COUTS = [8, 16, 32, 12, 48, 64, 3, 5]
BLOCK = st.fixed_dictionaries(dict(ch=st.sampled_from(CH_CLASSES), cout=st.sampled_from(COUTS), train=st.booleans(), slope=st.sampled_from([0.0, 0.01]),
                                   transposed=st.booleans(), sd=st.integers(0, 999), **_shape))
_SMALL = [(1, 5, 9, 17), (2, 3, 10, 9), (1, 6, 7, 20)]


def _blk(ch, cout, i, shape, train=None):
    n, d, h, w = shape
    return dict(ch=ch, cout=cout, train=(i % 3 != 2) if train is None else train, slope=_cyc([0.01, 0.0], i), transposed=i % 4 == 3, sd=i, n=n, d=d, h=h, w=w, fixed=True)


BLOCK_PINNED = ([_blk(ch, _cyc(COUTS, i), i, _cyc(_SMALL, i)) for i, ch in enumerate(CH_CLASSES)] +
                [_blk(_cyc(CH16 + CH8, i), co, 20 + i, _cyc(_SMALL, i + 1)) for i, co in enumerate(COUTS)] +
                [_blk((16, 0) if i % 2 else (8, 0), 16 if i % 3 else 8, 40 + i, s, train=True) for i, s in enumerate(SHAPES_PINNED)] +
                [_blk((8, 0), co, 60 + i, s, train=True) for i, (s, co) in enumerate(NREP_PINNED)] +
                # two N-tiles with 16-channel chunks (paired staging off: NREP = 2), in eval mode (no statistics: the plain NREP = 2 kernels), and a data gradient of two
                # N-tiles split over two output tensors (Cin = 16 + 16)
                [_blk((16, 0), 32, 70, (1, 1, 1, 4112), train=True), _blk((8, 0), 32, 71, (1, 1, 3, 4112), train=False), _blk((16, 16), 8, 72, (1, 1, 3, 4112), train=True)])


def stats_from_epilogue(case):
    """Does the forward's epilogue deliver the train-mode statistics (split matrix mode)?  da_conv3_mfma_fwd_supported."""
    c1, c2 = case['ch']
    return (c1 + c2) % 8 == 0 and c1 % 8 == 0 and case['cout'] >= 8 and case['cout'] % 4 == 0


def build_block(case):
    (c1, c2), cout, n = case['ch'], case['cout'], case['n']
    d, h, w = fit(n, case['d'], case['h'], case['w'], [(c1 + c2, cout)], case['train'], fixed=case.get('fixed', False))
    sd = 100 * case['sd']
    return dict(x1=nrm((n, c1, d, h, w), sd + 10), x2=nrm((n, c2, d, h, w), sd + 11) if c2 else None, p=block_params(c1 + c2, cout, sd, case['transposed']),
                gout=nrm((n, cout, d, h, w), sd + 12), train=case['train'], slope=case['slope'], transposed=case['transposed'], dims=(n, d, h, w))


def ref_block(inp, dtype, decided=None):
    """dict of the block's quantities; decided: {'act0': activated tensor of the tested side} (None: own decisions)."""
    counts = []
    x1, x2 = _leaf(inp['x1'], dtype), (_leaf(inp['x2'], dtype) if inp['x2'] is not None else None)
    blk = _Block(inp['p'], dtype, inp['train'], inp['slope'], inp['transposed'])
    out = blk(torch.cat((x1, x2), 1) if x2 is not None else x1, decided['act0'] if decided else None, counts)
    out.backward(inp['gout'].to(dtype))
    res = dict(out=_f64(out), dx1=_f64(x1.grad), dx2=_f64(x2.grad) if x2 is not None else None, act0=out.detach(), band=counts)
    blk.results(0, res)
    return res


# ---- family 2: chains of SegBlocks linked by LazyAct ------------------------------------------------------------------------------
# b1(x, lazy_out=True) -> b2(lazy [, skip] | skip, lazy) [lazy -> b3]; the last block materialised.  form: 'single' | 'lazy_skip' | 'skip_lazy'
# (block-1 Cout, form, skip channels, block-2 Cout) drawn from the route rows, half of them the routes that hand BatchNorm-backward sums over through ops._bwd_stats
CHAIN_ROWS = ([(cm, 'single', 16, co) for cm in (8, 16) for co in (8, 16, 32)] + [(32, 'lazy_skip', 16, 16)] * 3 +
              [(32, 'single', 16, 16), (4, 'single', 16, 16), (12, 'single', 8, 16), (16, 'single', 16, 12), (16, 'single', 16, 3), (8, 'single', 16, 4),
               (16, 'skip_lazy', 16, 16), (8, 'skip_lazy', 8, 16), (16, 'lazy_skip', 8, 16)])
CHAIN = st.fixed_dictionaries(dict(cin=st.sampled_from([1, 4, 8]), row=st.sampled_from(CHAIN_ROWS), third=st.sampled_from([None, None, 8, 16]),
                                   train=st.sampled_from([True, True, False]), slopes=st.sampled_from([(0.01, 0.01), (0.0, 0.0), (0.01, 0.0), (0.0, 0.01)]),
                                   neg=st.booleans(), sd=st.integers(0, 999), **_shape)).map(
    lambda c: dict({k: v for k, v in c.items() if k != 'row'}, cmid=c['row'][0], form=c['row'][1], cskip=c['row'][2], cout=c['row'][3]))


def _chn(cmid, cout, i, shape=None, form='single', cskip=16, route=None, train=True, neg=False):
    n, d, h, w = shape or _cyc(_SMALL, i)
    return dict(cin=_cyc([4, 8, 1], i), cmid=cmid, form=form, cskip=cskip, cout=cout, third=None, train=train, slopes=_cyc([(0.01, 0.01), (0.0, 0.0), (0.01, 0.0)], i),
                neg=neg, sd=200 + i, n=n, d=d, h=h, w=w, route=route, fixed=True)


# route <- value (two-block chains).  route = which of (fwd_pro, wgrad_pro, dgrad_bst + bn_act_bwd_dbias_pre) must have run for block 2; the plain entries
# (da_bn_act_fwd fall-back, da_conv3d_k3_wgrad, da_conv3d_k3_dgrad + the stand-alone sums) must have run wherever they did not.
FULL, NO_BST, NONE = (True, True, True), (True, True, False), (False, False, False)
CHAIN_PINNED = ([_chn(cm, co, i, route=FULL, neg=i == 1) for i, (cm, co) in enumerate([(8, 8), (16, 16), (16, 32), (16, 8), (8, 32)])] +
                [_chn(32, 16, 5, form='lazy_skip', cskip=16, route=FULL),                     # the two-launch concat form of dgrad_bst
                 _chn(4, 16, 6, route=NONE), _chn(12, 16, 13, route=NONE, neg=True),          # pick_ck(4 | 12, 0) = 0: fwd_pro declines, nothing of block 2 takes the prologue
                 _chn(32, 16, 7, route=NO_BST),                                               # single-input C1 = 32: ops._DGRAD_BST_MAXC
                 _chn(16, 12, 8, route=NO_BST),                                               # dgrad_bst declines (pick_ck(12, 0) = 0)
                 _chn(8, 3, 9, route=NONE), _chn(16, 4, 10, route=NONE),                      # fwd_pro declines: _apply_pro
                 _chn(16, 16, 11, form='skip_lazy', cskip=16, route=NO_BST),                  # the lazy tensor second: prologue on input 2, no hand-over
                 _chn(16, 16, 12, route=FULL, train=False)] +                                 # eval: the sums are handed over and dropped, da_bn_act_bwd_dbias runs (train = 0)
                [_chn(16 if i % 2 else 8, 16, 20 + i, shape=s, route=FULL) for i, s in enumerate(SHAPES_PINNED)] +
                # block 2 with two and four N-tiles behind a LazyAct at tile counts that force NREP = 2 (the prologue + statistics kernels of two N-tiles), and the
                # concat form of the hand-over at a second, ragged shape
                [_chn(8, 32, 40, shape=(1, 1, 3, 4112), route=FULL), _chn(16, 64, 41, shape=(1, 1, 1, 2050), route=FULL),
                 _chn(32, 16, 42, shape=(1, 5, 9, 17), form='lazy_skip', cskip=16, route=FULL), _chn(32, 16, 43, shape=(2, 4, 8, 48), form='lazy_skip', cskip=16, route=FULL)])


def build_chain(case):
    n, cin, cmid, cout, form = case['n'], case['cin'], case['cmid'], case['cout'], case['form']
    c2in = cmid + (case['cskip'] if form != 'single' else 0)
    convs = [(cin, cmid), (c2in, cout)] + ([(cout, case['third'])] if case['third'] else [])
    d, h, w = fit(n, case['d'], case['h'], case['w'], convs, case['train'], fixed=case.get('fixed', False))
    sd = 100 * case['sd']
    s1, s2 = case['slopes']
    slopes = [s1, s2, s1][:len(convs)]
    return dict(x=nrm((n, cin, d, h, w), sd + 10), skip=nrm((n, case['cskip'], d, h, w), sd + 11) if form != 'single' else None, form=form,
                blocks=[block_params(ci, co, sd + 20 * (i + 1), neg_gamma=case['neg'] and i == 0) for i, (ci, co) in enumerate(convs)], slopes=slopes,
                gout=nrm((n, convs[-1][1], d, h, w), sd + 12), train=case['train'], dims=(n, d, h, w))


def ref_chain(inp, dtype, decided=None):
    counts = []
    x, skip = _leaf(inp['x'], dtype), (_leaf(inp['skip'], dtype) if inp['skip'] is not None else None)
    blocks = [_Block(p, dtype, inp['train'], s) for p, s in zip(inp['blocks'], inp['slopes'])]
    a = x
    res = {}
    for i, blk in enumerate(blocks):
        if i == 1 and skip is not None:
            a = torch.cat((a, skip) if inp['form'] == 'lazy_skip' else (skip, a), 1)
        a = blk(a, decided['act%d' % i] if decided else None, counts)
        res['act%d' % i] = a.detach()
    a.backward(inp['gout'].to(dtype))
    res.update(out=_f64(a), dx=_f64(x.grad), dskip=_f64(skip.grad) if skip is not None else None, band=counts)
    for i, blk in enumerate(blocks):
        blk.results(i, res)
    return res


# ---- family 3: SegBlock(lazy) -> MaxPool2SkipFn(raw, scale, shift, slope) -> one SegBlock per output --------------------------------
# C = 8, 16, 32: da_maxpool2_fwd_pro / da_maxpool2_bwd_bst (C / 4 a power of two);  C = 12: the backward declines -> da_maxpool2_bwd[_add] + stand-alone sums
POOL = st.fixed_dictionaries(dict(cin=st.sampled_from([1, 4, 8]), c=st.sampled_from([8, 12, 16, 32]), cs=st.sampled_from([8, 16]), cp=st.sampled_from([8, 16]),
                                  skip_grad=st.booleans(), train=st.sampled_from([True, True, False]), slope=st.sampled_from([0.0, 0.01]), neg=st.booleans(),
                                  sd=st.integers(0, 999), n=st.integers(1, 2), d=st.integers(1, 4), h=st.integers(1, 9), w=st.integers(1, 17)))
POOL_BETA0 = 0.5
POOL_PINNED = [dict(cin=_cyc([4, 1, 8], i), c=c, cs=_cyc([8, 16], i), cp=_cyc([16, 8], i), skip_grad=i % 2 == 0, train=True, slope=_cyc([0.01, 0.0], i // 2), neg=i in (1, 2),
                    sd=300 + i, n=1 + i % 2, d=_cyc([2, 3], i), h=_cyc([5, 4, 9], i), w=_cyc([9, 8, 17], i), fixed=True) for i, c in enumerate([8, 16, 32, 12, 8, 16, 32, 12])]


def build_pool(case):
    n, cin, c = case['n'], case['cin'], case['c']
    convs = [(cin, c), (c, case['cs']), (c, case['cp'])]
    # the pooled block keeps M_MIN voxels, in eval mode too: a tensor of fewer than 1000 elements could not enter the guard band even once
    d, h, w = fit(n, 2 * case['d'], 2 * case['h'], 2 * case['w'], convs, True, step=2, m_min=8 * M_MIN, fixed=case.get('fixed', False), per_voxel=8)
    sd = 100 * case['sd']
    # The pooled block's beta is centred at POOL_BETA0 instead of 0.  A window whose eight voxels are all negative holds LeakyReLU values compressed 100-fold, its
    # top-two gap with them, and 3 - 5 % of such windows fall below G max|a|; with beta centred at 0 a channel of small |gamma| has up to 20 % of them, and
    # the band was entered at 0.1 - 0.8 % of the windows (measured on these examples), above the cap.  The cap is kept; the inputs move.
    return dict(x=nrm((n, cin, d, h, w), sd + 10), blocks=[block_params(ci, co, sd + 20 * (i + 1), neg_gamma=case['neg'] and i == 0, beta0=POOL_BETA0 if i == 0 else 0.0)
                                                            for i, (ci, co) in enumerate(convs)],
                gs=nrm((n, case['cs'], d, h, w), sd + 12), gp=nrm((n, case['cp'], d // 2, h // 2, w // 2), sd + 13), train=case['train'], slope=case['slope'],
                skip_grad=case['skip_grad'], dims=(n, d, h, w))


def ref_pool(inp, dtype, decided=None):
    """decided: 'act0' (the activated skip tensor: block 1's mask and the pool's routing), 'act1' / 'act2' (the skip / pooled branch's output)."""
    counts = []
    x = _leaf(inp['x'], dtype)
    b0, bs, bp = (_Block(p, dtype, inp['train'], inp['slope']) for p in inp['blocks'])
    a = b0(x, decided['act0'] if decided else None, counts)
    pooled = pool(a, decided['act0'].to(dtype) if decided else None, counts)
    outp = bp(pooled, decided['act2'] if decided else None, counts)
    loss = (outp * inp['gp'].to(dtype)).sum()
    outs = None
    if inp['skip_grad']:
        outs = bs(a, decided['act1'] if decided else None, counts)
        loss = loss + (outs * inp['gs'].to(dtype)).sum()
    loss.backward()
    res = dict(outp=_f64(outp), outs=_f64(outs) if outs is not None else None, dx=_f64(x.grad), act0=a.detach(), act2=outp.detach(),
               act1=outs.detach() if outs is not None else None, band=counts)
    b0.results(0, res)
    bp.results(2, res)
    if outs is not None:
        bs.results(1, res)
    return res


# ---- family 4: the epilogue sums through the C ABI ---------------------------------------------------------------------------------
# forward statistics: every channel class of the matrix path;  data gradient: C1 = 8, 12, 16, 32 (two N-tiles, reached by no caller) single, 32 + 16 concat
SUMS = st.fixed_dictionaries(dict(ch=st.sampled_from(CH16 + CH8), cout=st.sampled_from([8, 12, 16, 32, 48, 64]), c1=st.sampled_from([8, 12, 16, 32, (32, 16)]),
                                  lcout=st.sampled_from([8, 16, 32]), slope=st.sampled_from([0.0, 0.01]), sd=st.integers(0, 999), **_shape))
SUMS_PINNED = ([dict(ch=_cyc([(16, 0), (8, 0)], i), cout=_cyc([16, 8], i), c1=_cyc([16, 8, 32, 12, (32, 16)], i), lcout=_cyc([16, 8], i), slope=_cyc([0.01, 0.0], i),
                     sd=400 + i, n=s[0], d=s[1], h=s[2], w=s[3]) for i, s in enumerate(SHAPES_PINNED)] +
               [dict(ch=(8, 0), cout=co, c1=8, lcout=8, slope=0.01, sd=440 + i, n=s[0], d=s[1], h=s[2], w=s[3]) for i, (s, co) in enumerate(NREP_PINNED)] +
               [dict(ch=ch, cout=_cyc([16, 12, 48, 64, 8, 32], i), c1=_cyc([(32, 16), 32, 12, 8, 16], i), lcout=_cyc([16, 8, 32], i), slope=_cyc([0.0, 0.01], i),
                     sd=420 + i, n=s[0], d=s[1], h=s[2], w=s[3]) for i, (ch, s) in enumerate(zip(CH16 + CH8, _SMALL + [(2, 5, 9, 17), (1, 8, 9, 33), (2, 4, 8, 16), (1, 3, 17, 20)]))])


def build_sums(case):
    (c1, c2), cout, n = case['ch'], case['cout'], case['n']
    g1, g2 = case['c1'] if isinstance(case['c1'], tuple) else (case['c1'], 0)
    d, h, w = fit(n, case['d'], case['h'], case['w'], [(c1 + c2, cout), (g1 + g2, case['lcout'])], False, fixed=True)      # (no decision is taken here: no minimum size)
    sd = 100 * case['sd']
    stats = torch.stack([nrm((g1,), sd + 30, 0.1), torch.ones(g1), 1.0 + 0.3 * nrm((g1,), sd + 31), nrm((g1,), sd + 32, 0.2)])      # mean | rstd (not read) | scale | shift
    return dict(x1=nrm((n, c1, d, h, w), sd + 10), x2=nrm((n, c2, d, h, w), sd + 11) if c2 else None, w=nrm((cout, c1 + c2, 3, 3, 3), sd, 0.2), b=nrm((cout,), sd + 1, 0.1),
                dy=nrm((n, case['lcout'], d, h, w), sd + 12), wl=nrm((case['lcout'], g1 + g2, 3, 3, 3), sd + 2, 0.2), yraw=nrm((n, g1, d, h, w), sd + 13),
                stats=stats, g=(g1, g2), slope=case['slope'], dims=(n, d, h, w))


def ref_sums(inp, dtype):
    """The forward output and the data gradient of the two convolutions of a family-4 example."""
    x = torch.cat((inp['x1'], inp['x2']), 1) if inp['x2'] is not None else inp['x1']
    y = F.conv3d(x.to(dtype), inp['w'].to(dtype), inp['b'].to(dtype), padding=1)
    xin = torch.zeros((inp['dims'][0], sum(inp['g'])) + tuple(inp['dims'][1:]), dtype=dtype, requires_grad=True)
    F.conv3d(xin, inp['wl'].to(dtype), None, padding=1).backward(inp['dy'].to(dtype))
    return _f64(y), _f64(xin.grad)


def col_err(got, terms):
    """Largest per-channel error of column sums `got` [C] against the float64 sum of `terms` [..., C] (channels last), in units of sum |term|."""
    t = terms.double().cpu().reshape(-1, terms.shape[-1])
    return float(((got.double().cpu() - t.sum(0)).abs() / t.abs().sum(0).clamp_min(1e-300)).max())
