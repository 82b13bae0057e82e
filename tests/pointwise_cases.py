"""Shared by tests/test_gpu_pointwise_shapes.py (the up-sampler and 1x1 conv kernels of deconv.hip / pointwise_mfma.hip against float64) and
tests/test_pointwise_reference.py (the same operations in fp32 on torch-CPU against float64, no GPU): pinned examples that name every launcher branch,
hypothesis strategies, builders that turn a case into well-conditioned fp32 CPU inputs, the float64 references, the two launcher decisions the pinned
sizes are built on (restated), and the tolerances.

Conventions are those of tests/block_cases.py: every family runs `run_cases` (loss_cases.run_cases: seed 160950, the pinned examples first, then 60
derandomised examples, at least 90 % compared to the end); distances by `close` / `dist` / `note`; LeakyReLU / ReLU decisions by block_cases.activate (the
float64 reference decides for itself outside the guard band |z| < G max|z| and takes the tested side's decision inside it, capped per tensor at 0.1 % of
its elements and 64).  With DA_POINTWISE_SHAPES_REPORT=<path> set, run_cases writes the worst distance per family and quantity to that JSON file.

Plain module, no fixtures, no pytest settings."""
import json
import os

import torch
import torch.nn.functional as F
from hypothesis import strategies as st

import block_cases as bc
import loss_cases as lc
from block_cases import BAND_ELEMS, EPS, M_MIN, MOMENTUM, activate, check_band, compare, nrm      # noqa: F401  (re-exported for the two test files)
from loss_cases import _cyc, _f64, _leaf, close, dist, note                                       # noqa: F401

FAMILIES = ('conv1x1', 'deconv', 'upblock', 'bf16')


def run_cases(strategy, body, pinned=()):
    ran = lc.run_cases(strategy, body, pinned)
    write_report()
    return ran


def write_report():
    path = os.environ.get('DA_POINTWISE_SHAPES_REPORT')
    if path:
        with open(path, 'w') as f:
            json.dump({k: v for k, v in lc.WORST.items() if any(w in FAMILIES for w in k.split('/')[0].split())}, f, indent=1, sort_keys=True)


# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# CEIL: what the suite asserted before these files (tests/test_gpu_ops.py check(): 1e-4 for y, dx, dW, db; block_cases._Q for the BatchNorm quantities;
# test_deconv_fused_batchnorm_statistics: 1e-6 of sum |term| for epilogue sums).
# TOL: what both new files assert, never above CEIL.  Rule (tests/loss_cases.py): where max(4 x device worst, 8 x fp32-CPU-oracle worst) is more than 10 x
# below the ceiling, that value rounded up to two digits; otherwise the ceiling.  The figures are in the table of tests/test_gpu_pointwise_shapes.py.
_P = {'y': 1e-4, 'dx': 1e-4, 'dw': 1e-4, 'db': 1e-4}
CEIL = {'conv1x1': dict(_P), 'deconv': dict(_P), 'upblock': dict(bc._Q, sum=1e-6)}
TOL = {
    'conv1x1': {'y': 3.7e-6, 'dx': 3.3e-6, 'dw': 4.7e-6, 'db': 3.7e-6},
    # dw, db: 8 x the fp32 oracle's own distance (3.5e-6 / 1.2e-5: torch-CPU's fp32 sums over up to 270 000 fine voxels) is less than 10 x below the ceiling: stay
    'deconv': {'y': 5.9e-6, 'dx': 7.2e-6, 'dw': 1e-4, 'db': 1e-4},
    # out, run, db, d_gamma, d_beta: max(4 x device, 8 x oracle) = 4.9e-6, 1.2e-6, 1.5e-5, 2.3e-5, 2.1e-5 are less than 10 x below their ceilings: stay; dw: 8 x oracle = 2.7e-5: stays
    'upblock': dict(bc._Q, dx=6.3e-6, db_zero=6.5e-7, sum=1e-6),
}
# the bf16 twins' fp32 results, and the `tol` of their bf16 results' bound, take the fp32 family's tolerance for the quantity: TOL['conv1x1'] for the 1x1 twins,
# TOL['deconv'] for the up-sampler's.  The family has no tolerance of its own.
assert all(TOL[f][k] <= CEIL[f][k] for f in CEIL for k in CEIL[f])
BF16_EPS = 2.0 ** -8       # bf16 keeps 8 significant bits: its spacing is between 2^-8 and 2^-7 of the value, so a correctly rounded store is off by at most 2^-8 |value|


# ---- the two launcher decisions, restated ----------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def pw_supported(k, n):
    """da_pw_supported: both channel counts multiples of 16 in 16 ... 1024 (the matrix path)."""
    return k % 16 == 0 and n % 16 == 0 and 16 <= k <= 1024 and 16 <= n <= 1024


def wg_vox_per_wave(M, ntaps, cin_slice, cout_slice):
    """pointwise_mfma.hip wg_blocks: blocks = min(1024, 64 MiB / (4 O)), O the outputs of one (<= 64 x 64) slice; a wave takes ceil(M / (4 blocks)) voxels
    ROUNDED UP TO A MULTIPLE OF 4 (one K-step is 4 voxels).  4: one K-step, one voxel per lane; 8: two K-steps (one loop trip, one carry per lane);
    12: the loop's second trip, whose fetch(vb + 8) delivers data.  So 8 needs M > 16 blocks and 12 needs M > 32 blocks."""
    O = ntaps * min(cin_slice, 64) * min(cout_slice, 64)
    blocks = max(1, min(1024, (64 << 20) // (4 * O)))
    return max(4, _cdiv(_cdiv(M, 4 * blocks), 4) * 4)


def wg_idle_waves(M, vpw):
    """waves of the last workgroup whose range starts at or past M (v0 >= v1)"""
    last = M - (_cdiv(M, 4 * vpw) - 1) * 4 * vpw
    return 4 - _cdiv(last, vpw)


def db_chunks_per_block(M):
    """pointwise_mfma.hip db_blocks: 32-voxel chunks walked by min(chunks, 512) workgroups -> the most chunks one workgroup walks."""
    n = _cdiv(M, 32)
    return _cdiv(n, min(n, 512))


def vox(dims):
    n, d, h, w = dims
    return n * d * h * w


# ---- family 1: 1x1x1 convolution through ops.Conv1x1Fn ------------------------------------------------------------------------------
# launcher branch <- (Cin, Cout)
TILE_PAIRS = [(16 * a, 16 * b) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4)]      # pw_mfma_kernel<KC, NT>, its swapped GATHER pair, pw_wgrad_slice ntaps = 1
C1_WIDE = [(80, 144), (128, 32), (192, 16), (48, 96), (96, 48), (112, 64)]       # host-tiled 64-wide slices; three K slices; the 48-channel slices
C1_DIRECT = [(6, 5), (16, 3), (16, 40), (16, 42), (40, 5), (40, 100)]            # conv1x1_kernel<8 | 32>, ragged group + scalar stores, dgrad <32>, direct wgrad O = 4000
C1_ROWS = [1, 15, 17, 63, 65, 255, 256, 257]                                     # lane, wave-tile (64 rows) and workgroup (256 rows) edges
# weight-gradient walk at (16, 16) (O = 256: 1024 blocks).  4096 ... 8193 are the sizes the issue named; by wg_vox_per_wave they all still take ONE K-step
# (the launcher rounds voxels per wave up to a multiple of 4 after dividing by 4 blocks), so the sizes that do reach the branches stand next to them:
# 16384 last with one voxel per lane; 16385 (three idle waves) and 16411 (ragged last wave) 8 per wave; 32769 and 32771 12 per wave.
C1_WALK = [4096, 4097, 8203, 8193, 16384, 16385, 16411, 32769]
C1_SMALL = [(1, 3, 5, 7), (2, 2, 3, 11), (1, 1, 1, 67)]
_CH_IN, _CH_OUT = [6, 16, 32, 48, 64, 80, 112], [3, 5, 16, 32, 48, 64, 96]
C1 = st.fixed_dictionaries(dict(cin=st.sampled_from(_CH_IN), cout=st.sampled_from(_CH_OUT), n=st.integers(1, 2), d=st.integers(1, 5), h=st.integers(1, 6),
                                w=st.integers(1, 33), pro=st.sampled_from([None, None, 0.0, 0.01]), sd=st.integers(0, 999))).map(
    lambda c: dict(cin=c['cin'], cout=c['cout'], dims=(c['n'], c['d'], c['h'], c['w']), pro=c['pro'], sd=c['sd']))


def _c1(ch, i, dims, pro=None):
    return dict(cin=ch[0], cout=ch[1], dims=dims, pro=pro, sd=i, fixed=True)


C1_PINNED = ([_c1(ch, i, _cyc(C1_SMALL, i), _cyc([None, 0.01, None, 0.0], i)) for i, ch in enumerate(TILE_PAIRS)] +
             [_c1(ch, 20 + i, _cyc(C1_SMALL, i + 1), 0.01 if ch == (128, 32) else None) for i, ch in enumerate(C1_WIDE)] +
             # (the prologue on 48-channel slices: da_conv1x1_wgrad_pro; and on a non-matrix Cin, where both prologue entries decline and ops._apply_pro runs)
             [_c1((48, 96), 27, (1, 3, 5, 7), 0.01), _c1((112, 64), 28, (2, 2, 3, 11), 0.0)] +
             [_c1(ch, 30 + i, _cyc(C1_SMALL, i), 0.01 if ch == (6, 5) else None) for i, ch in enumerate(C1_DIRECT)] + [_c1((16, 3), 37, (1, 3, 5, 7), 0.0)] +
             [_c1(ch, 40 + i, (1, 1, 1, m)) for ch in ((16, 16), (32, 64)) for i, m in enumerate(C1_ROWS)] +
             [_c1((16, 16), 60 + i, (1, 1, 1, m)) for i, m in enumerate(C1_WALK)] + [_c1((16, 16), 69, (1, 1, 1, 32771), 0.01)] +
             [_c1((6, 5), 70, (1, 1, 1, 65601))])       # direct weight gradient: parts_for gives 1024 blocks of 2 x 64 rows


def pro_params(c, sd):
    """the deferred BatchNorm of a LazyAct input: scale = 1 + 0.3 n with one negative channel, shift = 0.2 n"""
    scale = 1.0 + 0.3 * nrm((c,), sd + 2)
    scale[1 % c] = -0.8
    return scale, nrm((c,), sd + 3, 0.2)


def build_c1(case):
    cin, cout, (n, d, h, w) = case['cin'], case['cout'], case['dims']
    if case['pro'] is not None and not case.get('fixed'):
        while n * d * h * w * cin < BAND_ELEMS:
            w += 1
    sd = 100 * case['sd']
    inp = dict(x=nrm((n, cin, d, h, w), sd + 10), w=nrm((cout, cin, 1, 1, 1), sd, 0.2), b=nrm((cout,), sd + 1, 0.1), gout=nrm((n, cout, d, h, w), sd + 12),
               pro=case['pro'], dims=(n, d, h, w), cin=cin, cout=cout)
    if case['pro'] is not None:
        inp['scale'], inp['shift'] = pro_params(cin, sd)
    return inp


def ref_c1(inp, dtype, decided=None):
    """y, dx (with a prologue: the gradient with respect to the ACTIVATED input, which is what a LazyAct's producer receives), dW, db.
    decided: {'act': the activated input of the tested side}."""
    counts = []
    x = inp['x'].to(dtype)
    if inp['pro'] is not None:
        z = x * inp['scale'].to(dtype).view(1, -1, 1, 1, 1) + inp['shift'].to(dtype).view(1, -1, 1, 1, 1)
        x = activate(z, inp['pro'], decided['act'] if decided else None, counts)
    a, w, b = _leaf(x, dtype), _leaf(inp['w'], dtype), _leaf(inp['b'], dtype)
    y = F.conv3d(a, w, b)
    y.backward(inp['gout'].to(dtype))
    return dict(y=_f64(y), dx=_f64(a.grad), dw=_f64(w.grad), db=_f64(b.grad), act=a.detach() if inp['pro'] is not None else None, band=counts)


def compare_plain(family, got, ref, tol):
    for k in ('y', 'dx', 'dw', 'db'):
        close(family, k, got[k], ref[k], tol[k])


# ---- family 2: 2x2x2 stride-2 transposed convolution through ops.DeconvK2S2Fn --------------------------------------------------------
D2_WIDE, D2_DIRECT = [(128, 128), (256, 80), (48, 192)], [(6, 5), (16, 5), (5, 16)]
# one voxel; W < 4; W = 1; odd everything with a sample boundary inside a workgroup; exactly 256 coarse voxels; one row of 257
D2_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 3), (1, 2, 3, 1), (2, 3, 5, 7), (1, 4, 8, 8), (1, 1, 1, 257)]
# the weight-gradient walk of the up-sampler form (its (cw, chh, crest) carry).  The issue's sizes, which by wg_vox_per_wave still take one K-step:
D2_WALK_NAMED = [((16, 16), (1, 3, 37, 41)), ((16, 16), (1, 19, 73, 3)), ((16, 16), (1, 67, 63, 1)), ((16, 16), (2, 5, 29, 31)), ((64, 64), (1, 5, 19, 23))]
# ... and the sizes that reach the branches: (16, 16) has 1024 blocks, so 8 voxels per wave from 16385 coarse voxels on (odd W with H and D wraps; W = 3,
# where `cw += 4` wraps more than once; W = 1) and 12 from 32769 on (two loop trips, an N wrap); a (64, 64) slice is capped at 512 blocks: 8 from 8193 on.
D2_WALK = [((16, 16), (1, 11, 37, 41), 8), ((16, 16), (1, 75, 73, 3), 8), ((16, 16), (1, 261, 63, 1), 8), ((16, 16), (2, 19, 29, 31), 12), ((64, 64), (1, 19, 19, 23), 8)]
# a wide layer whose 48 x 64 slice runs MORE blocks than a 64 x 64 slice would (682-block cap against 512): 8303 coarse voxels give 519 blocks of 4 voxels per wave and
# 51 MB of partials where the 64 x 64 figure is 260 blocks and 34 MB -- the wide loop's placement scratch has to lie behind the larger of the two
D2_WIDE_PARTIALS = ((112, 64), (1, 19, 19, 23))
D2_SMALL = [(1, 3, 5, 7), (2, 2, 3, 5), (1, 1, 4, 9)]
D2 = st.fixed_dictionaries(dict(cin=st.sampled_from(_CH_IN), cout=st.sampled_from(_CH_OUT), n=st.integers(1, 2), d=st.integers(1, 5), h=st.integers(1, 6),
                                w=st.integers(1, 9), sd=st.integers(0, 999))).map(
    lambda c: dict(cin=c['cin'], cout=c['cout'], dims=(c['n'], c['d'], c['h'], c['w']), sd=c['sd']))


def _d2(ch, i, dims):
    return dict(cin=ch[0], cout=ch[1], dims=dims, sd=100 + i, fixed=True)


D2_PINNED = ([_d2(ch, i, _cyc(D2_SMALL, i)) for i, ch in enumerate(TILE_PAIRS)] + [_d2(ch, 20 + i, (1, 2, 3, 5)) for i, ch in enumerate(D2_WIDE)] +
             [_d2(ch, 30 + i, _cyc(D2_SMALL, i)) for i, ch in enumerate(D2_DIRECT)] +
             [_d2(ch, 40 + i, s) for ch in ((16, 16), (32, 32)) for i, s in enumerate(D2_SHAPES)] +
             [_d2(ch, 60 + i, s) for i, (ch, s) in enumerate(D2_WALK_NAMED)] + [_d2(ch, 70 + i, s) for i, (ch, s, _) in enumerate(D2_WALK)] + [_d2(D2_WIDE_PARTIALS[0], 80, D2_WIDE_PARTIALS[1])])


def build_d2(case):
    cin, cout, (n, d, h, w) = case['cin'], case['cout'], case['dims']
    sd = 100 * case['sd']
    return dict(x=nrm((n, cin, d, h, w), sd + 10), w=nrm((cin, cout, 2, 2, 2), sd, 0.2), b=nrm((cout,), sd + 1, 0.1), gout=nrm((n, cout, 2 * d, 2 * h, 2 * w), sd + 12),
                dims=(n, d, h, w), cin=cin, cout=cout)


def ref_d2(inp, dtype):
    x, w, b = _leaf(inp['x'], dtype), _leaf(inp['w'], dtype), _leaf(inp['b'], dtype)
    y = F.conv_transpose3d(x, w, b, stride=2)
    y.backward(inp['gout'].to(dtype))
    return dict(y=_f64(y), dx=_f64(x.grad), dw=_f64(w.grad), db=_f64(b.grad))


# ---- family 3: the up-sampler block through ops.DeconvBNActFn ----------------------------------------------------------------------
# (32, 32): da_deconv_k2s2_bn_bwd (deconv_bn_bwd_kernel) in train mode;  (16, 16), (64, 32), (48, 16): the three-call backward on the matrix path;
# (6, 5): the direct kernels, *stats_nparts == 0, da_bn_train_stats runs
UP_CH = [(32, 32), (6, 5), (16, 16), (32, 32), (64, 32), (48, 16), (32, 32)]
# coarse shapes of the fused kernel's chunk walk: one partial chunk; 31, 32, 33 voxels; 512; 16384 = 512 chunks, the last with one chunk per workgroup;
# 16695 = 522 chunks, workgroups 0 ... 9 walk two; 36378 = 1137 chunks, two or three per workgroup, ragged last chunk
UP_SHAPES = [(1, 1, 1, 5), (1, 1, 1, 31), (1, 4, 2, 4), (1, 1, 3, 11), (1, 4, 8, 16), (1, 16, 32, 32), (1, 7, 45, 53), (2, 9, 43, 47)]
UP_CHUNKS = [1, 1, 1, 1, 1, 1, 2, 3]
UP = st.fixed_dictionaries(dict(ch=st.sampled_from(UP_CH), n=st.integers(1, 2), d=st.integers(1, 5), h=st.integers(1, 6), w=st.integers(1, 9),
                                train=st.sampled_from([True, True, False]), slope=st.sampled_from([0.0, 0.01]), lazy=st.booleans(), neg=st.booleans(),
                                chain=st.booleans(), sd=st.integers(0, 999))).map(
    lambda c: dict({k: v for k, v in c.items() if k not in ('n', 'd', 'h', 'w')}, dims=(c['n'], c['d'], c['h'], c['w']), chain=c['chain'] and c['ch'] == (32, 32),
                   lazy=c['lazy'] or (c['chain'] and c['ch'] == (32, 32))))      # (the consumer takes the up-block's output as a LazyAct)
CHAIN_SKIP, CHAIN_COUT = 16, 16      # the consumer whose data gradient hands the BatchNorm-backward sums over: SegBlock(32 lazy + 16 skip -> 16), ops.ConvBNActFn


def _up(ch, i, dims, train=True, chain=False, lazy=None):
    return dict(ch=ch, dims=dims, train=train, slope=_cyc([0.01, 0.0], i), lazy=chain or ((i // 2) % 2 == 1 if lazy is None else lazy), neg=i % 3 == 1, chain=chain, sd=200 + i, fixed=True)


UP_PINNED = ([_up((32, 32), i, s) for i, s in enumerate(UP_SHAPES)] + [_up((32, 32), 10, (1, 1, 3, 11), train=False, lazy=False), _up((32, 32), 11, (1, 4, 8, 16), train=False, lazy=False)] +
             [_up(ch, 20 + i, _cyc([(1, 3, 5, 7), (2, 2, 3, 5), (2, 2, 3, 5), (1, 3, 5, 7)], i), train=i < 6) for i, ch in enumerate([(16, 16), (64, 32), (48, 16), (6, 5)] * 2)] +
             [_up((32, 32), 30, (1, 1, 3, 11), chain=True), _up((32, 32), 31, (1, 4, 8, 16), chain=True)])


# Tensors of more than BAND_LARGE elements (the three chunk-walk shapes: 4.2 - 9.3 M elements): with z centred at 0 an element falls inside the guard band with
# probability 2 G max|z| pdf(0) = 7.6e-5 (measured: 711 of 9.3 M), far above the cap of 64 per tensor.  The cap is kept; the inputs move, as block_cases.POOL_BETA0
# does: beta is centred at 3 and gamma drawn as 1 + 0.1 n, so a channel's zero crossing lies 2.4 - 4 standard deviations out and about 1 element in 500 is negative.
BAND_LARGE, LARGE_BETA0, LARGE_GSD = 1000000, 3.0, 0.1


def up_params(cin, cout, sd, neg, large=False):
    gamma = 1.0 + (LARGE_GSD if large else 0.3) * nrm((cout,), sd + 2)
    if neg:
        gamma[1 % cout] = -0.8
    return dict(w=nrm((cin, cout, 2, 2, 2), sd, 0.2), b=nrm((cout,), sd + 1, 0.1), gamma=gamma, beta=(LARGE_BETA0 if large else 0.0) + nrm((cout,), sd + 3, 0.2), rm=nrm((cout,), sd + 4, 0.1),
                rv=nrm((cout,), sd + 5).abs() * 0.5 + 0.5, cin=cin, cout=cout)


def build_up(case):
    (cin, cout), (n, d, h, w) = case['ch'], case['dims']
    if not case.get('fixed'):       # train mode: M_MIN fine voxels per channel; every decided tensor BAND_ELEMS elements
        lo = max(_cdiv(M_MIN, 8) if case['train'] else 1, _cdiv(BAND_ELEMS, 8 * min(cout, CHAIN_COUT if case['chain'] else cout)))
        while n * d * h * w < lo:
            w += 1
    sd = 100 * case['sd']
    fine = (n, 2 * d, 2 * h, 2 * w)
    inp = dict(x=nrm((n, cin, d, h, w), sd + 10), p=up_params(cin, cout, sd, case['neg'], large=8 * n * d * h * w * cout > BAND_LARGE), gout=nrm((n, cout) + fine[1:], sd + 12), train=case['train'],
               slope=case['slope'], lazy=case['lazy'], chain=case['chain'], dims=(n, d, h, w), cin=cin, cout=cout)
    if case['chain']:
        inp.update(skip=nrm((n, CHAIN_SKIP) + fine[1:], sd + 11), p2=bc.block_params(cout + CHAIN_SKIP, CHAIN_COUT, sd + 20), slope2=0.01 - case['slope'],
                   gout=nrm((n, CHAIN_COUT) + fine[1:], sd + 12))
    return inp


class _UpBlock(bc._Block):
    """ConvTranspose3d(k2, s2) -> BatchNorm -> activation of the reference, its leaves in `dtype` (block_cases._Block with the up-sampler's convolution)."""

    def __call__(self, x, decided, counts):
        y = F.conv_transpose3d(x, self.w, self.b, stride=2)
        y.retain_grad()
        self.y = y
        z = F.batch_norm(y, self.rm, self.rv, self.gamma, self.beta, self.train, MOMENTUM, EPS)
        self.act = activate(z, self.slope, decided, counts)
        return self.act


def ref_up(inp, dtype, decided=None):
    """decided: {'act0': the up-block's activated output of the tested side [, 'act1': the consumer's]} (None: own decisions)."""
    counts = []
    x = _leaf(inp['x'], dtype)
    up = _UpBlock(inp['p'], dtype, inp['train'], inp['slope'])
    a = up(x, decided['act0'] if decided else None, counts)
    res = dict(act0=a.detach())
    out = a
    if inp['chain']:
        skip = _leaf(inp['skip'], dtype)
        blk = bc._Block(inp['p2'], dtype, inp['train'], inp['slope2'])
        out = blk(torch.cat((a, skip), 1), decided['act1'] if decided else None, counts)
        res['act1'] = out.detach()
    out.backward(inp['gout'].to(dtype))
    res.update(out=_f64(out), dx=_f64(x.grad), band=counts)
    up.results(0, res)
    if inp['chain']:
        res['dskip'] = _f64(skip.grad)
        blk.results(1, res)
    return res


# ---- family 4: the bf16 twins through the C ABI --------------------------------------------------------------------------------------
# (Cin / 16, Cout / 16): pair loads for even tile counts, single loads for 3; rows / shapes: the ragged ones of families 1 and 2
BF_ROWS = [1, 17, 65, 255, 257, 105]
BF_SHAPES = [(1, 1, 1, 3), (1, 2, 3, 1), (2, 3, 5, 7), (1, 1, 1, 257), (1, 4, 8, 8), (1, 3, 5, 7)]
BF_PINNED = ([dict(cin=ci, cout=co, m=_cyc(BF_ROWS, i), dims=_cyc(BF_SHAPES, i), sd=300 + i) for i, (ci, co) in enumerate(TILE_PAIRS)] +
             # one multi-step weight-gradient shape each on the pair path (12 voxels per wave) and on the single-load path (48, 48): the 1x1 form has O = 2304 and
             # 1024 blocks, 12 per wave; the up-sampler form O = 18432 and 910 blocks, 8 per wave
             [dict(cin=32, cout=32, m=32769, dims=(2, 19, 29, 31), sd=320), dict(cin=48, cout=48, m=32771, dims=(1, 11, 37, 41), sd=321)] +
             # host-tiled layers with a 48-channel slice: the slice loop's bf16 pointer offsets (2 bytes per channel) with the tile-count-3 instantiations
             [dict(cin=48, cout=96, m=105, dims=(1, 3, 5, 7), sd=322), dict(cin=112, cout=64, m=257, dims=(2, 3, 5, 7), sd=323)])
BF_DECLINED = [(6, 5), (16, 5), (40, 16)]


def build_bf(c):
    """(family-1 inputs with M = c['m'] rows, family-2 inputs at c['dims']) whose activations hold bf16 values; the logit gradient of the 1x1 head stays fp32"""
    i1 = build_c1(dict(cin=c['cin'], cout=c['cout'], dims=(1, 1, 1, c['m']), pro=None, sd=c['sd'], fixed=True))
    i1['x'] = to_bf16(i1['x'])
    i2 = build_d2(dict(cin=c['cin'], cout=c['cout'], dims=c['dims'], sd=c['sd'], fixed=True))
    i2['x'], i2['gout'] = to_bf16(i2['x']), to_bf16(i2['gout'])
    return i1, i2


def to_bf16(t):
    """round to nearest even, widened again: the values a bf16 tensor holds"""
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_close(what, got, ref, tol):
    """per element |got - ref| <= 2^-8 |ref| + tol max|ref| (one bf16 spacing + the fp32 family's tolerance for the quantity; derived, not measured);
    records the largest |got - ref| / (2^-8 |ref| + tol max|ref|)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    e = float(((got - ref).abs() / (BF16_EPS * ref.abs() + tol * ref.abs().max()).clamp_min(1e-300)).max())
    note('bf16', what + ' (stored bf16, fraction of its bound)', e)
    assert e <= 1.0, 'bf16 %s: %.3f of the bound' % (what, e)
