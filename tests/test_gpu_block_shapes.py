"""Randomised float64 parity for the conv -> BatchNorm -> LeakyReLU block on its shipped route (ops.LAZY_BN, ops.FUSE_BN_BWD_STATS, matrix mode
'fp32_split'): da_conv3d_k3_fwd_bnstats + da_bn_train_stats_from_partials, da_conv3d_k3_fwd_pro / _wgrad_pro (ops.LazyAct), da_conv3d_k3_dgrad_bst +
da_bn_act_bwd_dbias_pre, da_maxpool2_fwd_pro / da_maxpool2_bwd_bst and da_head_dice_bwd_bst.

Reference: plain torch in float64 on the widened fp32 inputs (F.conv3d / F.conv_transpose3d of the concatenated inputs, F.batch_norm with the module's
momentum and eps, the activation, F.max_pool3d), gradients by autograd with a drawn output gradient, running statistics compared after the call.  The
device side goes through the public surfaces (modules.SegBlock with lazy_out= and ops.LazyAct, ops.ConvBNActFn, ops.MaxPool2SkipFn); the raw C ABI only
where the epilogue sums themselves are under test.  Cases, builders, references, the guard-band rule for the activation / arg-max kinks and the tolerances
live in tests/block_cases.py; every family runs `block_cases.run_cases`: the pinned examples that reach each launcher branch by construction, then 60
derandomised hypothesis examples.  tests/test_block_reference.py runs the same examples on the CPU and shows the fp32 oracle within a quarter of each
tolerance and the guard band under its cap, so a tolerance here is a statement about the kernel.

Launcher branch <- value
  shapes (block_cases.SHAPES_PINNED, every family): one 4 x 8 x 16 tile; 5 x 9 x 17 (one voxel over a tile on every axis); 1 x 1 x 128; W = 1 (9 x 19 x 1);
      N = 2 with three tiles per sample; 1, 7, 8, 9, 17 tiles -> nblocks = min(512 / gy, ntiles) & ~7 = 1, 7, 8, 8 walking 9, 16 walking 17.
      Drawn: N 1 ... 2, D 1 ... 9, H 1 ... 19, W 1 ... 35, W widened until M >= 128 (train) and every decided tensor has 4000 elements (straddles the forward tile and the weight gradient's two z planes); family 3 even sizes.
  family 1 `block` (C1, C2): pick_ck = 16 <- (16, 0), (32, 16), (16, 16), (64, 32);  pick_ck = 8 <- (8, 0), (8, 16), (24, 0);  pick_ck = 0 (direct kernels,
      *stats_nparts == 0, da_bn_train_stats runs) <- (1, 0), (3, 0), (12, 4).  Cout on the matrix path: 8, 16, 32 (one or two N-tiles), 12 (ragged N-tile),
      48 (three N-tiles, two per workgroup), 64;  3, 5 leave it.  train / eval, slope 0 / 0.01, Conv3d / ConvTranspose3d(k3, s1, p1) weights.
      N-tiles per workgroup (block_cases.launcher_nrep restates conv3_mfma_fwd_impl's choice; below 129 tiles it is 1 whatever Cout is, so the drawn shapes never
      leave it): NREP = 2 <- Cout 32 at 257 tiles, 48 at 171, 64 at 129 (block_cases.NREP_PINNED: 1 x 3 x 4112 / 2725 / 2050, ragged), with statistics, with the
      prologue (family 2: block-2 Cout 32 and 64 behind a LazyAct), plain (eval), with 16-channel chunks, and as a data gradient split over two inputs (16 + 16);
      NREP = 3 <- fp32 mode, Cout 48 at 341 tiles (no statistics epilogue: da_bn_train_stats must run, and *stats_nparts == 0 in family 4).
      Asserted with _native.CallProfiler: da_bn_train_stats did NOT run wherever the epilogue delivers the statistics, and did run elsewhere.
  family 2 `chain`, block-1 Cout -> block 2 (block_cases.CHAIN_PINNED; per example the profiler shows which entries ran):
      fwd_pro + wgrad_pro + dgrad_bst + bn_act_bwd_dbias_pre <- block-1 Cout 8, 16, single input, block-2 Cout 8, 16, 32
      the two-launch concat form of dgrad_bst                  <- block-1 Cout 32 lazy + a 16-channel skip, block-2 Cout 16
      dgrad_bst not taken (da_conv3d_k3_dgrad + stand-alone sums) <- block-1 Cout 4; block-1 Cout 32 single input; block-2 Cout 12; the lazy tensor second
      fwd_pro declined, ops._apply_pro                          <- block-2 Cout 3, 4; block-1 Cout 4, 12 (pick_ck = 0)
      eval mode: da_bn_eval_affine, the sums handed over and dropped, da_bn_act_bwd_dbias with train = 0.
      Drawn: (block-1 Cout, form, skip, block-2 Cout) from block_cases.CHAIN_ROWS, half of them the two hand-over routes (the concat form 3 of 18), so the
      hand-over through ops._bwd_stats runs on ragged drawn shapes; the concat form is also pinned at 5 x 9 x 17 and N = 2.
      Every example runs with ops.FUSE_BN_BWD_STATS on and off, both against float64; `not ops._bwd_stats` after every backward.
  family 3 `chain_pool`: C = 8, 16, 32 -> da_maxpool2_fwd_pro + da_maxpool2_bwd_bst + bn_act_bwd_dbias_pre;  C = 12 -> da_maxpool2_bwd_bst declines,
      da_maxpool2_bwd[_add] + stand-alone sums;  with / without a gradient on the skip branch;  a negative-gamma channel (raw order reversed).
  family 4 `sums` (C ABI): da_conv3d_k3_fwd_bnstats for every matrix-path channel class; da_conv3d_k3_dgrad_bst single input C1 = 8, 12, 16 and 32 (two
      N-tiles, reached by no caller) and concat 32 + 16; DA_ERR_UNSUPPORTED with *bst_n == 0 for C1 = 4, 20, 16 + 16, matrix mode fp32, bst_cap 511;
      da_head_dice_bwd_bst Cin 16, C 16 / 32, V = 105, 256, 693; da_bn_train_stats_from_partials nparts 1, 8, 512.

Worst case over all examples on an MI355X (distance from float64: tensors max(rel-l2, max-abs / max|ref|); 'db, train': max |db| / sum |dz_ref|; sums: largest
per-channel error / sum |term|), the fp32 CPU oracle's worst case on the same examples (tests/test_block_reference.py), the ceiling (what the existing fp32
comparisons assert, block_cases.CEIL) and what is asserted.  Device: the larger of the split-mode, fp32-mode and unfused runs (they differ by < 1.5 x).
  family / quantity        device worst   fp32 oracle worst   ceiling   asserted
  block  output               1.6e-6         6.8e-7            2e-5      2e-5    (less than 10 x below the ceiling: stays)
  block  running stats        1.0e-6         2.2e-7            1e-5      1e-5    (stays)
  block  dx1, dx2             1.8e-6         8.2e-7            2e-4      7.2e-6
  block  dw                   6.9e-7         7.0e-7            1e-4      5.6e-6
  block  db, eval             2.2e-7         6.4e-7            1e-4      5.2e-6
  block  db, train            2.4e-8         5.4e-8            1e-5      4.4e-7
  block  d_gamma              1.5e-6         1.2e-6            2e-4      9.9e-6
  block  d_beta               1.4e-7         7.1e-7            2e-4      5.8e-6
  chain  output               1.1e-6         1.1e-6            2e-5      2e-5    (stays)
  chain  running stats        1.7e-7         1.4e-7            1e-5      1e-5    (stays)
  chain  dx, d_skip           1.3e-6         9.1e-7            2e-4      7.4e-6
  chain  dw                   8.8e-7         1.4e-6            1e-4      1e-4    (8 x oracle = 1.1e-5: stays)
  chain  db, eval             5.7e-7         3.1e-7            1e-4      2.5e-6
  chain  db, train            1.9e-8         5.4e-8            1e-5      4.4e-7
  chain  d_gamma              1.5e-6         1.9e-6            2e-4      1.5e-5
  chain  d_beta               1.4e-6         1.4e-6            2e-4      1.1e-5
  pool   output               1.3e-6         1.3e-6            2e-5      2e-5    (stays)
  pool   running stats        2.5e-7         1.6e-7            1e-5      1e-5    (stays)
  pool   dx                   1.1e-6         9.4e-7            2e-4      7.6e-6
  pool   dw                   9.3e-7         1.5e-6            1e-4      1e-4    (stays)
  pool   db, eval             1.7e-6         6.4e-7            1e-4      6.7e-6
  pool   db, train            1.5e-8         4.1e-8            1e-5      3.4e-7
  pool   d_gamma              2.0e-6         2.6e-6            2e-4      2e-4    (8 x oracle = 2.1e-5: stays)
  pool   d_beta               1.4e-5         1.2e-5            2e-4      9.4e-5  (8 x oracle, see block_cases.TOL)
  sums   y (fwd_bnstats)      2.0e-6         1.1e-6            1e-4      9.1e-6
  sums   dx (dgrad_bst)       7.8e-7         7.8e-7            1e-4      6.3e-6
  sums   sum y / sum y^2      5.8e-8 / 1.2e-7   1.9e-7         1e-6      1e-6    (stays)
  sums   sum dz / dz (y - mean), dgrad_bst   1.9e-7 / 9.1e-8   -   1e-6   1e-6   (stays)
  sums   sum dz / dz (x - mean), head        3.6e-8 / 3.2e-8   -   1e-6   1e-6   (stays)
  sums   head dx, dW, db vs da_head_dice_bwd 0 (bit-identical)  -   1e-4   1e-4   (as test_fused_head_softmax_dice_vs_torch_cpu)
  sums   from_partials stats / running       9.3e-8 / 8.5e-8    -   2e-5 / 1e-5   4.8e-7 (8 x 2^-24, block_cases.TOL)
Asserted = max(4 x device worst, 8 x fp32 oracle worst) rounded up to two digits wherever that is more than 10 x below the ceiling, else the ceiling.
Device against oracle: in no quantity is the device further from float64 than the fp32 oracle by more than the split arithmetic's per-product bound (2^-21 + 2^-22
against fp32's 2^-24) explains -- y 1.7 x, running statistics 4.6 x (they inherit y's error with one sign), dx 2.2 x, the eval-mode bias
gradient 2.6 x; everything else is within 1.3 x of the oracle.  No finding.  Guard band: at most 31 elements of a tensor per example (a 393 600-element tensor; cap:
0.1 % and 64).  Total time of this file on one MI355X: 12 s of pytest time, the slowest test 2.5 s.

What the issue's route table says and the launcher does not: block-1 Cout = 12 is listed on the full prologue route, but pick_ck(12, 0) = 0, so
da_conv3d_k3_fwd_pro declines a 12-channel input and ops materialises it (asserted as such); da_conv3d_k3_dgrad_bst with C1 = 12 is reached through the C ABI (family 4).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import block_cases as bc
from test_gpu_ops import cl, dev

pytestmark = pytest.mark.gpu


class _Profile(object):
    """_native.CallProfiler around a block of calls; count(name) = how often the C entry was CALLED (a declined call counts)."""

    def __init__(self, names):
        from deepatlas_amd import _native as nat
        self.nat, self.prof = nat, nat.CallProfiler(names)

    def __enter__(self):
        self.prev, self.nat.profiler = self.nat.profiler, self.prof
        return self

    def __exit__(self, *exc):
        self.nat.profiler = self.prev

    def count(self, name):
        return sum(len(v) for k, v in self.prof.records.items() if k[0] == name)


class _mode(object):
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from deepatlas_amd import ops
        self.prev = ops.set_matrix_precision(self.mode)

    def __exit__(self, *exc):
        from deepatlas_amd import ops
        ops.set_matrix_precision(self.prev)


def _cpu(t):
    return t.detach().cpu() if t is not None else None


# ---- family 1 --------------------------------------------------------------------------------------------------------------------
def _run_block(inp):
    from deepatlas_amd import ops
    p = inp['p']
    x1 = cl(inp['x1']).requires_grad_(True)
    x2 = cl(inp['x2']).requires_grad_(True) if inp['x2'] is not None else None
    w, b, gamma, beta = (p[k].to(dev()).requires_grad_(True) for k in ('w', 'b', 'gamma', 'beta'))
    rm, rv = p['rm'].to(dev()), p['rv'].to(dev())
    out = ops.ConvBNActFn.apply(x1, x2, w, b, gamma, beta, rm, rv, inp['train'], bc.MOMENTUM, bc.EPS, inp['slope'], inp['transposed'])
    out.backward(cl(inp['gout']))
    return dict(out=_cpu(out), act0=_cpu(out), dx1=_cpu(x1.grad), dx2=_cpu(x2.grad) if x2 is not None else None, dw0=_cpu(w.grad), db0=_cpu(b.grad),
                dgamma0=_cpu(gamma.grad), dbeta0=_cpu(beta.grad), rm0=_cpu(rm), rv0=_cpu(rv))


@pytest.mark.parametrize('mode', ['fp32_split', 'fp32'])
def test_block_random_shapes(mode):
    """ops.ConvBNActFn, every quantity against float64: output, running statistics, dx1, dx2, dw, db, d_gamma, d_beta.  'fp32': the dense kStats kernels."""
    family = 'block' if mode == 'fp32_split' else 'block fp32'

    def body(case):
        inp = bc.build_block(case)
        with _Profile(['da_bn_train_stats', 'da_bn_train_stats_from_partials', 'da_conv3d_k3_fwd_bnstats']) as prof:
            got = _run_block(inp)
        ref = bc.ref_block(inp, torch.float64, decided=got)
        bc.check_band(ref['band'])
        bc.compare(family, got, ref, bc.TOL['block'])
        if case['train']:
            assert prof.count('da_conv3d_k3_fwd_bnstats') == 1
            if not bc.stats_from_epilogue(case):
                assert prof.count('da_bn_train_stats') == 1 and prof.count('da_bn_train_stats_from_partials') == 0, case
            elif bc.launcher_nrep(bc.ntiles(*inp['dims']), case['cout'], mode) == 3:      # (fp32 mode, three N-tiles in one workgroup: no statistics epilogue)
                assert prof.count('da_bn_train_stats') == 1 and prof.count('da_bn_train_stats_from_partials') == 0, case
            else:
                assert prof.count('da_bn_train_stats') == 0 and prof.count('da_bn_train_stats_from_partials') == 1, case
        else:
            assert prof.count('da_conv3d_k3_fwd_bnstats') == 0 and prof.count('da_bn_train_stats') == 0
    with _mode(mode):
        bc.run_cases(bc.BLOCK, body, pinned=bc.BLOCK_PINNED)


# ---- families 2 and 3 ------------------------------------------------------------------------------------------------------------
def _seg_block(p, slope, train):
    from deepatlas_amd.lib.network_factory.modules import SegBlock
    m = SegBlock(p['cin'], p['cout'], batchnorm=True, act='ReLU' if slope == 0.0 else 'LeakyReLU')
    assert m.slope == slope
    with torch.no_grad():
        m.conv.weight.copy_(p['w']); m.conv.bias.copy_(p['b'])
        m.BN.weight.copy_(p['gamma']); m.BN.bias.copy_(p['beta']); m.BN.running_mean.copy_(p['rm']); m.BN.running_var.copy_(p['rv'])
    return m.to(dev()).train(train)


def _block_results(m, i, res):
    res['dw%d' % i], res['db%d' % i], res['dgamma%d' % i], res['dbeta%d' % i] = (_cpu(t.grad) for t in (m.conv.weight, m.conv.bias, m.BN.weight, m.BN.bias))
    res['rm%d' % i], res['rv%d' % i] = _cpu(m.BN.running_mean), _cpu(m.BN.running_var)


def _activated(lazy):
    """The activated tensor a LazyAct stands for, as the device forms it (ops.materialize: da_bn_act_fwd, the expression of the input prologue)."""
    from deepatlas_amd import ops
    with torch.no_grad():
        return _cpu(ops.materialize(ops.LazyAct(lazy.raw.detach(), lazy.scale, lazy.shift, lazy.slope)))


CHAIN_ENTRIES = ['da_conv3d_k3_fwd_pro', 'da_conv3d_k3_wgrad_pro', 'da_conv3d_k3_dgrad_bst', 'da_bn_act_bwd_dbias_pre', 'da_bn_act_bwd_dbias', 'da_bn_act_fwd',
                 'da_conv3d_k3_wgrad', 'da_conv3d_k3_dgrad', 'da_bn_eval_affine', 'da_bn_train_stats']


def _run_chain(inp):
    from deepatlas_amd import ops
    blocks = [_seg_block(p, s, inp['train']) for p, s in zip(inp['blocks'], inp['slopes'])]
    x = cl(inp['x']).requires_grad_(True)
    skip = cl(inp['skip']).requires_grad_(True) if inp['skip'] is not None else None
    third = len(blocks) == 3
    with _Profile(CHAIN_ENTRIES) as prof:
        l0 = blocks[0](x, lazy_out=True)
        args = (l0,) if skip is None else ((l0, skip) if inp['form'] == 'lazy_skip' else (skip, l0))
        a = blocks[1](*args, lazy_out=third)
        l1 = a
        if third:
            a = blocks[2](l1)
        a.backward(cl(inp['gout']))
        torch.cuda.synchronize()
    _no_stale_sums()
    res = dict(out=_cpu(a), dx=_cpu(x.grad), dskip=_cpu(skip.grad) if skip is not None else None, act0=_activated(l0))
    res['act1'] = _activated(l1) if third else _cpu(a)
    if third:
        res['act2'] = _cpu(a)
    for i, m in enumerate(blocks):
        _block_results(m, i, res)
    return res, prof


def _no_stale_sums():
    """`not ops._bwd_stats` after a backward; a stale entry is dropped before the assertion so that it cannot be consumed by a later test."""
    from deepatlas_amd import ops
    stale = [(v[3], v[4]) for v in ops._bwd_stats.values()]
    ops.drop_bwd_stats()
    assert not stale, 'BatchNorm-backward sums handed over and never consumed: (M, C) = %r' % (stale,)


def _same_decisions(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if k.startswith('act'))


@pytest.mark.parametrize('mode', ['fp32_split', 'fp32'])
def test_chain_random_shapes(mode):
    """Two or three SegBlocks linked by LazyAct, every gradient of every block, the output and the running statistics against float64; in the shipped mode each
    example with ops.FUSE_BN_BWD_STATS on and off (the unfused run is held to float64 too, not to the fused one), and the pinned examples show their route."""
    from deepatlas_amd import ops
    family = 'chain' if mode == 'fp32_split' else 'chain fp32'

    def body(case):
        inp = bc.build_chain(case)
        ref = None
        for fuse in ((True, False) if mode == 'fp32_split' else (True,)):
            ops.FUSE_BN_BWD_STATS = fuse
            got, prof = _run_chain(inp)
            if ref is None or not _same_decisions(got, ref_from):
                ref, ref_from = bc.ref_chain(inp, torch.float64, decided=got), got
                bc.check_band(ref['band'])
            bc.compare(family if fuse else family + ' unfused', got, ref, bc.TOL['chain'])
            route = case.get('route')
            if route is None:
                continue
            fwd_pro, wgrad_pro, bst = route
            bst = bst and fuse and mode == 'fp32_split'
            n = {k: prof.count(k) for k in CHAIN_ENTRIES}
            assert n['da_conv3d_k3_fwd_pro'] == 1 and n['da_bn_act_fwd'] == (1 if fwd_pro else 2), (case, n)          # (2: the materialised output + ops._apply_pro)
            assert n['da_conv3d_k3_wgrad_pro'] == int(wgrad_pro) and n['da_conv3d_k3_wgrad'] == 2 - int(wgrad_pro), (case, n)
            assert n['da_conv3d_k3_dgrad'] == 2 - int(bst), (case, n)
            assert (n['da_conv3d_k3_dgrad_bst'] > 0) >= bst, (case, n)
            pre = int(bst and case['train'])
            assert n['da_bn_act_bwd_dbias_pre'] == pre and n['da_bn_act_bwd_dbias'] == 2 - pre, (case, n)
            assert n['da_bn_eval_affine'] == (0 if case['train'] else 2) and (case['train'] or n['da_bn_train_stats'] == 0), (case, n)
    prev = ops.FUSE_BN_BWD_STATS
    try:
        with _mode(mode):
            bc.run_cases(bc.CHAIN, body, pinned=bc.CHAIN_PINNED)
    finally:
        ops.FUSE_BN_BWD_STATS = prev


POOL_ENTRIES = ['da_maxpool2_fwd_pro', 'da_maxpool2_fwd', 'da_maxpool2_bwd_bst', 'da_maxpool2_bwd', 'da_maxpool2_bwd_add', 'da_bn_act_bwd_dbias_pre']


def _run_pool(inp):
    from deepatlas_amd import ops
    b0, bs, bp = (_seg_block(p, inp['slope'], inp['train']) for p in inp['blocks'])
    x = cl(inp['x']).requires_grad_(True)
    with _Profile(POOL_ENTRIES) as prof:
        lz = b0(x, lazy_out=True)
        skip, pooled = ops.MaxPool2SkipFn.apply(lz.raw, lz.scale, lz.shift, lz.slope)
        outp = bp(pooled)
        loss = (outp * cl(inp['gp'])).sum()
        outs = None
        if inp['skip_grad']:
            outs = bs(skip)
            loss = loss + (outs * cl(inp['gs'])).sum()
        loss.backward()
        torch.cuda.synchronize()
    _no_stale_sums()
    res = dict(outp=_cpu(outp), outs=_cpu(outs), dx=_cpu(x.grad), act0=_cpu(skip), act1=_cpu(outs), act2=_cpu(outp))
    _block_results(b0, 0, res)
    _block_results(bp, 2, res)
    if outs is not None:
        _block_results(bs, 1, res)
    return res, prof


def test_chain_pool_random_shapes():
    """SegBlock(lazy) -> ops.MaxPool2SkipFn(raw, scale, shift, slope) -> one SegBlock per output, with and without a gradient on the skip branch, with
    ops.FUSE_BN_BWD_STATS on and off, against float64 (the pool's gradient routed as block_cases.pool says)."""
    from deepatlas_amd import ops

    def body(case):
        inp = bc.build_pool(case)
        ref = None
        for fuse in (True, False):
            ops.FUSE_BN_BWD_STATS = fuse
            got, prof = _run_pool(inp)
            if ref is None or not _same_decisions({k: v for k, v in got.items() if v is not None}, ref_from):
                ref, ref_from = bc.ref_pool(inp, torch.float64, decided=got), got
                bc.check_band(ref['band'])
            bc.compare('chain_pool' if fuse else 'chain_pool unfused', got, ref, bc.TOL['chain_pool'])
            n = {k: prof.count(k) for k in POOL_ENTRIES}
            plain = n['da_maxpool2_bwd'] + n['da_maxpool2_bwd_add']
            assert n['da_maxpool2_fwd_pro'] == 1 and n['da_maxpool2_fwd'] == 0, (case, n)
            if not fuse:
                assert n['da_maxpool2_bwd_bst'] == 0 and plain == 1 and n['da_bn_act_bwd_dbias_pre'] == 0, (case, n)
            elif case['c'] == 12:                          # C / 4 = 3 is no power of two: declined, the plain backward on the activated tensor
                assert n['da_maxpool2_bwd_bst'] == 1 and plain == 1 and n['da_bn_act_bwd_dbias_pre'] == 0, (case, n)
            else:
                assert n['da_maxpool2_bwd_bst'] == 1 and plain == 0 and n['da_bn_act_bwd_dbias_pre'] == int(case['train']), (case, n)
    prev = ops.FUSE_BN_BWD_STATS
    try:
        with _mode('fp32_split'):
            bc.run_cases(bc.POOL, body, pinned=bc.POOL_PINNED)
    finally:
        ops.FUSE_BN_BWD_STATS = prev


# ---- family 4: the epilogue sums through the C ABI ---------------------------------------------------------------------------------
def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().to(dev()) if t is not None else None


def _tio(w):
    """[Cout][Cin][3,3,3] -> the kernels' [27][Cin][Cout]"""
    return w.permute(2, 3, 4, 1, 0).reshape(27, w.shape[1], w.shape[0]).contiguous().to(dev())


def _sum_close(what, got, terms, undecided=None):
    """Column sums against float64; `undecided` (same shape as terms): what each term may move by if its activation decision falls the other way (guard band)."""
    assert bool(torch.isfinite(got).all()), what
    t = terms.double().cpu().reshape(-1, terms.shape[-1])
    slack = undecided.double().cpu().reshape(-1, terms.shape[-1]).abs().sum(0) if undecided is not None else 0.0
    e = float((((got.double().cpu() - t.sum(0)).abs() - slack).clamp_min(0.0) / t.abs().sum(0).clamp_min(1e-300)).max())
    bc.note('sums', what, e)
    assert e < bc.TOL['sums']['sum'], 'sums %s: %.3e of sum|term| (tolerance %.1e)' % (what, e, bc.TOL['sums']['sum'])


def _bst_terms(dx, y, stats, slope):
    """float64 (dz, dz (y - mean)), dz = dx act'(y scale + shift), channels last; dx, y: the device's tensors, stats = [mean | rstd | scale | shift]."""
    y, st, dx = y.double().cpu(), stats.double().cpu(), dx.double().cpu()
    z = y * st[2] + st[3]
    dz = dx * torch.where(z > 0, 1.0, float(slope))
    # the kernel decides act' on its fp32 z: inside the guard band (block_cases.G) either decision is taken as right, the sums may differ by dx (1 - slope) there
    band = z.abs() < bc.G * z.abs().max()
    assert int(band.sum()) <= max(1, min(bc.BAND_FRAC * band.numel(), bc.BAND_MAX)), int(band.sum())      # (these shapes are not widened: one voxel of a small tensor may fall in)
    und = torch.where(band, dx * (1.0 - float(slope)), torch.zeros_like(dx))
    return dz, dz * (y - st[0]), und, und * (y - st[0])


@pytest.mark.parametrize('mode', ['fp32_split', 'fp32'])
def test_forward_statistics_epilogue(mode):
    """da_conv3d_k3_fwd_bnstats: partials[:n].sum(0) against the float64 sum y and sum y^2 of the device's OWN output (the epilogue apart from the
    convolution's rounding), and that output against float64."""
    from deepatlas_amd import _native as nat
    call, ptr = nat.call, nat.ptr

    def body(case):
        inp = bc.build_sums(case)
        N, D, H, W = inp['dims']
        a1, a2, w, b = _ndhwc(inp['x1']), _ndhwc(inp['x2']), _tio(inp['w']), inp['b'].to(dev())
        C1, C2, Cout = a1.shape[-1], (a2.shape[-1] if a2 is not None else 0), w.shape[-1]
        y = torch.empty((N, D, H, W, Cout), device=dev())
        pbuf = torch.full((512, 2, Cout), float('nan'), dtype=torch.float64, device=dev())
        n = ctypes.c_int(0)
        wp, wn = nat.workspace.get(nat.lib().da_conv3d_k3_ws_bytes(N, D, H, W, C1 + C2, Cout, 1), dev())
        call('da_conv3d_k3_fwd_bnstats', ptr(a1), C1, ptr(a2), C2, ptr(w), ptr(b), ptr(y), N, D, H, W, Cout, 1, ptr(pbuf), 512, ctypes.byref(n), wp, wn, nat.stream())
        torch.cuda.synchronize()
        y64, _ = bc.ref_sums(inp, torch.float64)
        bc.close('sums', 'y', y.permute(0, 4, 1, 2, 3), y64, bc.TOL['sums']['y'])
        tiles = bc.ntiles(N, D, H, W)
        if bc.launcher_nrep(tiles, Cout, mode) == 3:
            assert n.value == 0, case                       # (fp32 mode, three N-tiles per workgroup: no statistics epilogue, the caller runs da_bn_train_stats)
            return
        assert 0 < n.value <= min(512, tiles) and (n.value == tiles or n.value % 8 == 0), (case, n.value, tiles)
        got = pbuf[:n.value].sum(0)
        yd = y.double()
        _sum_close('fwd sum y', got[0], yd)
        _sum_close('fwd sum y^2', got[1], yd * yd)
    with _mode(mode):
        bc.run_cases(bc.SUMS, body, pinned=bc.SUMS_PINNED)


def _dgrad_bst(inp, mode_ok=True, bst_cap=512):
    from deepatlas_amd import _native as nat
    ptr = nat.ptr
    N, D, H, W = inp['dims']
    g1, g2 = inp['g']
    dy, w, yraw, stats = _ndhwc(inp['dy']), _tio(inp['wl']), _ndhwc(inp['yraw']), inp['stats'].to(dev())
    Cout = dy.shape[-1]
    dx1 = torch.empty((N, D, H, W, g1), device=dev())
    dx2 = torch.empty((N, D, H, W, g2), device=dev()) if g2 else None
    bst = torch.full((512, 2, g1), float('nan'), dtype=torch.float64, device=dev())
    nb = ctypes.c_int(7)
    wp, wn = nat.workspace.get(nat.lib().da_conv3d_k3_ws_bytes(N, D, H, W, g1 + g2, Cout, 1), dev())
    ok = nat.call_supported('da_conv3d_k3_dgrad_bst', ptr(dy), ptr(w), ptr(dx1), g1, ptr(dx2), g2, N, D, H, W, Cout, ptr(yraw), ptr(stats), float(inp['slope']),
                            ptr(bst), bst_cap, ctypes.byref(nb), wp, wn, nat.stream())
    torch.cuda.synchronize()
    return ok, nb.value, dx1, dx2, bst, yraw, stats


def test_dgrad_epilogue_sums():
    """da_conv3d_k3_dgrad_bst: dx1 / dx2 against the float64 data gradient, and the partials against float64 sum dz, sum dz (y - mean) formed from the device's
    own dx1.  Single input C1 = 8, 12, 16, 32 (the two-N-tile form only this test reaches) and the 32 + 16 concat form."""
    def body(case):
        inp = bc.build_sums(case)
        ok, nb, dx1, dx2, bst, yraw, stats = _dgrad_bst(inp)
        tiles = bc.ntiles(*inp['dims'])
        assert ok and 0 < nb <= min(512, tiles) and (nb == tiles or nb % 8 == 0), (case, ok, nb, tiles)
        _, dx64 = bc.ref_sums(inp, torch.float64)
        dx = torch.cat((dx1, dx2), -1) if dx2 is not None else dx1
        bc.close('sums', 'dx', dx.permute(0, 4, 1, 2, 3), dx64, bc.TOL['sums']['dx'])
        dz, dzy, u1, u2 = _bst_terms(dx1, yraw, stats, inp['slope'])
        got = bst[:nb].sum(0)
        _sum_close('dgrad sum dz', got[0], dz, u1)
        _sum_close('dgrad sum dz (y - mean)', got[1], dzy, u2)
    with _mode('fp32_split'):
        bc.run_cases(bc.SUMS, body, pinned=bc.SUMS_PINNED)


def test_dgrad_epilogue_declines():
    """DA_ERR_UNSUPPORTED with *bst_n == 0: C1 = 4, C1 = 20, C1 = 16 with C2 = 16, matrix mode 'fp32', bst_cap = 511 (ops then runs da_conv3d_k3_dgrad and the
    stand-alone sums, which family 2 follows)."""
    base = dict(ch=(16, 0), cout=16, lcout=16, slope=0.01, sd=77, n=1, d=5, h=9, w=17)
    with _mode('fp32_split'):
        for c1 in (4, 20, (16, 16)):
            ok, nb = _dgrad_bst(bc.build_sums(dict(base, c1=c1)))[:2]
            assert not ok and nb == 0, c1
        ok, nb = _dgrad_bst(bc.build_sums(dict(base, c1=16)), bst_cap=511)[:2]
        assert not ok and nb == 0
        ok, nb = _dgrad_bst(bc.build_sums(dict(base, c1=16)))[:2]
        assert ok and nb > 0
    with _mode('fp32'):
        ok, nb = _dgrad_bst(bc.build_sums(dict(base, c1=16)))[:2]
        assert not ok and nb == 0


@pytest.mark.parametrize('C', [16, 32])
@pytest.mark.parametrize('N,dims', [(1, (3, 5, 7)), (2, (4, 8, 8)), (1, (7, 9, 11))])
def test_head_dice_epilogue_sums(C, N, dims):
    """da_head_dice_bwd_bst (Cin = 16; V = 105, 256, 693: below, equal to and no multiple of the 256-voxel chunk): dx, dW, db against da_head_dice_bwd at
    the tolerance of test_fused_head_softmax_dice_vs_torch_cpu, the partials against float64 sums formed from the device's own dx."""
    from deepatlas_amd import _native as nat, ops
    call, ptr = nat.call, nat.ptr
    Cin, V, slope = 16, dims[0] * dims[1] * dims[2], 0.01
    sd = 500 + C + V
    a = bc.nrm((N,) + dims + (Cin,), sd, 2.0).to(dev())
    stats = torch.stack([bc.nrm((Cin,), sd + 1, 0.1), torch.ones(Cin), 1.0 + 0.3 * bc.nrm((Cin,), sd + 2), bc.nrm((Cin,), sd + 3, 0.2)]).to(dev())
    w_io, b = bc.nrm((Cin, C), sd + 4, 0.5).to(dev()), bc.nrm((C,), sd + 5, 0.2).to(dev())
    lab = torch.randint(0, C, (N, V), generator=torch.Generator().manual_seed(sd)).to(dev())
    loss, coef, gl = torch.empty(1, device=dev()), torch.empty((2, N, C), device=dev()), torch.ones(1, device=dev())
    wp, wn = nat.workspace.get(nat.lib().da_head_dice_ws_bytes(N, V, Cin, C), dev())
    st = nat.stream()
    call('da_head_dice_fwd', ptr(a), ptr(stats[2]), ptr(stats[3]), slope, ptr(w_io), ptr(b), ptr(lab), 8, N, V, Cin, C, ops._WEIGHT_TYPES['Uniform'], 0, 1e-6,
         ptr(loss), ptr(coef), wp, wn, st)
    out = []
    for fused in (False, True):
        dx, dw, db = torch.empty_like(a), torch.empty_like(w_io), torch.empty_like(b)
        if fused:
            bst = torch.full((1024, 2, Cin), float('nan'), dtype=torch.float64, device=dev())
            nb = ctypes.c_int(0)
            call('da_head_dice_bwd_bst', ptr(a), ptr(stats[2]), ptr(stats[3]), slope, ptr(stats[0]), ptr(w_io), ptr(b), ptr(lab), 8, ptr(coef), ptr(gl), ptr(dx), ptr(dw), ptr(db),
                 N, V, Cin, C, ptr(bst), 1024, ctypes.byref(nb), wp, wn, st)
        else:
            call('da_head_dice_bwd', ptr(a), ptr(stats[2]), ptr(stats[3]), slope, ptr(w_io), ptr(b), ptr(lab), 8, ptr(coef), ptr(gl), ptr(dx), ptr(dw), ptr(db),
                 N, V, Cin, C, wp, wn, st)
        torch.cuda.synchronize()
        out.append((dx, dw, db))
    assert nb.value == N * ((V + 255) // 256)
    for got, ref in zip(out[1], out[0]):
        bc.close('sums', 'head', got, ref, bc.TOL['sums']['head'])
    dz, dzy, u1, u2 = _bst_terms(out[1][0], a, stats, slope)
    got = bst[:nb.value].sum(0)
    _sum_close('head sum dz', got[0], dz, u1)
    _sum_close('head sum dz (x - mean)', got[1], dzy, u2)
    bc.write_report()


@pytest.mark.parametrize('nparts', [1, 8, 512])
def test_statistics_from_partials(nparts):
    """da_bn_train_stats_from_partials against F.batch_norm in float64: mean, rstd, scale, shift and the running statistics."""
    from deepatlas_amd import _native as nat
    M, C, sd = 1531, 12, 600 + nparts
    y = (bc.nrm((M, C), sd, 1.5) + bc.nrm((C,), sd + 1)).double()
    gamma, beta, rm, rv = 1.0 + 0.3 * bc.nrm((C,), sd + 2), bc.nrm((C,), sd + 3, 0.2), bc.nrm((C,), sd + 4, 0.1), bc.nrm((C,), sd + 5).abs() * 0.5 + 0.5
    partials = torch.stack([torch.stack((c.sum(0), (c * c).sum(0))) for c in torch.tensor_split(y, nparts)]).to(dev())
    stats = torch.empty((4, C), device=dev())
    rmd, rvd = rm.to(dev()), rv.to(dev())
    g, b = gamma.to(dev()), beta.to(dev())
    nat.call('da_bn_train_stats_from_partials', nat.ptr(partials), nparts, M, C, nat.ptr(g), nat.ptr(b), bc.EPS, bc.MOMENTUM, nat.ptr(rmd), nat.ptr(rvd),
             nat.ptr(stats[0]), nat.ptr(stats[1]), nat.ptr(stats[2]), nat.ptr(stats[3]), nat.stream())
    torch.cuda.synchronize()
    rm64, rv64 = rm.double(), rv.double()
    z = F.batch_norm(y, rm64, rv64, gamma.double(), beta.double(), True, bc.MOMENTUM, bc.EPS)
    mean, rstd = y.mean(0), 1.0 / torch.sqrt(y.var(0, unbiased=False) + bc.EPS)
    scale = gamma.double() * rstd
    for got, ref in zip(stats.cpu(), (mean, rstd, scale, beta.double() - mean * scale)):
        bc.close('sums', 'stats', got, ref, bc.TOL['sums']['stats'])
    bc.close('sums', 'stats', y.float().to(dev()) * stats[2] + stats[3], z, bc.TOL['sums']['stats'])
    bc.close('sums', 'run', rmd, rm64, bc.TOL['sums']['run'])
    bc.close('sums', 'run', rvd, rv64, bc.TOL['sums']['run'])
    bc.write_report()
