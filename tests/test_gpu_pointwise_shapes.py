"""Randomised float64 parity for the up-sampler and 1x1 conv kernels (deconv.hip, pointwise_mfma.hip): the 2x2x2 stride-2 transposed convolution, the 1x1x1
head, their BatchNorm-statistics epilogue and input prologue, the fused up-sampler backward da_deconv_k2s2_bn_bwd and the bf16 twins.

Reference: plain torch in float64 on the widened fp32 inputs (F.conv_transpose3d(stride=2), F.conv3d, F.batch_norm with momentum 0.1 and eps 1e-5, the
activation), gradients by autograd with a drawn output gradient, running statistics compared after the call.  The device side goes through the public
surfaces (ops.Conv1x1Fn with and without a LazyAct prologue, ops.DeconvK2S2Fn, ops.DeconvBNActFn, modules.SegBlock as the consumer that hands sums over); the
raw C ABI only where a return code, the epilogue sums, the workspace size or a bf16 twin is itself under test.  Cases, builders, references, the two launcher
decisions (restated) and the tolerances live in tests/pointwise_cases.py; every family runs `pointwise_cases.run_cases`.  tests/test_pointwise_reference.py
runs the same examples on the CPU: fp32 oracle within a quarter of each tolerance, guard band under its cap, every pinned size on its branch.

Launcher branch <- value
  family 1 `conv1x1` (ops.Conv1x1Fn: y, dx, dW, db)
      pw_mfma_kernel<KC, NT, false>, its swapped GATHER pair, pw_wgrad_slice ntaps = 1  <- all 16 (Cin / 16, Cout / 16) in {1, 2, 3, 4}^2
      host-tiled 64-wide slices <- (80, 144), (128, 32); three K slices <- (192, 16); 48-channel slices <- (48, 96), (96, 48), (112, 64)
      conv1x1_kernel<8> <- (6, 5), (16, 3); <32> <- (16, 40); ragged last group of <32>, scalar stores <- (16, 42); data gradient on <32> <- (40, 5);
      direct weight gradient at O = 4000 <- (40, 100); two 64-row runs per block <- (6, 5) at M = 65601; DA_ERR_UNSUPPORTED <- (50, 100)
      rows (lane, 64-row wave tile, 256-row workgroup edges; a wave with no valid row, a workgroup with one) <- M = 1, 15, 17, 63, 65, 255, 256, 257 on (16, 16), (32, 64)
      weight-gradient walk at (16, 16), voxels per wave by pointwise_cases.wg_vox_per_wave: 4 <- M = 4096, 4097, 8203, 8193, 16384; 8 <- 16385 (three waves start
      past M), 16411 (ragged last wave); 12 (the loop's second trip, fetch(vb + 8) delivers) <- 32769, and 32771 behind a prologue
      prologue (Conv1x1Fn(..., pro)): slope 0 / 0.01, one negative scale channel, sliced K (Cin = 128), 48-channel slices; non-matrix shapes decline both
      prologue entries and ops._apply_pro runs (asserted with _native.CallProfiler)
  family 2 `deconv` (ops.DeconvK2S2Fn): the 16 tile pairs (taps per block 8, 4, 2 of the weight gradient); wide (128, 128), (256, 80), (48, 192); direct (6, 5),
      (16, 5) scalar stores, (5, 16); shapes 1 x 1 x 1, W = 3, W = 1, 2 x 3 x 5 x 7, 256 voxels, 1 x 1 x 257 on (16, 16), (32, 32)
      weight-gradient walk with the (cw, chh, crest) carry: 8 voxels per wave <- (16, 16) at 11 x 37 x 41, 75 x 73 x 3, 261 x 63 x 1 and (64, 64) (512 blocks) at
      19 x 19 x 23; 12 <- (16, 16) at 2 x 19 x 29 x 31 (N wrap)
  family 3 `upblock` (ops.DeconvBNActFn): train / eval, slope 0 / 0.01, lazy_out on / off, a negative-gamma channel, ops.FUSE_DECONV_BN_BWD on / off
      deconv_bn_bwd_kernel <- (32, 32): 5, 31, 32, 33, 512 coarse voxels; 16384 (512 chunks, one per workgroup); 16695 (workgroups 0 ... 9 walk two); 36378 (two or three)
      three-call backward on the matrix path <- (16, 16), (64, 32), (48, 16); direct kernels, *stats_nparts == 0, da_bn_train_stats runs <- (6, 5)
      hand-over of the BatchNorm-backward sums <- up-block (32, 32) lazy + 16-channel skip -> modules.SegBlock(48 -> 16), ops.FUSE_BN_BWD_STATS on / off
  family 4 `bf16` (C ABI): every _bf16 entry of deconv.hip at tile counts 1 ... 4 on each side (pair loads for even counts, single loads for 3), and the host-tiled
      (48, 96), (112, 64): fp32-output entries natively, bf16-output entries declined beyond one 64-channel K slice and run through ops.call_act's conversion

What the issue's size table says and the launcher does not: wg_blocks rounds the voxels per wave up to a multiple of 4 AFTER dividing M by 4 x blocks, so a second
K-step needs M > 16 x blocks (16384 at 1024 blocks, 8192 for a 64 x 64 up-sampler slice), not M > 4 x blocks.  The sizes the issue names (4097, 8203, 8193; 4551,
4161, 4221, 8990, 2185 coarse voxels) are kept and run, but all take one K-step; the sizes above are the smallest that reach the branches.

Worst case over all examples on an MI355X (distance from float64: tensors max(rel-l2, max-abs / max|ref|); 'db, train': max |db| / sum |dz_ref|; sums: largest
per-channel error / sum |term|), the fp32 CPU oracle's worst case on the same examples, the ceiling (pointwise_cases.CEIL) and what is asserted.
  family / quantity          device worst   fp32 oracle worst   ceiling   asserted
  conv1x1  y                    5.8e-7         4.6e-7            1e-4      3.7e-6
  conv1x1  dx                   5.2e-7         4.1e-7            1e-4      3.3e-6
  conv1x1  dW                   3.2e-7         5.9e-7            1e-4      4.7e-6
  conv1x1  db                   3.1e-7         4.6e-7            1e-4      3.7e-6
  deconv   y                    5.5e-7         7.3e-7            1e-4      5.9e-6
  deconv   dx                   1.2e-6         8.9e-7            1e-4      7.2e-6
  deconv   dW                   1.3e-7         3.8e-6            1e-4      1e-4    (8 x oracle = 3.0e-5, less than 10 x below the ceiling: stays)
  deconv   db                   1.6e-7         1.1e-5            1e-4      1e-4    (8 x oracle = 8.9e-5: stays)
  upblock  output               1.1e-6         6.1e-7            2e-5      2e-5    (stays)
  upblock  running stats        1.9e-7         1.5e-7            1e-5      1e-5    (1.2e-6: stays)
  upblock  dx, d_skip           8.1e-7         7.9e-7            2e-4      6.3e-6
  upblock  dW                   3.4e-7         3.3e-6            1e-4      1e-4    (stays)
  upblock  db, eval             4.2e-7         1.8e-6            1e-4      1e-4    (1.5e-5: stays)
  upblock  db, train            2.4e-8         8.0e-8            1e-5      6.5e-7
  upblock  d_gamma              9.3e-7         2.9e-6            2e-4      2e-4    (2.3e-5: stays)
  upblock  d_beta               8.3e-7         2.6e-6            2e-4      2e-4    (2.1e-5: stays)
  upblock  sum y / sum y^2      1.5e-7 / 3.0e-7   1.6e-7         1e-6      1e-6    (against the float64 reference's sums; stays)
  bf16     1x1 logits, dW, db   4.0e-7, 1.6e-7, 9.7e-8   3.8e-7, 6.5e-7, 1.9e-7   1e-4   3.7e-6, 4.7e-6, 3.7e-6  (conv1x1's: the entries' own fp32 family)
  bf16     up-sampler dW, db    6.1e-8, 4.6e-8           2.3e-6, 7.6e-7           1e-4   1e-4, 1e-4              (deconv's)
  bf16     sum y / sum y^2      8.2e-8 / 1.9e-7   -              1e-6      1e-6
  bf16     y, dx, act (stored bf16)   0.994, 0.994, 0.994 of 2^-8 |ref| + tol max|ref| (tol: 3.3e-6 ... 7.2e-6, the family's for the quantity): the bound is met
           with nothing to spare, as round-to-nearest must
Asserted = max(4 x device worst, 8 x fp32 oracle worst) rounded up to two digits wherever that is more than 10 x below the ceiling, else the ceiling.  Device: the
largest of the fused, three-call and no-hand-over runs (they differ by < 1.2 x).  Device against oracle: the kernels use exact fp32 matrix instructions and sit within
1.3 x of the fp32 oracle in every quantity but the up-block's output (1.8 x; its BatchNorm statistics come from double partial sums of fp32 values, the oracle's from
torch's own reduction -- both are a few roundings of z) -- and they are CLOSER to float64 than the oracle in every weight and bias gradient, up to 70 x (double partial
reductions against torch-CPU's fp32 sums).  No finding in the arithmetic.  Guard band: at most 33 elements of a tensor per example (a 524 336-element tensor; cap 0.1 % and 64).
The three chunk-walk shapes hold 4.2 - 9.3 M elements per tensor, where inputs centred on the kink would enter the band 300 - 700 times: their beta is centred at 3
(pointwise_cases.LARGE_BETA0), which leaves 11 entries at most.
Time on one MI355X: this file 9.0 s of pytest time (test_gpu_block_shapes.py: 12 s), the slowest test 1.9 s.  The whole GPU suite:
262 s of pytest time with this file (877 passed), 249 s for the parent commit's suite on the parent commit's library (861 passed).

Finding (fixed here): da_conv1x1_wgrad returned 0 with part of dW unwritten for every matrix-shaped layer whose 64-wide slicing leaves a 48-channel slice and whose
Cin x Cout exceeds 4096: (48, 96) and (96, 48) had outputs 4096 ... 4607 of 4608 unwritten, (112, 64) outputs 4096 ... 7167 of 7168 (distance 0.83 - 0.98 from float64; y, dx,
db right).  pw_wgrad_slice had no ntaps = 1 instantiation with a tile count of 3, so the matrix path declined and the direct kernel, which owns 16 x 256 outputs, ran.
The instantiations exist now and the direct fall-back declines above 4096 outputs.
Two more, found by the shapes added in review and fixed here.  (1) The host-tiled weight gradient put its placement scratch behind the partials of a 64 x 64 slice, but a
narrower slice has a higher block cap and can need more: (112, 64) at 19 x 19 x 23 = 8303 coarse voxels runs its 48 x 64 slice on 519 blocks (51 MB of partials) where the
64 x 64 figure is 260 blocks (34 MB), the scratch overlapped the partials and dW was 0.78 from float64; it now lies behind the largest slice's partials.  (2) A bf16-output
entry whose reduction spans more than one 64-channel slice accumulated the slices through the bf16 output, rounding once per slice: da_conv1x1_dgrad_bf16 at (48, 96) was
80 x its per-element bound.  Those entries now decline (forward Cin > 64, data gradients Cout > 64) and ops.call_act converts around the fp32 entry; the bound holds.

Mutants (one change each, built outside the tree, loaded through DA_LIB; every address stays inside its tensor), the tests that caught them and the distance:
  (a) weight-gradient fetch without `++chh`         test_deconv_random_shapes dW 1.03; test_upblock_chunk_walk[1x7x45x53], [2x9x43x47] dW 0.31, 0.42; test_bf16_twins dW 0.59
  (b) tapoff with j and k swapped                   test_deconv_random_shapes y 1.05 (41 pinned examples); test_upblock_*; test_upsampler_statistics_epilogue; test_bf16_twins
  (c) the loop's fetch(vb + 8) replaced by zeros    test_conv1x1_random_shapes dW 0.64 (M = 32769, 32771); test_deconv_random_shapes dW 0.58; chunk_walk[2x9x43x47] 0.59; test_bf16_twins 0.57
  (d) deconv_bn_bwd_kernel re-reads its first chunk test_upblock_chunk_walk[1x7x45x53], [2x9x43x47]: max |db| = 1.4e-3, 3.7e-3 of sum |dz| (tolerance 6.5e-7); 16384 voxels pass, as they must
  (e) statistics epilogue without a workgroup's last wave   test_upsampler_statistics_epilogue sum y 0.037 - 0.070 of sum |y| (257, 210, 256 voxels); test_upblock_*; test_bf16_twins sum y 0.038
None of the sizes the issue named for (a) and (c) catches them: they take one K-step (see above).
"""
import ctypes

import pytest
import torch

import pointwise_cases as pc
from test_gpu_block_shapes import _Profile, _activated, _block_results, _cpu, _mode, _no_stale_sums, _seg_block
from test_gpu_ops import cl, dev

pytestmark = pytest.mark.gpu


def _lazy_act(x, pro):
    from deepatlas_amd import ops
    with torch.no_grad():
        return _cpu(ops.materialize(ops.LazyAct(x.detach(), pro[0], pro[1], pro[2])))


def _records(prof, name):
    """integer arguments of every call of `name`"""
    return [k[1] for k, v in prof.prof.records.items() if k[0] == name for _ in v]


# ---- family 1 --------------------------------------------------------------------------------------------------------------------
C1_ENTRIES = ['da_conv1x1_fwd_pro', 'da_conv1x1_fwd', 'da_conv1x1_wgrad_pro', 'da_conv1x1_wgrad', 'da_conv1x1_dgrad', 'da_bn_act_fwd']


def _run_c1(inp):
    from deepatlas_amd import ops
    x = cl(inp['x']).requires_grad_(True)
    w, b = inp['w'].to(dev()).requires_grad_(True), inp['b'].to(dev()).requires_grad_(True)
    pro = (inp['scale'].to(dev()), inp['shift'].to(dev()), inp['pro']) if inp['pro'] is not None else None
    act = _lazy_act(x, pro) if pro is not None else None
    with _Profile(C1_ENTRIES) as prof:
        y = ops.Conv1x1Fn.apply(x, w, b, pro) if pro is not None else ops.Conv1x1Fn.apply(x, w, b)
        y.backward(cl(inp['gout']))
        torch.cuda.synchronize()
    return dict(y=_cpu(y), dx=_cpu(x.grad), dw=_cpu(w.grad), db=_cpu(b.grad), act=act), prof


def _wgrad_exact_workspace(inp, got, ref):
    """da_conv1x1_wgrad handed exactly da_conv1x1_wgrad_ws_bytes: rc 0, the right dW and db, and nothing written behind the workspace."""
    from deepatlas_amd import _native as nat
    cin, cout, M = inp['cin'], inp['cout'], pc.vox(inp['dims'])
    a = (got['act'] if got['act'] is not None else inp['x']).permute(0, 2, 3, 4, 1).contiguous().to(dev())
    dy = inp['gout'].permute(0, 2, 3, 4, 1).contiguous().to(dev())
    nbytes, guard = int(nat.lib().da_conv1x1_wgrad_ws_bytes(M, cin, cout)), 4096
    buf = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=dev())
    dw, db = torch.full((cin, cout), float('nan'), device=dev()), torch.full((cout,), float('nan'), device=dev())
    nat.call('da_conv1x1_wgrad', nat.ptr(a), nat.ptr(dy), nat.ptr(dw), nat.ptr(db), M, cin, cout, ctypes.c_void_p(buf.data_ptr()), ctypes.c_size_t(nbytes), nat.stream())
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == 0xA5).all()), 'written behind the workspace'
    pc.close('conv1x1', 'dw', dw.t().reshape(ref['dw'].shape), ref['dw'], pc.TOL['conv1x1']['dw'])
    pc.close('conv1x1', 'db', db, ref['db'], pc.TOL['conv1x1']['db'])


def test_conv1x1_random_shapes():
    """ops.Conv1x1Fn with and without a LazyAct prologue: y, dx, dW, db against float64; the route each example took; da_conv1x1_wgrad on an exact workspace."""
    def body(case):
        inp = pc.build_c1(case)
        got, prof = _run_c1(inp)
        ref = pc.ref_c1(inp, torch.float64, decided=got)
        pc.check_band(ref['band'])
        pc.compare_plain('conv1x1', got, ref, pc.TOL['conv1x1'])
        _wgrad_exact_workspace(inp, got, ref)
        n = {k: prof.count(k) for k in C1_ENTRIES}
        matrix = pc.pw_supported(inp['cin'], inp['cout'])
        assert n['da_conv1x1_dgrad'] == 1, (case, n)
        if inp['pro'] is None:
            assert (n['da_conv1x1_fwd'], n['da_conv1x1_wgrad'], n['da_conv1x1_fwd_pro'], n['da_conv1x1_wgrad_pro'], n['da_bn_act_fwd']) == (1, 1, 0, 0, 0), (case, n)
        elif matrix:       # both prologue entries take every matrix-path shape, the 48-channel slices included
            assert (n['da_conv1x1_fwd'], n['da_conv1x1_wgrad'], n['da_conv1x1_fwd_pro'], n['da_conv1x1_wgrad_pro'], n['da_bn_act_fwd']) == (0, 0, 1, 1, 0), (case, n)
        else:              # da_conv1x1_fwd_pro declines, ops._apply_pro materialises the activation once and the plain entries run on it
            assert (n['da_conv1x1_fwd'], n['da_conv1x1_wgrad'], n['da_conv1x1_fwd_pro'], n['da_conv1x1_wgrad_pro'], n['da_bn_act_fwd']) == (1, 1, 1, 0, 1), (case, n)
    pc.run_cases(pc.C1, body, pinned=pc.C1_PINNED)


def test_conv1x1_declines():
    """Return codes through the C ABI: (50, 100), O = 5000 and not matrix-shaped, is DA_ERR_UNSUPPORTED for the weight gradient; the prologue entries decline every
    non-matrix shape; (40, 100), O = 4000, is accepted."""
    from deepatlas_amd import _native as nat
    M = 130
    for cin, cout, ok in ((50, 100, False), (40, 100, True)):
        a, dy = pc.nrm((M, cin), 1).to(dev()), pc.nrm((M, cout), 2).to(dev())
        dw, db = torch.empty((cin, cout), device=dev()), torch.empty((cout,), device=dev())
        wp, wn = nat.workspace.get(nat.lib().da_conv1x1_wgrad_ws_bytes(M, cin, cout), dev())
        assert nat.call_supported('da_conv1x1_wgrad', nat.ptr(a), nat.ptr(dy), nat.ptr(dw), nat.ptr(db), M, cin, cout, wp, wn, nat.stream()) == ok
        if ok:
            pc.close('conv1x1', 'dw', dw, a.double().t() @ dy.double(), pc.TOL['conv1x1']['dw'])
    for cin, cout in ((6, 5), (50, 100), (16, 3), (40, 16)):
        a, dy, w = pc.nrm((M, cin), 1).to(dev()), pc.nrm((M, cout), 2).to(dev()), pc.nrm((cin, cout), 3).to(dev())
        s, t = torch.ones(cin, device=dev()), torch.zeros(cin, device=dev())
        y, dw = torch.empty((M, cout), device=dev()), torch.empty((cin, cout), device=dev())
        wp, wn = nat.workspace.get(max(nat.lib().da_conv1x1_wgrad_ws_bytes(M, cin, cout), nat.lib().da_pointwise_ws_bytes(1, cin, cout)), dev())
        assert not nat.call_supported('da_conv1x1_fwd_pro', nat.ptr(a), nat.ptr(s), nat.ptr(t), 0.01, nat.ptr(w), None, nat.ptr(y), M, cin, cout, wp, wn, nat.stream())
        assert not nat.call_supported('da_conv1x1_wgrad_pro', nat.ptr(a), nat.ptr(s), nat.ptr(t), 0.01, nat.ptr(dy), nat.ptr(dw), None, M, cin, cout, wp, wn, nat.stream())
    torch.cuda.synchronize()


# ---- family 2 --------------------------------------------------------------------------------------------------------------------
def test_deconv_random_shapes():
    """ops.DeconvK2S2Fn: y, dx, dW, db against float64."""
    from deepatlas_amd import ops

    def body(case):
        inp = pc.build_d2(case)
        x = cl(inp['x']).requires_grad_(True)
        w, b = inp['w'].to(dev()).requires_grad_(True), inp['b'].to(dev()).requires_grad_(True)
        y = ops.DeconvK2S2Fn.apply(x, w, b)
        y.backward(cl(inp['gout']))
        torch.cuda.synchronize()
        pc.compare_plain('deconv', dict(y=_cpu(y), dx=_cpu(x.grad), dw=_cpu(w.grad), db=_cpu(b.grad)), pc.ref_d2(inp, torch.float64), pc.TOL['deconv'])
    pc.run_cases(pc.D2, body, pinned=pc.D2_PINNED)


# ---- family 3 --------------------------------------------------------------------------------------------------------------------
UP_ENTRIES = ['da_deconv_k2s2_fwd_bnstats', 'da_deconv_k2s2_fwd', 'da_bn_train_stats', 'da_bn_train_stats_from_partials', 'da_deconv_k2s2_bn_bwd', 'da_deconv_k2s2_dgrad',
              'da_deconv_k2s2_wgrad', 'da_bn_act_bwd_dbias', 'da_bn_act_bwd_dbias_pre', 'da_conv3d_k3_dgrad_bst']


def _run_up(inp):
    from deepatlas_amd import ops
    p = inp['p']
    x = cl(inp['x']).requires_grad_(True)
    w, b, gamma, beta = (p[k].to(dev()).requires_grad_(True) for k in ('w', 'b', 'gamma', 'beta'))
    rm, rv = p['rm'].to(dev()), p['rv'].to(dev())
    blk = _seg_block(inp['p2'], inp['slope2'], inp['train']) if inp['chain'] else None
    skip = cl(inp['skip']).requires_grad_(True) if inp['chain'] else None
    args = (x, w, b, gamma, beta, rm, rv, inp['train'], pc.MOMENTUM, pc.EPS, inp['slope'])
    with _Profile(UP_ENTRIES) as prof:
        lz = None
        if inp['lazy']:
            yraw, scale, shift = ops.DeconvBNActFn.apply(*(args + (True,)))
            lz = ops.LazyAct(yraw, scale, shift, inp['slope'])
            out = blk(lz, skip) if blk is not None else yraw
        else:
            out = ops.DeconvBNActFn.apply(*args)
        out.backward(cl(inp['gout']))
        torch.cuda.synchronize()
    _no_stale_sums()
    act0 = _activated(lz) if lz is not None else _cpu(out)
    res = dict(out=_cpu(out) if (blk is not None or lz is None) else act0, act0=act0, dx=_cpu(x.grad), dw0=_cpu(w.grad), db0=_cpu(b.grad), dgamma0=_cpu(gamma.grad),
               dbeta0=_cpu(beta.grad), rm0=_cpu(rm), rv0=_cpu(rv))
    if blk is not None:
        res.update(act1=_cpu(out), dskip=_cpu(skip.grad))
        _block_results(blk, 1, res)
    return res, prof


def _upblock_body(case):
    """One example in every switch setting, each against float64: ops.FUSE_DECONV_BN_BWD on / off; with the consumer also ops.FUSE_BN_BWD_STATS on / off."""
    from deepatlas_amd import ops
    inp = pc.build_up(case)
    cin, cout = inp['cin'], inp['cout']
    ref = None
    for bst, fuse in (((True, True), (False, True), (True, False)) if inp['chain'] else ((True, True), (True, False))):
        ops.FUSE_BN_BWD_STATS, ops.FUSE_DECONV_BN_BWD = bst, fuse
        got, prof = _run_up(inp)
        if ref is None or not all(torch.equal(got[k], ref_from[k]) for k in got if k.startswith('act')):
            ref, ref_from = pc.ref_up(inp, torch.float64, decided=got), got
            pc.check_band(ref['band'])
        pc.compare('upblock' + ('' if fuse else ' three-call') + ('' if bst else ' no hand-over'), got, ref, pc.TOL['upblock'])
        n = {k: prof.count(k) for k in UP_ENTRIES}
        matrix = pc.pw_supported(cin, cout)
        if inp['train']:
            # the epilogue delivers the statistics on the matrix path (one partial per 256 coarse voxels); elsewhere *stats_nparts == 0 and da_bn_train_stats runs
            assert n['da_deconv_k2s2_fwd_bnstats'] == 1 and n['da_deconv_k2s2_fwd'] == 0, (case, n)
            assert n['da_bn_train_stats'] == (0 if matrix else 1) and n['da_bn_train_stats_from_partials'] == (1 if matrix else 0) + int(inp['chain']), (case, n)
        else:
            assert n['da_deconv_k2s2_fwd_bnstats'] == 0 and n['da_deconv_k2s2_fwd'] == 1 and n['da_bn_train_stats'] == 0, (case, n)
        fused = fuse and inp['train'] and (cin, cout) == (32, 32)
        assert n['da_deconv_k2s2_bn_bwd'] == int(fused) and n['da_deconv_k2s2_dgrad'] == n['da_deconv_k2s2_wgrad'] == 1 - int(fused), (case, n)
        if inp['chain']:
            handed = bst and inp['train']
            assert (n['da_conv3d_k3_dgrad_bst'] > 0) == bst, (case, n)
            if fused:
                assert (_records(prof, 'da_deconv_k2s2_bn_bwd')[0][-1] > 0) == handed, (case, _records(prof, 'da_deconv_k2s2_bn_bwd'))
            else:
                assert n['da_bn_act_bwd_dbias_pre'] == int(handed), (case, n)


def _with_switches(fn):
    from deepatlas_amd import ops
    prev = ops.FUSE_BN_BWD_STATS, ops.FUSE_DECONV_BN_BWD
    try:
        with _mode('fp32_split'):      # (the shipped mode: the consumer's data gradient hands its sums over there only)
            fn()
    finally:
        ops.FUSE_BN_BWD_STATS, ops.FUSE_DECONV_BN_BWD = prev


UP_LARGE = [c for c in pc.UP_PINNED if pc.vox(c['dims']) > 10000]


def test_upblock_random_shapes():
    """ops.DeconvBNActFn: output, running statistics, dx, dW, d_gamma, d_beta, db (train mode: zero in exact arithmetic, asserted as block_cases' db_zero) against
    float64, fused and three-call backward, and the hand-over of the BatchNorm-backward sums from a modules.SegBlock consumer."""
    _with_switches(lambda: pc.run_cases(pc.UP, _upblock_body, pinned=[c for c in pc.UP_PINNED if c not in UP_LARGE]))


@pytest.mark.parametrize('case', UP_LARGE, ids=lambda c: 'x'.join(map(str, c['dims'])))
def test_upblock_chunk_walk(case):
    """deconv_bn_bwd_kernel at 512 chunks (one per workgroup), 522 (workgroups 0 ... 9 walk two) and 1137 (two or three, ragged last chunk); one float64
    reference per shape, shared by the fused and the three-call run."""
    assert pc.db_chunks_per_block(pc.vox(case['dims'])) == pc.UP_CHUNKS[pc.UP_SHAPES.index(case['dims'])]
    pc.lc._state['case'] = case
    _with_switches(lambda: _upblock_body(case))
    pc.write_report()


def _tio(w):
    """[Cin][Cout][2,2,2] -> the kernels' [8][Cin][Cout]"""
    return w.permute(2, 3, 4, 0, 1).reshape(8, w.shape[0], w.shape[1]).contiguous().to(dev())


def _ndhwc(t, dtype=torch.float32):
    return t.permute(0, 2, 3, 4, 1).contiguous().to(dev()).to(dtype)


def _sum_err(got, terms):
    return pc.bc.col_err(got, terms)


@pytest.mark.parametrize('cin,cout,dims', [(32, 32, (1, 1, 1, 257)), (16, 48, (1, 2, 3, 5)), (128, 80, (2, 3, 5, 7)), (64, 64, (1, 4, 8, 8)), (48, 16, (1, 1, 1, 1)), (6, 5, (1, 3, 5, 7))],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_upsampler_statistics_epilogue(cin, cout, dims):
    """da_deconv_k2s2_fwd_bnstats: partials[:n].sum(0) against the float64 reference's sum y and sum y^2 (1e-6 of sum |term|, as
    test_deconv_fused_batchnorm_statistics), the output against float64; with stats_capacity = nblk - 1 it reports 0 parts and writes the same output; (6, 5): 0 parts."""
    from deepatlas_amd import _native as nat
    pc.lc._state['case'] = (cin, cout, dims)
    inp = pc.build_d2(dict(cin=cin, cout=cout, dims=dims, sd=500 + cin))
    N, D, H, W = dims
    a, w, b = _ndhwc(inp['x']), _tio(inp['w']), inp['b'].to(dev())
    nblk = (pc.vox(dims) + 255) // 256
    wp, wn = nat.workspace.get(nat.lib().da_pointwise_ws_bytes(8, cin, cout), dev())
    ref_y = pc.ref_d2(inp, torch.float64)['y']
    outs = []
    for cap in (nblk, nblk - 1):
        y = torch.full((N, 2 * D, 2 * H, 2 * W, cout), float('nan'), device=dev())
        pbuf = torch.full((nblk + 1, 2, cout), float('nan'), dtype=torch.float64, device=dev())
        n = ctypes.c_int(-1)
        nat.call('da_deconv_k2s2_fwd_bnstats', nat.ptr(a), nat.ptr(w), nat.ptr(b), nat.ptr(y), N, D, H, W, cin, cout, nat.ptr(pbuf), cap, ctypes.byref(n), wp, wn, nat.stream())
        torch.cuda.synchronize()
        outs.append(y)
        if cap == nblk and pc.pw_supported(cin, cout):
            assert n.value == nblk and bool(torch.isnan(pbuf[nblk]).all())
            got, yd = pbuf[:nblk].sum(0), ref_y.movedim(1, -1)
            for what, g, terms in (('fwd sum y', got[0], yd), ('fwd sum y^2', got[1], yd * yd)):
                e = _sum_err(g, terms)
                pc.note('upblock', what, e)
                assert e < pc.TOL['upblock']['sum'], (what, e)
        else:
            assert n.value == 0 and bool(torch.isnan(pbuf).all())
    assert torch.equal(outs[0], outs[1])
    pc.close('deconv', 'y', outs[0].permute(0, 4, 1, 2, 3), ref_y, pc.TOL['deconv']['y'])
    pc.write_report()


# ---- family 4: the bf16 twins --------------------------------------------------------------------------------------------------------
BF = torch.bfloat16


def _bf_out(name, k, *args):
    """An entry whose OUTPUT is bf16, through ops.call_act (arguments wrapped in ops.A / ops.O): the twin itself while its reduction fits one 64-channel slice;
    beyond that the twin declines (the slices accumulate through the output tensor, which would round a bf16 output once per slice) and call_act converts
    around the fp32 entry.  Either way the stored result is held to the one-rounding bound by the caller."""
    from deepatlas_amd import ops
    before = ops.bridged_calls.get(name, 0)
    ops.call_act(name, *args)
    assert ops.bridged_calls.get(name, 0) - before == int(k > 64), (name, k, dict(ops.bridged_calls))


def _bf_conv1x1(c, i1):
    from deepatlas_amd.ops import A, O
    from deepatlas_amd import _native as nat
    call, ptr, st = nat.call, nat.ptr, nat.stream()
    cin, cout, M = c['cin'], c['cout'], c['m']
    tol = pc.TOL['conv1x1']      # the fp32 family of these entries
    x32 = i1['x'].permute(0, 2, 3, 4, 1).reshape(M, cin).contiguous()
    x, dy = x32.to(dev()).to(BF), i1['gout'].permute(0, 2, 3, 4, 1).reshape(M, cout).contiguous().to(dev())
    w, b = i1['w'].reshape(cout, cin).t().contiguous().to(dev()), i1['b'].to(dev())
    assert torch.equal(x.float().cpu(), x32)                                                # (the inputs are exactly representable)
    ref = pc.ref_c1(i1, torch.float64)
    wp, wn = nat.workspace.get(max(nat.lib().da_conv1x1_wgrad_ws_bytes(M, cin, cout), nat.lib().da_pointwise_ws_bytes(1, cin, cout)), dev())
    y, dx = torch.full((M, cout), float('nan'), device=dev()), torch.full((M, cin), float('nan'), device=dev()).to(BF)
    dw, db = torch.full((cin, cout), float('nan'), device=dev()), torch.full((cout,), float('nan'), device=dev())
    call('da_conv1x1_fwd_bf16', ptr(x), ptr(w), ptr(b), ptr(y), M, cin, cout, wp, wn, st)
    _bf_out('da_conv1x1_dgrad', cout, A(dy), ptr(w), O(dx), M, cin, cout, wp, wn, st)
    call('da_conv1x1_wgrad_bf16', ptr(x), ptr(dy), ptr(dw), ptr(db), M, cin, cout, wp, wn, st)
    torch.cuda.synchronize()
    rows = lambda t: t.permute(0, 2, 3, 4, 1).reshape(M, -1)
    pc.close('bf16', 'conv1x1 y', y, rows(ref['y']), tol['y'])
    pc.bf16_close('conv1x1 dx', dx.float(), rows(ref['dx']), tol['dx'])
    pc.close('bf16', 'conv1x1 dw', dw, ref['dw'].reshape(cout, cin).t(), tol['dw'])
    pc.close('bf16', 'conv1x1 db', db, ref['db'], tol['db'])
    # the prologue twins: act(x scale + shift) rounded to bf16 is what the convolution consumes -- the tensor da_bn_act_fwd_bf16 stores, which is held to
    # float64 within one bf16 spacing and then taken as the float64 reference's input
    scale, shift = (t.to(dev()) for t in pc.pro_params(cin, 100 * c['sd']))
    slope = 0.01
    act = torch.empty_like(x)
    call('da_bn_act_fwd_bf16', ptr(x), ptr(scale), ptr(shift), slope, ptr(act), M, cin, st)
    z = x32.double() * scale.double().cpu() + shift.double().cpu()
    pc.bf16_close('conv1x1 act', act.float(), torch.maximum(z, z * slope), tol['y'])
    y2, dw2, db2 = torch.full_like(y, float('nan')), torch.full_like(dw, float('nan')), torch.full_like(db, float('nan'))
    call('da_conv1x1_fwd_pro_bf16', ptr(x), ptr(scale), ptr(shift), slope, ptr(w), ptr(b), ptr(y2), M, cin, cout, wp, wn, st)
    call('da_conv1x1_wgrad_pro_bf16', ptr(x), ptr(scale), ptr(shift), slope, ptr(dy), ptr(dw2), ptr(db2), M, cin, cout, wp, wn, st)
    torch.cuda.synchronize()
    a64 = act.double().cpu()
    pc.close('bf16', 'conv1x1 y', y2, a64 @ w.double().cpu() + b.double().cpu(), tol['y'])
    pc.close('bf16', 'conv1x1 dw', dw2, a64.t() @ dy.double().cpu(), tol['dw'])
    pc.close('bf16', 'conv1x1 db', db2, ref['db'], tol['db'])


def _bf_deconv(c, i2):
    from deepatlas_amd.ops import A, O
    from deepatlas_amd import _native as nat
    call, ptr, st = nat.call, nat.ptr, nat.stream()
    cin, cout, (N, D, H, W) = c['cin'], c['cout'], c['dims']
    tol = pc.TOL['deconv']       # the fp32 family of these entries
    x, g, w, b = _ndhwc(i2['x'], BF), _ndhwc(i2['gout'], BF), _tio(i2['w']), i2['b'].to(dev())
    ref = pc.ref_d2(i2, torch.float64)
    wp, wn = nat.workspace.get(max(nat.lib().da_deconv_k2s2_wgrad_ws_bytes(N, D, H, W, cin, cout), nat.lib().da_pointwise_ws_bytes(8, cin, cout)), dev())
    nblk = (pc.vox(c['dims']) + 255) // 256
    y, y2 = (torch.full((N, 2 * D, 2 * H, 2 * W, cout), float('nan'), device=dev()).to(BF) for _ in range(2))
    dx = torch.full((N, D, H, W, cin), float('nan'), device=dev()).to(BF)
    dw, db = torch.full((8, cin, cout), float('nan'), device=dev()), torch.full((cout,), float('nan'), device=dev())
    pbuf, n = torch.full((nblk, 2, cout), float('nan'), dtype=torch.float64, device=dev()), ctypes.c_int(-1)
    _bf_out('da_deconv_k2s2_fwd', cin, A(x), ptr(w), ptr(b), O(y), N, D, H, W, cin, cout, wp, wn, st)
    _bf_out('da_deconv_k2s2_fwd_bnstats', cin, A(x), ptr(w), ptr(b), O(y2), N, D, H, W, cin, cout, ptr(pbuf), nblk, ctypes.byref(n), wp, wn, st)
    _bf_out('da_deconv_k2s2_dgrad', cout, A(g), ptr(w), O(dx), N, D, H, W, cin, cout, wp, wn, st)
    call('da_deconv_k2s2_wgrad_bf16', ptr(x), ptr(g), ptr(dw), ptr(db), N, D, H, W, cin, cout, wp, wn, st)
    torch.cuda.synchronize()
    pc.bf16_close('deconv y', y.float().permute(0, 4, 1, 2, 3), ref['y'], tol['y'])
    pc.bf16_close('deconv dx', dx.float().permute(0, 4, 1, 2, 3), ref['dx'], tol['dx'])
    pc.close('bf16', 'deconv dw', dw.reshape(2, 2, 2, cin, cout).permute(3, 4, 0, 1, 2), ref['dw'], tol['dw'])
    pc.close('bf16', 'deconv db', db, ref['db'], tol['db'])
    # the statistics are taken from the fp32 accumulators, before the store rounds them: against the float64 reference's own sums
    assert n.value == nblk and torch.equal(y.view(torch.int16), y2.view(torch.int16))
    yr = ref['y'].movedim(1, -1)
    got = pbuf.sum(0)
    for what, gq, terms in (('bf16 sum y', got[0], yr), ('bf16 sum y^2', got[1], yr * yr)):
        e = _sum_err(gq, terms)
        pc.note('bf16', what, e)
        assert e < pc.TOL['upblock']['sum'], (what, e)


def test_bf16_twins():
    """Every _bf16 entry of deconv.hip at tile counts 1 ... 4 on each side.  Inputs are drawn in fp32, rounded to bf16 and handed over as bf16; the float64
    reference takes the widened values.  fp32 results (logits, dW, db) at the tolerance of the entry's own fp32 family (conv1x1 / deconv); bf16 results per element within
    2^-8 |ref| + tol max|ref| (pointwise_cases.bf16_close: derived, not measured)."""
    for c in pc.BF_PINNED:
        pc.lc._state['case'] = c
        i1, i2 = pc.build_bf(c)
        _bf_conv1x1(c, i1)
        _bf_deconv(c, i2)
    pc.write_report()


def test_bf16_twins_decline_a_sliced_reduction_into_a_bf16_output():
    """DA_ERR_UNSUPPORTED, with *stats_nparts == 0, from every bf16-output entry whose reduction spans more than one 64-channel slice: (112, 64) for the forward,
    (48, 96) for the data gradients.  The entries with fp32 outputs take the same shapes (test_bf16_twins)."""
    from deepatlas_amd import _native as nat
    ptr, st = nat.ptr, nat.stream()
    M, (N, D, H, W) = 70, (1, 2, 3, 5)
    z = lambda *shape: torch.zeros(shape, device=dev())
    wp, wn = nat.workspace.get(max(nat.lib().da_pointwise_ws_bytes(8, 112, 64), nat.lib().da_pointwise_ws_bytes(8, 48, 96)), dev())
    n = ctypes.c_int(-1)
    xs, ys, pbuf = z(N, D, H, W, 112).to(BF), z(N, 2 * D, 2 * H, 2 * W, 64).to(BF), torch.zeros((1, 2, 64), dtype=torch.float64, device=dev())
    assert not nat.call_supported('da_deconv_k2s2_fwd_bf16', ptr(xs), ptr(z(8, 112, 64)), None, ptr(ys), N, D, H, W, 112, 64, wp, wn, st)
    assert not nat.call_supported('da_deconv_k2s2_fwd_bnstats_bf16', ptr(xs), ptr(z(8, 112, 64)), None, ptr(ys), N, D, H, W, 112, 64, ptr(pbuf), 1, ctypes.byref(n), wp, wn, st)
    assert n.value == 0
    gs, dxs = z(N, 2 * D, 2 * H, 2 * W, 96).to(BF), z(N, D, H, W, 48).to(BF)
    assert not nat.call_supported('da_deconv_k2s2_dgrad_bf16', ptr(gs), ptr(z(8, 48, 96)), ptr(dxs), N, D, H, W, 48, 96, wp, wn, st)
    assert not nat.call_supported('da_conv1x1_dgrad_bf16', ptr(z(M, 96)), ptr(z(48, 96)), ptr(z(M, 48).to(BF)), M, 48, 96, wp, wn, st)
    # one slice: taken
    dy1, w1, dx1 = z(M, 64), z(48, 64), z(M, 48).to(BF)
    assert nat.call_supported('da_conv1x1_dgrad_bf16', ptr(dy1), ptr(w1), ptr(dx1), M, 48, 64, wp, wn, st)
    torch.cuda.synchronize()


def test_bf16_twins_decline_non_matrix_shapes():
    from deepatlas_amd import _native as nat
    ptr, st = nat.ptr, nat.stream()
    M, (N, D, H, W) = 70, (1, 2, 3, 5)
    for cin, cout in pc.BF_DECLINED:
        x, dy, w = torch.zeros((M, cin), device=dev()).to(BF), torch.zeros((M, cout), device=dev()), torch.zeros((cin, cout), device=dev())
        s, y, dw, db = torch.ones(cin, device=dev()), torch.zeros((M, cout), device=dev()), torch.zeros((cin, cout), device=dev()), torch.zeros(cout, device=dev())
        dxb = torch.zeros_like(x)
        wp, wn = nat.workspace.get(max(nat.lib().da_conv1x1_wgrad_ws_bytes(M, cin, cout), nat.lib().da_deconv_k2s2_wgrad_ws_bytes(N, D, H, W, cin, cout),
                                       nat.lib().da_pointwise_ws_bytes(8, cin, cout)), dev())
        xs, gs = torch.zeros((N, D, H, W, cin), device=dev()).to(BF), torch.zeros((N, 2 * D, 2 * H, 2 * W, cout), device=dev()).to(BF)
        w8, dw8, n = torch.zeros((8, cin, cout), device=dev()), torch.zeros((8, cin, cout), device=dev()), ctypes.c_int(-1)
        pbuf = torch.zeros((1, 2, cout), dtype=torch.float64, device=dev())
        calls = [('da_conv1x1_fwd_bf16', ptr(x), ptr(w), None, ptr(y), M, cin, cout, wp, wn, st),
                 ('da_conv1x1_fwd_pro_bf16', ptr(x), ptr(s), ptr(s), 0.01, ptr(w), None, ptr(y), M, cin, cout, wp, wn, st),
                 ('da_conv1x1_dgrad_bf16', ptr(dy), ptr(w), ptr(dxb), M, cin, cout, wp, wn, st),
                 ('da_conv1x1_wgrad_bf16', ptr(x), ptr(dy), ptr(dw), ptr(db), M, cin, cout, wp, wn, st),
                 ('da_conv1x1_wgrad_pro_bf16', ptr(x), ptr(s), ptr(s), 0.01, ptr(dy), ptr(dw), ptr(db), M, cin, cout, wp, wn, st),
                 ('da_deconv_k2s2_fwd_bf16', ptr(xs), ptr(w8), None, ptr(gs), N, D, H, W, cin, cout, wp, wn, st),
                 ('da_deconv_k2s2_fwd_bnstats_bf16', ptr(xs), ptr(w8), None, ptr(gs), N, D, H, W, cin, cout, ptr(pbuf), 1, ctypes.byref(n), wp, wn, st),
                 ('da_deconv_k2s2_dgrad_bf16', ptr(gs), ptr(w8), ptr(xs), N, D, H, W, cin, cout, wp, wn, st),
                 ('da_deconv_k2s2_wgrad_bf16', ptr(xs), ptr(gs), ptr(dw8), ptr(db), N, D, H, W, cin, cout, wp, wn, st)]
        for args in calls:
            assert not nat.call_supported(*args), (args[0], cin, cout)
        assert n.value == 0
    torch.cuda.synchronize()
