"""CPU companion of tests/test_gpu_pointwise_shapes.py (no GPU): on the SAME pinned and derandomised examples (tests/pointwise_cases.py run_cases), the
same operation evaluated in fp32 on torch-CPU must sit within a quarter of every tolerance of its float64 evaluation, and the guard-band caps must hold with
the fp32 oracle in the device's place.  That makes each tolerance of the device test a statement about the kernel.  The last test checks, by the two
launcher decisions restated in pointwise_cases.py, that every pinned size reaches the branch it is pinned for: arithmetic, not luck."""
import torch

import pointwise_cases as pc


def _quarter(family):
    return {k: v / 4 for k, v in pc.TOL[family].items()}


def test_conv1x1_inputs_are_well_conditioned():
    q = _quarter('conv1x1')

    def body(case):
        inp = pc.build_c1(case)
        r32 = pc.ref_c1(inp, torch.float32)
        r64 = pc.ref_c1(inp, torch.float64, decided=r32)
        pc.check_band(r64['band'])
        for k, n in r64['band']:
            pc.note('cpu conv1x1', 'band elements', k)
        pc.compare_plain('cpu conv1x1', r32, r64, q)
    pc.run_cases(pc.C1, body, pinned=pc.C1_PINNED)


def test_deconv_inputs_are_well_conditioned():
    q = _quarter('deconv')

    def body(case):
        inp = pc.build_d2(case)
        pc.compare_plain('cpu deconv', pc.ref_d2(inp, torch.float32), pc.ref_d2(inp, torch.float64), q)
    pc.run_cases(pc.D2, body, pinned=pc.D2_PINNED)


def test_upblock_inputs_are_well_conditioned():
    """Also the statistics epilogue's quantity: fp32 column sums of the fp32 output in units of sum |term|."""
    q = _quarter('upblock')

    def body(case):
        inp = pc.build_up(case)
        r32 = pc.ref_up(inp, torch.float32)
        r64 = pc.ref_up(inp, torch.float64, decided=r32)
        pc.check_band(r64['band'])
        for k, n in r64['band']:
            pc.note('cpu upblock', 'band elements', k)
        pc.compare('cpu upblock', r32, r64, q)
        if not inp['chain']:
            t = r32['act0'].float().movedim(1, -1)
            for got, terms in ((t.sum((0, 1, 2, 3)), t), ((t * t).sum((0, 1, 2, 3)), t * t)):
                e = pc.bc.col_err(got, terms)
                pc.note('cpu upblock', 'sum', e)
                assert e < q['sum'], e
    pc.run_cases(pc.UP, body, pinned=pc.UP_PINNED)


def test_bf16_inputs_are_well_conditioned():
    """The bf16 family's fp32 results (logits, dW, db) are asserted at the fp32 family's tolerance (conv1x1 for the 1x1 twins, deconv for the up-sampler's) on inputs rounded to bf16: the fp32 oracle on exactly those, per family."""
    for c in pc.BF_PINNED:
        pc.lc._state['case'] = c
        i1, i2 = pc.build_bf(c)
        pc.compare_plain('cpu bf16 conv1x1', pc.ref_c1(i1, torch.float32), pc.ref_c1(i1, torch.float64), _quarter('conv1x1'))
        pc.compare_plain('cpu bf16 deconv', pc.ref_d2(i2, torch.float32), pc.ref_d2(i2, torch.float64), _quarter('deconv'))
    pc.write_report()


def test_pinned_examples_reach_what_they_name():
    # family 1: every tile pair, wide, direct and row class has its example, and the builders leave pinned shapes alone
    chans = {(c['cin'], c['cout']) for c in pc.C1_PINNED}
    assert set(pc.TILE_PAIRS + pc.C1_WIDE + pc.C1_DIRECT) <= chans
    assert all(pc.pw_supported(*ch) for ch in pc.TILE_PAIRS + pc.C1_WIDE) and not any(pc.pw_supported(*ch) for ch in pc.C1_DIRECT)
    assert all(ci * co <= 4096 for ci, co in pc.C1_DIRECT) and 42 % 4 != 0
    for ch in ((16, 16), (32, 64)):
        assert {pc.vox(c['dims']) for c in pc.C1_PINNED if (c['cin'], c['cout']) == ch} >= set(pc.C1_ROWS)
    assert all(pc.build_c1(c)['dims'] == c['dims'] for c in pc.C1_PINNED) and all(pc.build_d2(c)['dims'] == c['dims'] for c in pc.D2_PINNED)
    assert all(pc.build_up(c)['dims'] == c['dims'] for c in pc.UP_PINNED)
    # the weight-gradient walk: voxels per wave by the launcher's own rule.  The four sizes named first all take one K-step; 8 and 12 start at 16385 and 32769.
    vpw = [pc.wg_vox_per_wave(m, 1, 16, 16) for m in pc.C1_WALK]
    assert vpw == [4, 4, 4, 4, 4, 8, 8, 12], vpw
    assert pc.wg_idle_waves(16385, 8) == 3 and pc.wg_idle_waves(16411, 8) == 0 and 16411 % 8 != 0 and pc.wg_vox_per_wave(32771, 1, 16, 16) == 12
    assert {pc.vox(c['dims']) for c in pc.C1_PINNED if (c['cin'], c['cout']) == (16, 16)} >= set(pc.C1_WALK)
    # direct weight gradient: 1026 tile runs of 64 rows over 1024 blocks = 2 per block
    assert pc._cdiv(pc._cdiv(65601, 64), 1024) == 2 and any(pc.vox(c['dims']) == 65601 and c['cin'] == 6 for c in pc.C1_PINNED)
    # family 2
    chans = {(c['cin'], c['cout']) for c in pc.D2_PINNED}
    assert set(pc.TILE_PAIRS + pc.D2_WIDE + pc.D2_DIRECT) <= chans
    # taps per block 8, 4, 2 of the ntaps = 8 weight gradient: tile products <= 4, <= 8, above
    assert {8 if a * b <= 4 else 4 if a * b <= 8 else 2 for a in (1, 2, 3, 4) for b in (1, 2, 3, 4)} == {8, 4, 2}
    for ch in ((16, 16), (32, 32)):
        assert {c['dims'] for c in pc.D2_PINNED if (c['cin'], c['cout']) == ch} >= set(pc.D2_SHAPES)
    assert [pc.wg_vox_per_wave(pc.vox(s), 8, *ch) for ch, s in pc.D2_WALK_NAMED] == [4, 4, 4, 4, 4]
    assert [pc.wg_vox_per_wave(pc.vox(s), 8, *ch) for ch, s, _ in pc.D2_WALK] == [v for _, _, v in pc.D2_WALK]
    # the wide layer whose narrower slice needs more partial bytes than a 64 x 64 slice: blocks x outputs of (48, 64) above those of (64, 64)
    (ci, co), s = pc.D2_WIDE_PARTIALS
    m = pc.vox(s)
    v48, v64 = pc.wg_vox_per_wave(m, 8, ci % 64, co), pc.wg_vox_per_wave(m, 8, 64, 64)
    assert (v48, v64) == (4, 8) and pc._cdiv(m, 4 * v48) * (ci % 64) * co > pc._cdiv(m, 4 * v64) * 64 * 64 and any((c['cin'], c['cout'], c['dims']) == (ci, co, s) for c in pc.D2_PINNED)
    (_, s0, _), (_, s1, _), (_, s2, _), (_, s3, _), _ = pc.D2_WALK
    assert s0[3] % 2 == 1 and s0[3] > 4 and s1[3] == 3 and s2[3] == 1 and s3[0] == 2
    # family 3: chunks per workgroup of the fused backward
    assert [pc.db_chunks_per_block(pc.vox(s)) for s in pc.UP_SHAPES] == pc.UP_CHUNKS
    assert pc._cdiv(16695, 32) == 522 and pc._cdiv(36378, 32) == 1137 and 36378 % 32 != 0 and pc.vox(pc.UP_SHAPES[5]) == 16384
    got = {(c['ch'], c['dims']) for c in pc.UP_PINNED if c['train'] and not c['chain']}
    assert {((32, 32), s) for s in pc.UP_SHAPES} <= got
    assert {c['ch'] for c in pc.UP_PINNED} == set(pc.UP_CH) and sum(c['chain'] for c in pc.UP_PINNED) == 2
    assert {(c['train'], c['slope'], c['lazy']) for c in pc.UP_PINNED} >= {(t, s, l) for t in (True, False) for s in (0.0, 0.01) for l in (True, False)}
    assert any(c['neg'] for c in pc.UP_PINNED)
    # family 4: every tile pair, and 12 voxels per wave on the pair path and on the single-load path
    assert {(c['cin'], c['cout']) for c in pc.BF_PINNED} >= set(pc.TILE_PAIRS)
    assert {(48, 96), (112, 64)} <= {(c['cin'], c['cout']) for c in pc.BF_PINNED}
    for c in pc.BF_PINNED[16:18]:
        assert pc.wg_vox_per_wave(c['m'], 1, c['cin'], c['cout']) == 12 and pc.wg_vox_per_wave(pc.vox(c['dims']), 8, c['cin'], c['cout']) >= 8, c
    # drawn examples: both prologue settings, at least six of the seven channel counts on each side and 12 pairs (the 60 examples reach 15), train and eval, the hand-over chain
    seen = []
    pc.run_cases(pc.C1, seen.append)
    assert {c['pro'] for c in seen} == {None, 0.0, 0.01} and len({c['cin'] for c in seen}) >= 6 and len({c['cout'] for c in seen}) >= 6 and len({(c['cin'], c['cout']) for c in seen}) >= 12
    seen = []
    pc.run_cases(pc.UP, seen.append)
    assert {c['ch'] for c in seen} == set(pc.UP_CH) and {c['train'] for c in seen} == {True, False} and any(c['chain'] for c in seen)
    for c in seen:
        inp = pc.build_up(c)
        assert not c['train'] or 8 * pc.vox(inp['dims']) >= pc.M_MIN
