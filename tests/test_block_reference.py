"""CPU companion of tests/test_gpu_block_shapes.py (no GPU): on the SAME derandomised examples (tests/block_cases.py run_cases), the same composition
evaluated in fp32 on torch-CPU must sit within a quarter of every tolerance of its float64 evaluation, and the guard-band caps must hold with the fp32
oracle in the device's place (it decides inside the band, as the device does in the GPU file).  That makes each tolerance of the device test a statement
about the kernel and each cap a property of the generated inputs, and it stops a later edit of the strategies from drifting into ill-conditioned territory."""
import torch

import block_cases as bc


def _quarter(family):
    return {k: v / 4 for k, v in bc.TOL[family].items()}


def _family(name, strategy, pinned, build, ref):
    def body(case):
        inp = build(case)
        r32 = ref(inp, torch.float32)
        r64 = ref(inp, torch.float64, decided=r32)
        bc.check_band(r64['band'])
        for k, n in r64['band']:
            bc.note('cpu ' + name, 'band elements', k)
        bc.compare('cpu ' + name, r32, r64, _quarter(name))
    bc.run_cases(strategy, body, pinned=pinned)


def test_block_inputs_are_well_conditioned():
    _family('block', bc.BLOCK, bc.BLOCK_PINNED, bc.build_block, bc.ref_block)


def test_chain_inputs_are_well_conditioned():
    _family('chain', bc.CHAIN, bc.CHAIN_PINNED, bc.build_chain, bc.ref_chain)


def test_chain_pool_inputs_are_well_conditioned():
    """Also measures how often the pool's guard band is entered on the final examples (recorded as 'cpu chain_pool/band elements')."""
    _family('chain_pool', bc.POOL, bc.POOL_PINNED, bc.build_pool, bc.ref_pool)


def test_epilogue_sum_inputs_are_well_conditioned():
    """Family 4: the two convolutions in fp32 against float64, and fp32 column sums of their outputs in units of sum |term|."""
    q = _quarter('sums')

    def body(case):
        inp = bc.build_sums(case)
        y32, dx32 = bc.ref_sums(inp, torch.float32)
        y64, dx64 = bc.ref_sums(inp, torch.float64)
        bc.close('cpu sums', 'y', y32, y64, q['y'])
        bc.close('cpu sums', 'dx', dx32, dx64, q['dx'])
        t = y32.float().movedim(1, -1)
        for got, terms in ((t.sum((0, 1, 2, 3)), t), ((t * t).sum((0, 1, 2, 3)), t * t)):
            e = bc.col_err(got, terms)
            bc.note('cpu sums', 'sum', e)
            assert e < q['sum'], e
    bc.run_cases(bc.SUMS, body, pinned=bc.SUMS_PINNED)


def test_pinned_examples_reach_what_they_name():
    """The builders leave the pinned shapes alone (tile counts 1, 6, 7, 8, 9, 17 of the persistent grid), every channel and Cout class has its example, train-mode
    examples keep M_MIN voxels per channel and every conv stays within WORK_MAX unless that bound forbids it."""
    assert [bc.ntiles(*s) for s in bc.SHAPES_PINNED] == bc.SHAPES_TILES and {1, 7, 8, 9, 17} <= set(bc.SHAPES_TILES)
    assert {c['ch'] for c in bc.BLOCK_PINNED} == set(bc.CH_CLASSES) and {c['cout'] for c in bc.BLOCK_PINNED} == set(bc.COUTS)
    for pinned, build in ((bc.BLOCK_PINNED, bc.build_block), (bc.CHAIN_PINNED, bc.build_chain), (bc.SUMS_PINNED, bc.build_sums)):
        got = [build(c)['dims'] for c in pinned]
        assert set(bc.SHAPES_PINNED) <= set(got), (set(bc.SHAPES_PINNED) - set(got))
    # the N-tile branches: the launcher's own choice, restated, at the pinned tile counts -- and at no other example of family 1
    for mode, want in (('fp32_split', [2, 2, 2, 1]), ('fp32', [2, 1, 2, 3])):
        assert [bc.launcher_nrep(bc.ntiles(*s), co, mode) for s, co in bc.NREP_PINNED] == want, mode
    assert [bc.launcher_nrep(bc.ntiles(*s), co, 'fp32_split', pro=True) for s, co in ((((1, 1, 3, 4112)), 32), ((1, 1, 1, 2050), 64))] == [2, 2]
    for pinned, build, key in ((bc.BLOCK_PINNED, bc.build_block, 'cout'), (bc.SUMS_PINNED, bc.build_sums, 'cout'), (bc.CHAIN_PINNED, bc.build_chain, 'cout')):
        reached = {(c[key], bc.launcher_nrep(bc.ntiles(*build(c)['dims']), c[key], 'fp32_split')) for c in pinned}
        assert {(32, 2), (64, 2)} <= reached and (key != 'cout' or pinned is bc.CHAIN_PINNED or (48, 2) in reached), reached
    seen = []

    def body(case):
        inp = bc.build_chain(case)
        n, d, h, w = inp['dims']
        seen.append(case)
        if case['train']:
            assert n * d * h * w >= bc.M_MIN
        for p in inp['blocks']:
            assert n * d * h * w * p['cin'] * p['cout'] <= bc.WORK_MAX or n * d * h * (w - 1) < bc.M_MIN or (w == 1 and h == 1)
    bc.run_cases(bc.CHAIN, body, pinned=bc.CHAIN_PINNED)
    assert seen[:len(bc.CHAIN_PINNED)] == bc.CHAIN_PINNED
    assert {c['form'] for c in seen} == {'single', 'lazy_skip', 'skip_lazy'} and {c['train'] for c in seen} == {True, False}
    assert {c['c'] for c in bc.POOL_PINNED} == {8, 12, 16, 32} and any(c['neg'] for c in bc.POOL_PINNED) and any(c['neg'] for c in bc.CHAIN_PINNED)
