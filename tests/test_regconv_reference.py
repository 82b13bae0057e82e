"""CPU companion of tests/test_gpu_regconv_shapes.py (no GPU): on the SAME derandomised examples (tests/regconv_cases.py run_cases), F.conv3d in fp32 on
torch-CPU -- the oracle, in the device's place -- must sit within a quarter of every tolerance of its float64 evaluation, in both matrix modes' tables, and the
guard-band cap must hold with the oracle deciding inside the band.  That makes each tolerance of the device test a statement about the kernel and the cap a
property of the generated inputs.  It also checks, without a GPU, that every pinned example still reaches the launcher branch and the tile / slab / grid counts
it names (regconv_cases.check_pinned: the launchers' predicates restated) and that the pinned sets name every branch the device file lists."""
import pytest
import torch

import regconv_cases as rc


def _quarter(family):
    """a quarter of the tighter of the two modes' tolerances, per quantity"""
    return {q: min(rc.TOL[family][m][q] for m in rc.MODES) / 4 for q in rc.QUANTITIES}


@pytest.mark.parametrize('family', rc.FAMILIES)
def test_inputs_are_well_conditioned(family):
    strategy, pinned = rc.FAMILY[family]
    tol = _quarter(family)

    def body(case):
        inp = rc.build(case)
        r32 = rc.ref(inp, torch.float32)
        r64 = rc.ref(inp, torch.float64, decided=r32['out'])
        rc.check_band(r64['band'])
        for k, n in r64['band']:
            rc.note('cpu ' + family, 'band elements', k)
        if (case.get('kind') or '').startswith('jump'):
            rc.compare_jump('cpu ' + family, inp, r32, r64, tol)
        else:
            rc.compare('cpu ' + family, r32, r64, tol)
    rc.run_cases(strategy, body, pinned=pinned)


def test_pinned_examples_reach_what_they_name():
    for family in rc.FAMILIES:
        for case in rc.FAMILY[family][1]:
            assert case['fam'] == family
            rc.check_pinned(case)
    S, F = 'fp32_split', 'fp32'

    def got(family, mode):
        return [(c, rc.reached(c, mode, rc.build_dims(c))) for c in rc.FAMILY[family][1]]
    # stride2: a slab of the native weight gradient walks a second and a third tile, for every (Cin, Cout) class of the native kernels; the masked and
    # direct classes; the structured kinds on a walked shape; fork
    s2 = got('stride2', S)
    assert {c['ch'] + (c['cout'],) for c, r in s2 if r['wgrad'] == 's2n' and r['walk'] >= 2} == {(ci, 0, co) for ci, co in rc.S2_NATIVE}
    assert {(r['tiles'], r['slabs']) for c, r in s2 if r['wgrad'] == 's2n'} >= {(1, 1), (8, 8), (36, 32), (129, 128), (257, 128), (65, 64), (66, 64)}
    assert {c['ch'][0:1] + (c['cout'],) for c, r in s2 if r['wgrad'] == 's2d'} == set(rc.S2_MASKED) and {c['ch'][0:1] + (c['cout'],) for c, r in s2 if r['wgrad'] == 'direct'} == set(rc.S2_DIRECT)
    assert all(r['wgrad'] != 's2n' for c, r in got('stride2', F))
    for fam in ('stride2', 'up2'):
        kinds = {c['kind']: r for c, r in got(fam, S) if c['kind']}
        assert set(kinds) == {'zero_first', 'zero_last', 'jump_dn', 'jump_up'} and all(r['walk'] == 2 and r['tiles'] == r['slabs'] + 1 for r in kinds.values())
        assert sum(c['fork'] for c in rc.FAMILY[fam][1]) >= 2
    # up2: every channel class of the table with its data-gradient N-tile count, the four Cout, the slab counts of up_wgrad_reduce_kernel's loop and tail, the walks
    up = got('up2', S)
    assert {(c['ch'], r['ntn']) for c, r in up} == set(rc.UP_CLASSES.items()) and {c['cout'] for c, r in up} == set(rc.UP_COUTS)
    assert {r['slabs'] for c, r in up} >= {1, 3, 4, 5, 8, 16, 64}
    assert {(sum(c['ch']), r['tiles'], r['slabs']) for c, r in up if r['walk'] >= 2} >= {(64, 9, 8), (64, 17, 8), (48, 9, 8), (32, 17, 16), (8, 65, 64)}
    assert all(r['wgrad'] == 'declined' for c, r in got('up2', F))
    assert not any(rc.upconv_supported(c1, c2, co, S) for c1, c2, co in rc.UP_DECLINED)
    # flow: the fifteen flowmm classes, the eighteen weight-gradient classes with their three templates in both kernels, the persistent grid's tile counts
    fl, flf = got('flow', S), got('flow', F)
    assert {(c['ch'], c['cout']) for c, r in fl if r['fwd'] == 'flowmm' and r['dgrad'] == 'flowmm'} == {(ch, co) for ch in rc.FLOWMM_CH for co in (1, 2, 3)}
    for rows, kern in ((fl, 'flow_split'), (flf, 'flow_fp32')):
        assert {(c['ch'], c['cout']) for c, r in rows if r['wgrad'] == kern} == {(ch, co) for ch in rc.FLOW_WGRAD_CH for co in (1, 2, 3)}
        assert {r['template'] for c, r in rows if r['wgrad'] == kern} == {(6, False, 8), (6, True, 8), (6, True, 16)}
    assert {r['wgrad'] for c, r in fl} >= {'swapped', 'generic', 'direct'} and {r['fwd'] for c, r in fl} >= {'thin', 'direct'} and all(r['fwd'] != 'flowmm' for c, r in flf)
    assert {r['tiles'] for c, r in fl if 'tiles' in r} >= set(rc.FLOW_TILE_SHAPES) and {r['wtiles'] for c, r in fl if 'wtiles' in r} >= set(rc.FLOW_TILE_SHAPES)
    assert {r['wtiles'] for c, r in flf if 'wtiles' in r} >= {v[1] for v in rc.FLOW_TILE_SHAPES.values()}
    assert {r['walk'] for c, r in fl if 'walk' in r} == {1, 2, 3} and {r['wwalk'] for c, r in flf if 'wwalk' in r} == {1, 2}
    assert {r['grid'] % 8 == 0 for c, r in fl if 'grid' in r} == {True, False}
    # first: the VALU kernel's strips, the exchanged form's tile counts, smallcin
    fi = got('first', S)
    va = [(c, r) for c, r in fi if r['wgrad'] == 'valu']
    assert {(c['cout'], c['h']) for c, r in va} >= {(co, hh) for co in (8, 16) for hh in (33, 34, 66, 67)}
    assert {(c['cout'], c['w'] - r['xw']) for c, r in va} >= {(co, k) for co in (8, 16) for k in (-1, 0, 1)}
    assert {r['tail'] for c, r in va} == {0, 1, 2} and {r['nys'] for c, r in va} == {1, 2, 3}
    assert any(r['ragged_x'] and r['tail'] and r['nys'] > 1 for c, r in va) and any(c['d'] == 1 for c, r in va) and any(c['n'] == 2 for c, r in va)
    assert any(r['strips'] > 2048 and r['wwalk'] == 2 for c, r in va)
    assert {r['wtiles'] for c, r in fi if r['wgrad'] == 'exchanged'} >= {1, 8, 9, 513} and {c['ch'] for c, r in fi if r['wgrad'] == 'exchanged'} == {(1, 0), (2, 0), (1, 1)}
    assert {c['ch'] for c, r in fi if r['wgrad'] == 'smallcin'} == set(rc.FIRST_CH)


def test_route_table_of_the_drawn_classes():
    """The route every drawn channel class takes, as the restated launchers give it (the table of the device file's docstring)."""
    S, F = 'fp32_split', 'fp32'

    def route(fam, ch, cout, mode, key):
        return rc.reached(dict(fam=fam, ch=ch, cout=cout, n=1, d=5, h=9, w=18), mode)[key]
    for ci, co in rc.S2_NATIVE:
        assert route('stride2', (ci, 0), co, S, 'fwd') == 's2n' and route('stride2', (ci, 0), co, F, 'fwd') == 's2d'
    for ci, co in rc.S2_MASKED:
        assert route('stride2', (ci, 0), co, S, 'wgrad') == route('stride2', (ci, 0), co, F, 'wgrad') == 's2d'
    for ci, co in rc.S2_DIRECT:
        assert route('stride2', (ci, 0), co, S, 'dgrad') == 'direct'
    for ch in rc.UP_CLASSES:
        for co in rc.UP_COUTS:
            assert route('up2', ch, co, S, 'fwd') == 'up2'
    for ch in rc.FLOW_CH:
        for co in (1, 2, 3, 4):
            want = 'flowmm' if (ch in rc.FLOWMM_CH and co <= 3) else ('direct' if ch == (12, 0) else 'thin')
            assert route('flow', ch, co, S, 'fwd') == want and route('flow', ch, co, F, 'fwd') == ('direct' if ch == (12, 0) else 'thin')
            wg = 'direct' if ch == (12, 0) else ('flow_split' if (ch in rc.FLOW_WGRAD_CH and co <= 3) else ('generic' if sum(ch) > 32 else 'swapped'))
            assert route('flow', ch, co, S, 'wgrad') == wg
    for ch in rc.FIRST_CH:
        for co in rc.FIRST_COUTS:
            wg = 'valu' if (ch == (1, 0) and co in (8, 16)) else ('exchanged' if (sum(ch) <= 2 and co <= 16) else 'smallcin')
            assert route('first', ch, co, S, 'wgrad') == route('first', ch, co, F, 'wgrad') == wg
            assert route('first', ch, co, S, 'fwd') == ('thin' if co >= 8 else 'direct')
