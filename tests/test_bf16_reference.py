"""CPU companion of tests/test_gpu_bf16_shapes.py (no GPU): on the SAME pinned and derandomised examples (tests/bf16_cases.py run_cases) an fp32 torch-CPU oracle that
rounds to bf16 wherever the product stores a tensor must meet the bounds the device is held to with the project's quarter margin -- fp32 results within a quarter of each tolerance, stored tensors within
bf16_close and the rounding-mode check at a quarter of their tol, neither below the floor of eight fp32 roundings -- and the conditioning facts the device test relies on must hold with the oracle in the device's place: the guard-band caps, the
share of a tensor left out of the rounding-mode check (at most 20 %), the share of pooling windows with a tied maximum (at least 30 %), and torch's own tie rule.  Four
deliberately wrong oracles show that the bounds have teeth, and a ledger holds every `_bf16` entry point to a test."""
import pytest
import torch
import torch.nn.functional as F

import bf16_cases as bx
import pointwise_cases as pc


_quarter = bx.quarter


def _report(*families):
    """the conditioning figures of the run so far: the worst left-out share per stored tensor, the tie share, the guard-band counts"""
    for k, v in sorted(bx.lc.WORST.items()):
        if any(f in k for f in families) and ('left-out' in k or 'tied' in k or 'band' in k):
            print('%-90s %.3g' % (k, v[0]))


# ---- family `stream` -----------------------------------------------------------------------------------------------------------------
def _stream_body(case, wrong=None):
    """wrong: None | 'trunc' (a truncating store)"""
    q, tol = _quarter('stream'), bx.TOL['stream']
    inp = bx.build_stream(case)
    o = bx.stream_oracle(inp)
    if wrong == 'trunc':
        for k in ('y', 'dx_train', 'dx_eval', 'act_dx', 'add_dx'):
            o[k] = bx.trunc_bf16(o[k + '_f32'])
    r = bx.ref_stream(inp, torch.float64, decided=o)
    bx.check_band(r['band'])
    for k, n in r['band']:
        bx.note('cpu stream', 'band elements', k)
    bx.close('cpu stream', 'stats', o['stats'], r['stats'], q['stats'])
    bx.close('cpu stream', 'run', o['rm'], r['rm'], q['run'])
    bx.close('cpu stream', 'run', o['rv'], r['rv'], q['run'])
    bx.close('cpu stream', 'dgamma', o['dgamma'], r['dgamma'], q['dgamma'])
    bx.close('cpu stream', 'dbeta', o['dbeta'], r['dbeta'], q['dbeta'])
    # stored tensors: the oracle at a quarter of the device's tol (not below the floor), the left-out cap at the device's tol
    bx.stored_close('stream y (cpu)', o['y'], r['y'], q['out'], cap_tol=tol['out'])
    bx.stored_close('stream dx train (cpu)', o['dx_train'], r['dx_train'], q['dx'], unit=r['dx_unit'], cap_tol=tol['dx'])
    bx.stored_close('stream dx eval (cpu)', o['dx_eval'], r['dx_eval'], q['dx'], cap_tol=tol['dx'])
    bx.check_act_dx('stream act_bwd dx (cpu)', o['act_dx'], r['act_dx'], r['af'], inp['slope'], q['act'])
    bx.check_act_dx('stream act_bwd_add dx (cpu)', o['add_dx'], r['add_dx'], r['af'], inp['slope'], q['act'])
    # the two bias-gradient routes: sums of the fp32 dx before the store (fused) and of the stored dx (stand-alone), each against the float64 sum of what it sums
    for k in ('dx_train', 'dx_eval', 'add_dx'):
        units = r['dx_units'] if k == 'dx_train' else None
        bx.sum_close('cpu stream', 'sum', bx.oracle_colsum(o[k + '_f32']), r[k], q['sum'], units)
        bx.sum_close('cpu stream', 'sum', bx.oracle_colsum(o[k]), o[k], q['sum'], units)
    bx.sum_close('cpu stream', 'sum', bx.oracle_colsum(inp['x']), inp['x'], q['sum'])


def test_stream_inputs_are_well_conditioned():
    bx.run_cases(bx.STREAM, _stream_body, pinned=bx.STREAM_PINNED)
    _report('stream')


@pytest.mark.parametrize('case', bx.STREAM_LARGE, ids=lambda c: '%dx%d' % (c['m'], c['c']))
def test_stream_large_inputs_are_well_conditioned(case):
    bx.lc._state['case'] = case
    _stream_body(case)
    bx.write_report()


def _act_bwd(numel, slope, sd):
    g = bx.to_bf16(bx.nrm((numel,), sd))
    y = bx.to_bf16(bx.nrm((numel,), sd + 1) + 1.0)
    y[::7] = 0.0
    return g, y, g * (torch.ones_like(y) if slope < 0 else torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope)))


def test_act_bwd_sizes():
    """numel % 4 = 0 ... 3 and numel = 1, 3: at slopes -1 and 0 the fp32 product is exact, at 0.01 the stored value is the rounding of the float64 product"""
    for i, numel in enumerate(bx.ACT_NUMEL[:-1]):
        for slope in bx.SLOPES:
            g, y, dx32 = _act_bwd(numel, slope, 70 + i)
            ref = g.double() * (torch.ones_like(y) if slope < 0 else torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))).double()
            if slope <= 0:
                assert torch.equal(dx32.double(), ref)
                bx.bits_equal('act_bwd', bx.to_bf16(dx32), ref)
            elif numel > 100:
                bx.stored_close('stream act_bwd dx (cpu)', bx.to_bf16(dx32), ref, bx.TOL['stream']['act'])


# ---- family `pool` -------------------------------------------------------------------------------------------------------------------
def _pool_body(case, ties, wrong=None):
    tol = bx.TOL['pool']
    inp = bx.build_pool(case)
    r32, r64 = bx.ref_pool(inp, torch.float32), bx.ref_pool(inp, torch.float64)
    t, n = bx.tie_counts(inp['x'])
    ties[0] += t
    ties[1] += n
    # torch's own MaxPool3d backward in float64 routes to the first maximum in (d, h, w) order: the reference's tie rule is checked, not assumed
    leaf = bx._ncdhw(inp['x'].double()).clone().requires_grad_(True)
    F.max_pool3d(leaf, 2).backward(bx._ncdhw(inp['dy'].double()))
    assert torch.equal(bx._ndhwc(leaf.grad), r64['routed']), case
    routed = bx.pool_route(inp['x'], inp['dy'], last=True) if wrong == 'last' else r32['routed']
    if wrong == 'plane':                                      # a trailing plane left unset
        routed = routed.clone()
        n_, d, h, w = inp['dims']
        if d % 2:
            routed[:, -1] = float('nan')
        elif h % 2:
            routed[:, :, -1] = float('nan')
        elif w % 2:
            routed[:, :, :, -1] = float('nan')
    bx.bits_equal('pool y', r32['y'], r64['y'])
    bx.bits_equal('pool dx', routed, r64['routed'])
    bx.bits_equal('pool dx add', bx.to_bf16(inp['gskip'] + routed), bx.rne(r64['dx_add']))
    bx.stored_close('pool act (cpu)', bx.to_bf16(r32['act']), r64['act'], bx.quarter_of(tol['act']), cap_tol=tol['act'])
    for k in (0, 1):
        bx.bits_equal('pool up', r32['up%d' % k], r64['up%d' % k])
        bx.stored_bound('pool up dx (cpu)', bx.to_bf16(r32['up_dx%d' % k]), r64['up_dx%d' % k], bx.quarter_of(tol['up_dx']))      # (sums of bf16 values sit on rounding midpoints: no mode check)


def test_pool_inputs_are_well_conditioned():
    ties = [0, 0]
    bx.run_cases(bx.POOL, lambda c: _pool_body(c, ties), pinned=bx.POOL_PINNED)
    share = ties[0] / ties[1]
    bx.note('cpu pool', 'share of windows with a tied maximum', share)
    bx.write_report()
    _report('pool')
    assert share >= bx.TIE_MIN, share


# ---- family `head` -------------------------------------------------------------------------------------------------------------------
def _head_body(case, wrong=None):
    q, tol = _quarter('head'), bx.TOL['head']
    inp = bx.build_head(case)
    act = None
    if inp['pro'] is not None:
        a32, a64 = bx.head_act(inp, torch.float32), bx.head_act(inp, torch.float64)
        act = bx.trunc_bf16(a32) if wrong == 'trunc' else bx.to_bf16(a32)
        bx.stored_close('head act (cpu)', act, a64, bx.F32_FLOOR)
    r32, r64 = bx.ref_head(inp, torch.float32, act), bx.ref_head(inp, torch.float64, act)
    e = bx.scalar_err(r32['loss'], r64['loss'], 'rel1')
    bx.note('cpu head', 'loss', e)
    assert e < q['loss'], e
    for k in ('coef', 'dw', 'db'):
        bx.close('cpu head', k, r32[k], r64[k], q[k])
    bx.stored_close('head dx (cpu)', bx.trunc_bf16(r32['dx']) if wrong == 'trunc' else bx.to_bf16(r32['dx']), r64['dx'], q['dx'], cap_tol=tol['dx'])


def test_head_inputs_are_well_conditioned():
    bx.run_cases(bx.HEAD, _head_body, pinned=bx.HEAD_PINNED)
    _report('head')


def test_head_coefficients_are_the_gradient_of_the_loss():
    """ref_head's coef (written out) against autograd of the same loss with respect to the probabilities"""
    inp = bx.build_head(bx.HEAD_PINNED[8])
    N, V, C = inp['N'], inp['V'], inp['c']
    p = torch.softmax(inp['x'].double() @ inp['w'].double() + inp['b'].double(), -1).requires_grad_(True)
    onehot = F.one_hot(inp['labels'].long(), C).double()
    den = p.sum(1) + onehot.sum(1) + 2 * bx.HEAD_EPS
    (1 - ((2 * (p * onehot).sum(1) + bx.HEAD_EPS) / den).sum() / (N * C)).backward()
    coef = bx.ref_head(inp, torch.float64)['coef']
    assert torch.allclose(p.grad, coef[0].unsqueeze(1) * onehot + coef[1].unsqueeze(1), rtol=1e-12, atol=1e-18)
    from oracle import losses
    x = bx._ncdhw((inp['x'].double() @ inp['w'].double() + inp['b'].double()).reshape(N, V, 1, 1, C))
    assert abs(float(losses.dice_loss(x, inp['labels'].long().reshape(N, V, 1, 1), C, 'Uniform', False, True, bx.HEAD_EPS)) - bx.ref_head(inp, torch.float64)['loss']) < 1e-12


# ---- family `conv3` ------------------------------------------------------------------------------------------------------------------
def _c3_compare(family, case, got, r, stored, tol, what=('y', 'dx1', 'dx2', 'dw')):
    """got: a side's results with its stored tensors already rounded"""
    for k in what:
        if r.get(k) is None:
            continue
        q = 'dx' if k.startswith('dx') else k
        if q != 'dw' and stored[q]:
            bx.stored_close('conv3 %s %s (cpu)' % (case['kind'], q), got[k], r[k], bx.quarter_of(bx.c3_tol(case['kind'])[q]), cap_tol=bx.c3_tol(case['kind'])[q])
        else:
            bx.close(family, '%s %s' % (case['kind'], q), got[k], r[k], tol[q])


def _conv3_body(case):
    stored = bx.c3_stored(case)
    tol = {k: bx.quarter_of(v) for k, v in bx.c3_tol(case['kind']).items()}
    inp = bx.build_conv3(case)
    r32 = bx.ref_conv3(inp, torch.float32)
    o = dict(r32, y=bx.to_bf16(r32['y']) if stored['y'] else r32['y'])
    for k in ('dx1', 'dx2'):
        if stored['dx'] and r32[k] is not None:
            o[k] = bx.to_bf16(r32[k])
    r = bx.ref_conv3(inp, torch.float64, decided=o['y'])
    bx.check_band(r['band'])
    _c3_compare('cpu conv3', case, o, r, stored, tol)
    if case['kind'] == 'mfma':
        # the statistics epilogue: sums of the unrounded convolution result
        z = r32['z'].float().movedim(1, -1).reshape(-1, inp['cout'])
        bx.sum_close('cpu conv3', 'sum', bx.oracle_colsum(z), r['z'].movedim(1, -1).reshape(-1, inp['cout']), bx.quarter('conv3')['sum'])
        bx.sum_close('cpu conv3', 'sum', bx.oracle_colsum(z * z), (r['z'] ** 2).movedim(1, -1).reshape(-1, inp['cout']), bx.quarter('conv3')['sum'])
        # the prologue: the stored activated tensors, then the convolution and the weight gradient on them
        acts = {}
        for i in (1, 2) if (case['pro'] != 'in1' and inp['c2']) else (1,):
            a32, a64 = bx.pro_act(inp, i, 0.01, torch.float32), bx.pro_act(inp, i, 0.01, torch.float64)
            acts['x%d' % i] = bx.to_bf16(a32)
            bx.stored_close('conv3 act (cpu)', acts['x%d' % i], a64, bx.TOL['conv3']['act'])
        p32, p64 = bx.ref_conv3(inp, torch.float32, slope=-1.0, **acts), bx.ref_conv3(inp, torch.float64, slope=-1.0, **acts)
        _c3_compare('cpu conv3 pro', case, dict(p32, y=bx.to_bf16(p32['y'])), p64, stored, tol, what=('y', 'dw'))


def test_conv3_inputs_are_well_conditioned():
    bx.check_c3_pinned()
    bx.run_cases(bx.C3, _conv3_body, pinned=bx.C3_PINNED)
    _report('conv3')


def test_conv3_drawn_examples_reach_every_kind():
    seen = []
    bx.run_cases(bx.C3, seen.append)
    assert {c['kind'] for c in seen} == {'mfma', 's2', 'first', 'flow'}
    for c in seen + bx.C3_PINNED:      # work per convolution (output voxels x Cin x Cout) within block_cases.WORK_MAX
        inp = bx.build_conv3(c)
        assert inp['dims'][0] * inp['odims'][0] * inp['odims'][1] * inp['odims'][2] * (inp['c1'] + inp['c2']) * inp['cout'] <= bx.bc.WORK_MAX, c
    routes = {(c['kind'],) + bx.c3_routes(c) for c in seen}
    assert {('mfma', 'mfma', 'mfma', 'mfma'), ('mfma', 'mfma', None, 'mfma'), ('s2', 's2', 's2', 's2'), ('s2', 's2', None, 's2'), ('first', 'thin', 'thin', 'fewcin'),
            ('flow', 'thin', 'thin', 'flow')} <= routes, routes
    # the masks: an absent second input still takes its bit position (the output of the forward is bit 2 with or without in2)
    assert bx.c3_want('fwd', 0) == 5 and bx.c3_want('fwd', 16) == 7 and bx.c3_want('dgrad', 0) == 3 and bx.c3_want('dgrad', 16) == 7 and bx.c3_want('wgrad', 0) == 5
    # every partial mask of an all-bf16 matrix shape declines
    for entry in ('fwd', 'dgrad', 'wgrad'):
        assert [m for m in range(8) if bx.c3_route(entry, 16, 16, 16, 1, m) is not None] == [7], entry
        assert [m for m in range(8) if bx.c3_route(entry, 16, 0, 16, 1, m) is not None] == sorted({bx.c3_want(entry, 0), bx.c3_want(entry, 0) | (4 if entry == 'dgrad' else 2)}), entry


# ---- the launcher decisions of family `stream` and the ledger ----------------------------------------------------------------------------
def test_stream_pinned_examples_reach_what_they_name():
    for c in bx.STREAM_FUSED + bx.STREAM_ALONE + bx.STREAM_VEC1:
        p, rows = bx.plan_rows(1, c), bx.stream_rows(c)
        assert p['vec'] == (4 if c % 4 == 0 else 1) and p['block'] <= 256
        assert [bx.plan_rows(m, c)['grid'] for m in rows] == [1, 1, 2, 1, 1], c
        assert rows[3] % 2 == 1 and {x['m'] for x in bx.STREAM_PINNED if x['c'] == c} == set(rows)
    assert all(bx.fused_dxsum(c) for c in bx.STREAM_FUSED) and not any(bx.fused_dxsum(c) for c in bx.STREAM_ALONE + bx.STREAM_VEC1)
    assert {x['slope'] for x in bx.STREAM_PINNED} == set(bx.SLOPES)
    # a workgroup whose rows start at or past M needs the 1024-workgroup cap: below it rows_per_block <= rpi * 16 < M / (grid - 1)
    assert all(bx.idle_workgroups(m, c) == 0 for c in (3, 12, 64) for m in list(range(1, 3000)) + [100000, 262144])
    p = bx.plan_rows(bx.STREAM_CAP['m'], 64)
    assert (p['grid'], p['rows_per_block'], bx.idle_workgroups(bx.STREAM_CAP['m'], 64)) == (1024, 257, 3)
    # bn_act_fwd: quads per grid stride
    stride = bx.da_grid(10 ** 9) * 256
    assert bx.STREAM_CAP['m'] * 16 > 3 * stride and bx.STREAM_STRIDE['m'] * 3 > stride and stride % 3 != 0
    assert {n % 4 for n in bx.ACT_NUMEL} == {0, 1, 2, 3} and {1, 3} <= set(bx.ACT_NUMEL) and bx.ACT_NUMEL[-1] // 4 > stride
    seen = []
    bx.run_cases(bx.STREAM, seen.append)
    assert {c['c'] for c in seen} == set(bx.STREAM_FUSED + bx.STREAM_ALONE) and {c['slope'] for c in seen} == set(bx.SLOPES)
    # head: the chunk classes; pool: every parity combination
    assert {(-(-v // 256)) for v in bx.HEAD_V} == {1, 2, 3, 5} and {c['ch'] for c in bx.HEAD_PINNED} == set(bx.HEAD_CH)
    assert {(c['d'] % 2, c['h'] % 2, c['w'] % 2) for c in bx.POOL_PINNED} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}


def test_every_bf16_entry_point_is_claimed():
    """the ledger: every name of _native.BF16_TWINS and BF16_MASKED_TWINS is tested entry by entry, by bf16_cases' families or by family 4 of pointwise_cases, and every
    claimed name is an entry point"""
    from deepatlas_amd import _native as nat
    mine = [n for names in bx.claimed().values() for n in names]
    assert len(set(mine)) == len(mine) and not set(mine) & set(bx.POINTWISE_CLAIMED)
    assert set(mine) | set(bx.POINTWISE_CLAIMED) == set(nat.BF16_TWINS) | set(nat.BF16_MASKED_TWINS)
    assert set(bx.claimed()['conv3']) == set(nat.BF16_MASKED_TWINS)
    for n in mine + bx.POINTWISE_CLAIMED:
        assert n in nat.SIGNATURES and n + '_bf16' in nat.SIGNATURES, n
    src = open(__file__.replace('test_bf16_reference.py', 'test_gpu_bf16_shapes.py')).read()
    assert all("'%s'" % n in src for n in mine)
    src = open(__file__.replace('test_bf16_reference.py', 'test_gpu_pointwise_shapes.py')).read()
    assert all(n in src for n in bx.POINTWISE_CLAIMED)


# ---- the bounds have teeth -------------------------------------------------------------------------------------------------------------
def _fails_somewhere(body, cases):
    n = 0
    for c in cases:
        bx.lc._state['case'] = c
        try:
            body(c)
        except AssertionError:
            n += 1
    return n


def test_wrong_oracles_fail():
    """a truncating store, last-maximum routing, a dropped scalar tail and a trailing plane left unset each fail on pinned examples"""
    assert _fails_somewhere(lambda c: _stream_body(c, wrong='trunc'), bx.STREAM_PINNED) == len(bx.STREAM_PINNED)
    assert _fails_somewhere(lambda c: _head_body(c, wrong='trunc'), bx.HEAD_PINNED[:7]) == 7
    assert _fails_somewhere(lambda c: _pool_body(c, [0, 0], wrong='last'), bx.POOL_PINNED) >= len(bx.POOL_PINNED) - 2
    odd = [c for c in bx.POOL_PINNED if (c['d'] | c['h'] | c['w']) & 1]
    assert len(odd) >= 8 and _fails_somewhere(lambda c: _pool_body(c, [0, 0], wrong='plane'), odd) == len(odd)
    # the scalar tail: the last numel % 4 elements keep the NaN prefill -> bits_equal / bf16_close's finiteness assertion
    for numel in (1, 3, 5, 6, 7, 1021, 1022, 1023):
        g, y, dx = _act_bwd(numel, 0.0, 5)
        dropped = bx.to_bf16(dx)
        dropped[numel // 4 * 4:] = float('nan')
        with pytest.raises(AssertionError):
            bx.bits_equal('act_bwd', dropped, dx)
        with pytest.raises(AssertionError):
            pc.bf16_close('stream act_bwd dx (cpu)', dropped, dx.double(), bx.TOL['stream']['act'])
