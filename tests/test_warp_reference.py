"""CPU companion of tests/test_gpu_warp_shapes.py (no GPU): on the SAME derandomised examples (tests/warp_cases.py through loss_cases.run_cases) the fp32
CPU oracle -- oracle.nets.identity_transform / warp_trilinear, torch.softmax and oracle.losses.dice_loss in fp32 -- must sit within a quarter of each
tolerance of the float64 reference, so that a tolerance of the device test is a statement about the kernel and not about the drawn inputs.  One
exception, stated with its reason at warp_cases.COORD_ERR: a sampled value (warped, d_src, the label warp's forward) carries the fp32 voxel coordinate's
rounding, which grows with the axis length, and on the volumes longer than 17 voxels the bound is COORD_ERR per voxel of length instead.  It also
asserts the conditioning the device test relies on: no coordinate of a drawn field lies within warp_cases.DELTA of an integer (the trilinear grid gradient
is one-sided there), no drawn case leaves a comparison out (the bodies below have no branch that does; a lattice case differs only in HOW d_disp is
compared), a non-finite or huge displacement gives finite references with exactly zero d_disp at its voxel, and the explicit examples name every class count
and launcher branch they claim."""
import torch

import warp_cases as wc


def _quarter(family, key):
    return wc.TOL[family][key] / 4


def _sampled(family, key, vol):
    """The bound for a SAMPLED value (the warped tensor, and d_src, its transpose): a quarter of the tolerance up to an axis of 17 voxels, then
    warp_cases.COORD_ERR per voxel of the longest axis, never above the tolerance itself."""
    return min(wc.TOL[family][key], max(wc.TOL[family][key] / 4, wc.COORD_ERR * (max(vol) - 1)))


def _field_ok(case, inp):
    """drawn fields are off the lattice; the voxels with non-finite coordinates are exactly the ones the case put there"""
    if wc.is_lattice(case):
        assert wc.lattice_distance(inp['disp'], inp['vol']) < wc.LATTICE_STEP
    else:
        assert wc.lattice_distance(inp['disp'], inp['vol']) >= wc.DELTA, case
    assert int(inp['bad'].sum()) == (4 if case.get('field') == 'nonfinite' else 0)


def _d_disp(family, case, inp, got, ref, ref_d_disp):
    tol = _quarter(family, 'd_disp')
    if wc.is_lattice(case):
        wc.close_either('cpu ' + family, 'd_disp', got, *wc.lattice_sides(ref_d_disp, inp), tol)
    else:
        wc.close('cpu ' + family, 'd_disp', got, ref, tol)
    bad = inp['bad'].expand_as(ref)
    assert float(ref[bad].abs().sum()) == 0.0 and float(got[bad].abs().sum()) == 0.0


def test_warp_inputs_are_well_conditioned():
    def body(case):
        inp = wc.build_warp(case)
        _field_ok(case, inp)
        r32, r64 = wc.ref_warp(inp, torch.float32), wc.cached(wc.ref_warp, case, inp)
        wc.close('cpu warp', 'warped', r32['warped'], r64['warped'], _sampled('warp', 'warped', inp['vol']))
        wc.close('cpu warp', 'deform', r32['deform'], r64['deform'], _quarter('warp', 'deform'))
        assert (r64['d_src'] is None) == (case['grads'] == 'disp') and (r64['d_disp'] is None) == (case['grads'] == 'src')
        if r64['d_src'] is not None:
            wc.close('cpu warp', 'd_src', r32['d_src'], r64['d_src'], _sampled('warp', 'd_src', inp['vol']))
        if r64['d_disp'] is not None:
            _d_disp('warp', case, inp, r32['d_disp'], r64['d_disp'], wc.ref_warp_d_disp)
    wc.run_cases(wc.WARP, body, pinned=wc.WARP_PINNED)


def test_warp_labels_inputs_are_well_conditioned():
    def body(case):
        inp = wc.build_warplabels(case)
        _field_ok(case, inp)
        r32, r64 = wc.ref_warplabels(inp, torch.float32), wc.cached(wc.ref_warplabels, case, inp)
        wc.close('cpu warplabels', 'fwd', r32['fwd'], r64['fwd'], _sampled('warplabels', 'fwd', inp['vol']))
        _d_disp('warplabels', case, inp, r32['d_disp'], r64['d_disp'], wc.ref_warplabels_d_disp)
    wc.run_cases(wc.WARPLABELS, body, pinned=wc.WARPLABELS_PINNED)


def test_label_warp_dice_inputs_are_well_conditioned():
    def body(case):
        inp = wc.build_lwd(case)
        _field_ok(case, inp)
        r32, r64 = wc.ref_lwd(inp, torch.float32), wc.cached(wc.ref_lwd, case, inp)
        wc.close('cpu lwd', 'loss', r32['loss'], r64['loss'], _quarter('lwd', 'loss'), 'rel1')
        _d_disp('lwd', case, inp, r32['d_disp'], r64['d_disp'], wc.ref_lwd_d_disp)
    wc.run_cases(wc.LWD, body, pinned=wc.LWD_PINNED)


def test_seg_phase_inputs_are_well_conditioned():
    def body(case):
        inp = wc.build_seg(case)
        _field_ok(case, inp)
        r32, r64 = wc.ref_seg(inp, torch.float32), wc.cached(wc.ref_seg, case, inp)
        wc.close('cpu segphase', 'loss', r32['l_sup'], r64['l_sup'], _quarter('segphase', 'loss'), 'rel1')
        wc.close('cpu segphase', 'loss', r32['l_anat'], r64['l_anat'], _quarter('segphase', 'loss'), 'rel1')
        wc.close('cpu segphase', 'dlogits', r32['dlogits'], r64['dlogits'], _quarter('segphase', 'dlogits'))
    wc.run_cases(wc.SEG, body, pinned=wc.SEG_PINNED)


def test_adjoint_scatter_reference_is_the_adjoint_of_the_warp():
    """warp_cases.adjoint_scatter_ref against autograd: sum_c B[c] g[c] + A g_out is the gradient of sum(warp(x) * onehot+(labels)) with respect to x, for
    labels outside [0, C) and a NaN coordinate as well."""
    g = torch.Generator().manual_seed(3)
    N, D, H, W, C = 2, 4, 5, 9, 3
    u = torch.randn((N, D, H, W, 3), generator=g) * torch.tensor([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)]) * 1.5
    u[0, 1, 2, 3, 1] = float('nan')
    lab = torch.randint(-1, C + 2, (N, D, H, W), generator=g)
    A, B = wc.adjoint_scatter_ref(u, lab, C)
    disp = u.permute(0, 4, 1, 2, 3).contiguous()
    inp = dict(disp=disp, vol=(D, H, W), bad=wc.bad_voxels(disp, (D, H, W)))
    assert int(inp['bad'].sum()) == 1
    _, _, grid = wc._grid(inp, torch.float64, None, False)
    x = torch.ones((N, C + 1, D, H, W), dtype=torch.float64, requires_grad=True)
    l = lab.long()
    sel = torch.zeros((N, C + 1, D, H, W), dtype=torch.float64).scatter_(1, torch.where((l >= 0) & (l < C), l, torch.full_like(l, C)).unsqueeze(1), 1.0)
    (wc.nets.warp_trilinear(x, grid) * sel).sum().backward()
    ref = x.grad.reshape(N, C + 1, -1)
    assert float((B - ref[:, :C]).abs().max()) < 1e-6 and float((A - ref[:, C]).abs().max()) < 1e-6      # (the scatter's identity grid is formed in fp32)
    assert float(A.sum()) > 0


def test_pinned_cases_name_their_branches():
    """what the docstring of tests/test_gpu_warp_shapes.py claims about the explicit examples, derived from the launcher formulas of warp.hip"""
    cdiv = lambda a, b: -(-a // b)
    V = lambda c: c['vol'][0] * c['vol'][1] * c['vol'][2]
    P = wc.WARP_PINNED
    assert {c['C'] for c in P} == set(wc.WARP_C) and {c['n'] for c in P} >= {1, 2, 3, 65536}
    grouped = [c for c in P if c['C'] in (8, 16, 32) and c['n'] <= 65535]
    assert {cdiv(V(c), 512) % 8 == 0 for c in grouped} == {True, False} and any(3584 < V(c) <= 4096 for c in grouped)
    assert any(V(c) % 64 and V(c) % 256 and V(c) % 512 and V(c) > 512 for c in grouped)
    assert any(c['C'] == 8 and c['n'] == 65536 and V(c) == 8 for c in P)
    for C in (3, 4, 16, 64, 128, 260):
        assert {c['grads'] for c in P if c['C'] == C} >= {'both', 'src', 'disp'}
    lpv = lambda C: C // 4 if C % 4 == 0 and (C // 4) & (C // 4 - 1) == 0 and C // 4 <= 64 else 1
    assert any(cdiv(c['n'] * V(c) * lpv(c['C']), 256) % 8 == 0 for c in P if c['C'] == 64) and any(cdiv(c['n'] * V(c), 256) % 8 == 0 for c in P if c['C'] in (3, 4))
    for pinned in (wc.WARP_PINNED, wc.WARPLABELS_PINNED, wc.LWD_PINNED, wc.SEG_PINNED):
        assert {c.get('field', 'rand') for c in pinned} == {'rand', 'zero', 'shift', 'nonfinite'}
    assert {c['C'] for c in wc.WARPLABELS_PINNED} == set(wc.WARPLABELS_C) and {c['wide'] for c in wc.WARPLABELS_PINNED} == {False, True}
    L = wc.LWD_PINNED
    assert {c['C'] for c in L} == set(range(1, 65)) and {c['n'] for c in L} >= {1, 2, 3, 64}
    assert {(c['wt'], c['no_bg']) for c in L} == {(w, b) for w in wc.WEIGHTS for b in (False, True)} and {(c['wm'], c['wtg']) for c in L} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c['km'] == 'const' and c['kt'] == 'const' for c in L) and any(c['C'] == 64 and c['km'] == 'iid' and c['kt'] == 'iid' for c in L)
    assert any(V(c) % 64 for c in L) and any(cdiv(V(c), 512) % 8 == 0 for c in L)
    S = wc.SEG_PINNED
    assert {(c['C'], c['labelled']) for c in S} == {(C, b) for C in wc.SEG_C for b in (False, True)} and {c['n'] for c in S} == {1, 2} and {c['ups'] for c in S} == {'both', 'anat'}
    tv = lambda C: 128 if C == 64 else 256
    for C in wc.SEG_C:
        assert any(c['n'] * cdiv(V(c), tv(C)) % 8 == 0 for c in S if c['C'] == C) and any(c['n'] * cdiv(V(c), tv(C)) % 8 and V(c) % tv(C) for c in S if c['C'] == C), C
        nb = lambda c: cdiv(V(c), 1024 // lpv(C))
        assert any(nb(c) % 8 == 0 for c in S if c['C'] == C) or C == 16, C
    assert any(cdiv(V(c), 256) % 8 for c in S if c['C'] == 16)


def test_both_files_see_the_same_examples():
    a, b = [], []
    wc.run_cases(wc.SEG, a.append, pinned=wc.SEG_PINNED)
    wc.run_cases(wc.SEG, lambda case: b.append(dict(case)), pinned=wc.SEG_PINNED)
    assert a == b and a[:len(wc.SEG_PINNED)] == wc.SEG_PINNED
    w = []
    wc.run_cases(wc.WARP, w.append, pinned=wc.WARP_PINNED)
    assert {c['C'] for c in w[len(wc.WARP_PINNED):]} <= set(wc.WARP_C) and {c['amp'] for c in w} == set(wc.AMPS)
