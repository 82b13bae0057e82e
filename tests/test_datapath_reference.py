"""CPU companion of tests/test_gpu_datapath_shapes.py: validates the references and the case builders of tests/datapath_cases.py without a GPU.

  * Adam: the float64 reference with Python's hyper-parameters is torch.optim.Adam in float64 (1e-12).  With the float32-rounded hyper-parameters the C ABI
    receives it deviates from that BY CONSTRUCTION: 1 - float32(0.999) is 1.29e-5 (relative) off 1 - 0.999, so v, which scales with it, is off by as much and
    sqrt(v) and the update by half of it, 6.45e-6 of the displacement; 1 - float32(0.9) adds 2.4e-7 through m and float32(lr) up to 6e-8.  The first step from zero
    moments at t = 100 000, where the bias correction no longer hides the factor, shows the whole of it; the test derives the figure from the roundings
    (datapath_cases.adam_hyper_dev) and asserts the deviation at 1.1 x that.  That is how far FlatAdam is from torch's Adam by construction.
  * the fp32 restatement of the kernel's expression order against the float64 reference: the "fp32 oracle worst" figures of the tolerance rule (family 'adam_f32').
  * da_adam_host_state, a pure host function, through the C ABI.
  * the layout references against F.conv3d / F.conv_transpose3d in float64, and ops.param_view / _tio_native / _from_tio_view on CPU tensors.
  * oracle.datapath.Partition against the per-voxel definition on the restated reflect_idx, the vote reference against a per-voxel count, the cover bound.
  * every family's pinned cases tell a deliberately wrong restatement (the mutants below) from the reference.
"""
import ctypes
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import datapath_cases as dc


# ---- launcher restatement ----------------------------------------------------------------------------------------------------------
def test_second_trip_sizes_come_from_the_restated_grid():
    assert dc.TRIP == 4096 * 256 + 1 and dc.LAYOUT_TRIP == 1024 * 256 + 1 and dc.cast_second_trip() == dc.TRIP
    assert dc.da_grid(0) == 1 and dc.da_grid(257) == 2 and dc.da_grid(10 ** 9) == 4096 and dc.da_grid(10 ** 9, cap=dc.LAYOUT_CAP) == 1024
    assert [c['n'] for c in dc.ADAM_PINNED[4:7]] == [dc.TRIP, dc.TRIP + 1, 2 * dc.TRIP + 257]
    assert dc.da_grid(2 * dc.TRIP + 257) * 256 * 2 < 2 * dc.TRIP + 257                      # ... a third trip
    assert dc.CAST_N[-1] // 4 >= dc.cast_second_trip() and dc.CAST_N[-1] % 4 == 3
    assert dc.CLAMP_SIZES[-1] == dc.TRIP + 3
    big = dc.LAYOUT_PINNED[-1]
    assert dc.da_grid(big['A'] * big['B'] * big['K3'], cap=dc.LAYOUT_CAP) * 256 < big['A'] * big['B'] * big['K3']
    for axis, values in (('t0', dc.ADAM_T0), ('p0', dc.ADAM_P0), ('lr', dc.ADAM_LR), ('betas', dc.ADAM_BETAS), ('eps', dc.ADAM_EPS), ('gs', dc.ADAM_GS), ('gmag', dc.ADAM_GMAG)):
        assert {c[axis] for c in dc.ADAM_PINNED} == set(values), axis
    assert {c['steps'] for c in dc.ADAM_PINNED} == {1, 2, 3, 4, 5}


# ---- Adam --------------------------------------------------------------------------------------------------------------------------
def _torch_adam(inp, case):
    """torch.optim.Adam in float64 on the CPU from the case's state, the gradients scaled by grad_scale beforehand."""
    p = torch.nn.Parameter(torch.from_numpy(inp['p0'].astype(np.float64)))
    opt = torch.optim.Adam([p], lr=case['lr'], betas=case['betas'], eps=case['eps'])
    if inp['t0'] > 0:
        opt.state[p] = {'step': torch.tensor(float(inp['t0'])), 'exp_avg': torch.from_numpy(inp['m0'].astype(np.float64)),
                        'exp_avg_sq': torch.from_numpy(inp['v0'].astype(np.float64))}
    for g in inp['grads']:
        p.grad = torch.from_numpy(g.astype(np.float64) * float(case['gs']))
        opt.step()
    st = opt.state[p]
    return p.detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy()


def test_adam_reference_is_torch_adam_in_float64():
    def body(case):
        inp = dc.build_adam(case)
        for got, ref, what in zip(dc.adam_ref(inp, dc.adam_hyper(case, rounded=False)), _torch_adam(inp, case), 'pmv'):
            assert dc.dist(got, ref) <= 1e-12, (what, dc.dist(got, ref))
    dc.run_cases(dc.ADAM, body, [c for c in dc.ADAM_PINNED if c['n'] < 1000])


def test_adam_float32_hyper_parameters_deviate_by_a_derivable_amount():
    """See the module docstring.  Zero moments and p0 at t = 100 000: after one step v is (1 - beta2) g^2 and bc2 is 1 to 1e-44."""
    for betas, lr in itertools.product(dc.ADAM_BETAS, dc.ADAM_LR):
        d1, d2, dup = dc.adam_hyper_dev(betas, lr)
        case = dict(n=400, t0=99999, steps=1, p0='zero', lr=lr, betas=betas, eps=1e-8, gs=1.0, gmag=1.0, sd=3)
        inp = dc.build_adam(case)
        inp['m0'][:] = 0
        inp['v0'][:] = 0
        a, b = dc.adam_ref(inp, dc.adam_hyper(case, rounded=False)), dc.adam_ref(inp, dc.adam_hyper(case, rounded=True))
        live = inp['grads'][0] != 0
        dev = [float(np.abs(x[live] / y[live] - 1).max()) for x, y in zip(b, a)]                # p0 = 0: p is the displacement
        assert dev[0] <= 1.1 * dup and dev[1] <= 1.1 * d1 + 1e-15 and dev[2] <= 1.1 * d2 + 1e-15, (betas, lr, dev, (dup, d1, d2))
        assert dev[2] >= 0.9 * d2 and dev[0] >= 0.5 * d2 - d1 - 1e-7, 'the case shows the deviation'
    d1, d2, dup = dc.adam_hyper_dev((0.9, 0.999), 1e-3)
    assert abs(d2 - 1.29e-5) < 1e-7 and abs(0.5 * d2 - 6.45e-6) < 5e-8 and dup < 6.8e-6


def test_adam_fp32_restatement_against_the_float64_reference():
    """The kernel's expression order in numpy float32 (the 'fp32 oracle' of the tolerance rule) on every case the device runs: p under the displacement bound,
    m and v by dist.  Worst: p 2.4e-7, m 1.7e-7, v 2.3e-7 -- about four fp32 roundings of the update.  8 x that is above the suite's 1e-6, so the tolerance stays
    at that ceiling and loss_cases' quarter rule has no room here: the restatement, IEEE arithmetic that does not depend on the host, is held to the tolerance itself."""
    def body(case):
        inp = dc.build_adam(case)
        hyper = dc.adam_hyper(case)
        ref, got = dc.adam_ref_path(inp, hyper), dc.adam_f32_path(inp, hyper)
        for k in range(1, case['steps'] + 1):
            e = dc.adam_p_excess(got[k - 1][0], inp['p0'], ref, k)
            dc.note('adam_f32', 'p', e)
            assert e <= dc.TOL['adam']['p'], (k, e)
        for j, what in ((1, 'm'), (2, 'v')):
            e = dc.dist(got[-1][j], ref[-1][j])
            dc.note('adam_f32', what, e)
            assert e <= dc.TOL['adam'][what], (what, e)
    dc.run_cases(dc.ADAM, body, dc.ADAM_PINNED)


def test_adam_host_state_through_the_c_abi():
    from deepatlas_amd import _native
    L = _native.lib()
    for (lr, betas, eps, gs), step in itertools.product([(1e-3, (0.9, 0.999), 1e-8, 1.0), (3e-5, (0.5, 0.9), 1e-3, 1.0 / 3.0)], [1, 2, 1000, 10 ** 6]):
        host = (ctypes.c_float * 6)()
        assert L.da_adam_host_state(lr, betas[0], betas[1], eps, step, gs, ctypes.cast(host, ctypes.c_void_p)) == 0
        got = np.array(list(host), dtype=np.float32)
        ref = dc.adam_host_state((lr, betas[0], betas[1], eps, gs), step)
        assert np.isfinite(got).all()
        ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1 and np.array_equal(got[[1, 2, 3, 5]], ref[[1, 2, 3, 5]]), (step, got, ref)
    host = (ctypes.c_float * 6)()
    assert L.da_adam_host_state(1e-3, 0.9, 0.999, 1e-8, 0, 1.0, ctypes.cast(host, ctypes.c_void_p)) == -1          # DA_ERR_BADARG
    assert L.da_adam_host_state(1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None) == -1


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
def _conv_tio(x, tio, k):
    """Convolution (cross-correlation, padding k // 2) from a tap-major [k^3][Cin][Cout] weight, tap by tap."""
    N, _, D, H, W = x.shape
    xp = F.pad(x, (k // 2,) * 6)
    out = torch.zeros((N, tio.shape[2], D, H, W), dtype=x.dtype)
    for t, (kz, ky, kx) in enumerate(itertools.product(range(k), repeat=3)):
        out += torch.einsum('ncdhw,co->nodhw', xp[:, :, kz:kz + D, ky:ky + H, kx:kx + W], tio[t])
    return out


def _deconv2_tio(x, tio):
    """2x2x2 stride-2 transposed convolution from a tap-major [8][Cin][Cout] weight."""
    N, _, D, H, W = x.shape
    out = torch.zeros((N, tio.shape[2], 2 * D, 2 * H, 2 * W), dtype=x.dtype)
    for t, (kz, ky, kx) in enumerate(itertools.product(range(2), repeat=3)):
        out[:, :, kz::2, ky::2, kx::2] = torch.einsum('ncdhw,co->nodhw', x, tio[t])
    return out


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def test_layout_references_are_the_convolutions_weights():
    g = torch.Generator().manual_seed(5)
    x = torch.rand((2, 3, 4, 5, 6), generator=g, dtype=torch.float64)
    w = torch.rand((5, 3, 3, 3, 3), generator=g, dtype=torch.float64)                       # Conv3d [Cout][Cin][k^3]
    tio = _t64(dc.layout_ref('da_w_oik_to_tio', w.numpy().reshape(5, 3, 27)))
    assert torch.allclose(F.conv3d(x, w, padding=1), _conv_tio(x, tio, 3), rtol=0, atol=1e-12)
    wt = torch.rand((3, 5, 3, 3, 3), generator=g, dtype=torch.float64)                      # ConvTranspose3d [Cin][Cout][k^3]
    tio = _t64(dc.layout_ref('da_w_iok_flip_to_tio', wt.numpy().reshape(3, 5, 27)))
    assert torch.allclose(F.conv_transpose3d(x, wt, stride=1, padding=1), _conv_tio(x, tio, 3), rtol=0, atol=1e-12)
    w2 = torch.rand((3, 4, 2, 2, 2), generator=g, dtype=torch.float64)
    tio = _t64(dc.layout_ref('da_w_iok_to_tio', w2.numpy().reshape(3, 4, 8)))
    assert torch.allclose(F.conv_transpose3d(x, w2, stride=2), _deconv2_tio(x, tio), rtol=0, atol=1e-12)
    # the way back inverts the way there, for the three kinds
    for kind in ('oik', 'iok', 'iok_flip'):
        src = dc.distinct((4, 7, 27), 3)
        assert np.array_equal(dc.layout_ref('da_w_tio_to_' + kind, dc.layout_ref('da_w_%s_to_tio' % kind, src)), src)
        before = dc.distinct((4, 7, 27), 4)
        assert np.array_equal(dc.layout_ref('da_w_tio_to_%s_acc' % kind, dc.layout_ref('da_w_%s_to_tio' % kind, src), before), before + src)


def test_ops_views_agree_with_the_layout_references():
    from deepatlas_amd import ops
    for kind, shape in (('oik', (5, 3, 3, 3, 3)), ('iok', (3, 4, 2, 2, 2)), ('oik', (1, 6, 1, 1, 1)), ('iok', (7, 1, 2, 2, 2))):
        K3 = shape[2] * shape[3] * shape[4]
        w = dc.distinct(shape, 9)
        tio = dc.layout_ref('da_w_%s_to_tio' % kind, w.reshape(shape[0], shape[1], K3))
        p = torch.empty(shape)
        p._da_kind = kind
        buf = torch.cat([torch.zeros(3), torch.from_numpy(tio.copy()).reshape(-1), torch.zeros(2)])
        view = ops.param_view(buf, 3, p)
        assert tuple(view.shape) == shape and np.array_equal(view.numpy(), w)
        native = ops._tio_native(view, kind)
        assert native is not None and native.data_ptr() == buf.data_ptr() + 12 and np.array_equal(native.numpy(), tio)
        assert np.array_equal(ops._from_tio_view(torch.from_numpy(tio.copy()), kind, shape).numpy(), w)
        assert ops._tio_native(torch.from_numpy(w.copy()), kind) is None or min(shape[0], shape[1]) == 1 and K3 == 1      # contiguous reference layout: no view
        prev, ops.NATIVE_TIO = ops.NATIVE_TIO, False
        try:
            assert ops.param_view(buf, 3, p).is_contiguous()
        finally:
            ops.NATIVE_TIO = prev


def test_layout_cases_draw_unequal_channel_counts():
    seen = []
    dc.run_cases(dc.LAYOUT_CASES, lambda c: seen.append(c['A'] != c['B']), dc.LAYOUT_PINNED)
    drawn = seen[len(dc.LAYOUT_PINNED):]
    assert len(drawn) == 60 and sum(drawn) >= 30
    a = dc.distinct((100, 101, 27), 0)
    assert np.unique(a).size == a.size


# ---- data path ---------------------------------------------------------------------------------------------------------------------
def test_reflect_idx_is_numpys_reflect_padding():
    for n in range(1, 8):
        for lo, hi in itertools.product(range(20), repeat=2):
            ref = np.pad(np.arange(n), (lo, hi), mode='reflect')
            assert [dc.reflect_idx(i - lo, n) for i in range(n + lo + hi)] == ref.tolist(), (n, lo, hi)


def test_partition_reference_is_the_per_voxel_definition():
    def body(case):
        vol = dc.volume_values(case)
        tiles = dc.partition_ref(case, vol)
        assert tiles.dtype == vol.dtype and np.array_equal(tiles, dc.partition_brute(case, vol))
        assert np.array_equal(dc.assemble_ref(case, tiles), vol)                              # the cores of the tiles are the volume
    dc.run_cases(dc.GEOM, body, dc.PARTITION_PINNED + dc.ASSEMBLE_PINNED)


def test_vote_reference_is_the_per_voxel_count():
    seen = dict(ties=0, gapped=0, declined=0, drawn=0, i=0)

    def body(case):
        seen['i'] += 1
        bound = dc.cover_bound(case)
        assert dc.cover_max(case) <= bound                                                  # the launcher's bound is an upper bound
        if seen['i'] > len(dc.VOTE_PINNED):                                                   # (run_cases runs the pinned cases first)
            seen['drawn'] += 1
            seen['declined'] += bound > 64
        if int(np.prod(case['vol'])) > 5000:                                                  # (the second-trip volume: the device test's reference only)
            return
        tiles = dc.noisy_tiles(case)
        ref = dc.vote_ref(case, tiles)
        brute, ties = dc.vote_brute(case, tiles)
        assert np.array_equal(ref, brute)
        seen['ties'] += ties
        seen['gapped'] += not np.array_equal(np.unique(tiles), np.arange(np.unique(tiles).size))
        clean = dc.partition_brute(case, dc.label_volume(case))                              # consistent tiles vote for the volume itself
        assert np.array_equal(dc.vote_ref(case, clean), dc.label_volume(case))
    dc.run_cases(dc.VOTE, body, dc.VOTE_PINNED)
    assert seen['drawn'] == 60 and seen['declined'] <= dc.VOTE_DECLINE_MAX, seen
    assert seen['ties'] > 100 and seen['gapped'] >= 10, seen
    full = dc.GEOM_SMALL[6]
    assert dc.cover_bound(full) == 64 == dc.cover_max(full)                                   # attained
    assert dc.cover_bound(dc.GEOM_DECLINE) == 125


def test_clamp_and_cast_and_synth_cases_hold_what_they_promise():
    for code, dtype in enumerate(dc.CLAMP_DTYPES):
        a = dc.clamp_values(dtype, 257, code)
        ref = dc.clamp_ref(a)
        assert ref.dtype == np.float32 and (a > 1).any() and (a == 1).any() and (a == 0).any() and (np.dtype(dtype).kind == 'u' or (a < 0).any())
        ok = ~np.isnan(ref)
        assert ref[ok].min() >= 0 and ref[ok].max() <= 1
    d = dc.clamp_values(np.float64, 257, 0)
    r = dc.clamp_ref(d)
    assert np.isnan(r[np.isnan(d)]).all() and np.signbit(r[(d == 0) & np.signbit(d)]).all() and not np.signbit(r[d == -1e-300]).any()
    assert (r[d == 1 + 1e-12] == 1).all() and (r[d == 1 - 1e-12] == 1).all() and (r[d == 5e-324] == 0).all() and (d == 5e-324).any()
    for dtype, bad in ((np.int64, [-2 ** 32 + 1, 2 ** 32]), (np.uint32, [2 ** 31 + 5])):
        a = dc.clamp_values(dtype, 40, 0)
        assert all(v in a.tolist() for v in bad)
    x = dc.cast_values(dict(n=1023, sd=0))
    fin = np.isfinite(x) & (x != 0)
    assert (np.abs(x[fin]) >= 2.0 ** -126).all() and np.isnan(x).any() and np.isinf(x).any()
    e = np.log2(np.abs(x[fin]))
    assert e.min() < -100 and e.max() > 100
    b = dc.bf16_bits_ref(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4028234663852886e38], dtype=np.float32))
    assert b.tolist() == [0x3F80, 0x3F82, 0x7F80]                                           # ties to even in both directions; the largest fp32 rounds to +inf
    assert any(dc.synth_crosses(c) and c['mode'] == m for c in dc.SYNTH_PINNED for m in (0,)) and any(dc.synth_crosses(c) and c['mode'] == 1 for c in dc.SYNTH_PINNED)
    assert {c['C'] for c in dc.SYNTH_PINNED} == {1, 2, 32, 256} and {c['which'] for c in dc.SYNTH_PINNED} == {'both', 'img', 'lab'}
    assert any(min(c['vol']) < 8 for c in dc.SYNTH_PINNED) and any(c['N'] * int(np.prod(c['vol'])) >= dc.TRIP for c in dc.SYNTH_PINNED)


# ---- the pinned cases discriminate: one deliberately wrong restatement per family ----------------------------------------------------
def _symmetric_idx(i, n):
    """numpy.pad(mode='symmetric'): the edge voxel is repeated."""
    m = i % (2 * n)
    return m if m < n else 2 * n - 1 - m


def _adam_mutant(inp, hyper, swap=False, lag=False):
    lr, b1, b2, eps, gs = hyper
    if swap:
        b1, b2 = b2, b1
    p, m, v = (inp[k].astype(np.float64) for k in ('p0', 'm0', 'v0'))
    for k, g in enumerate(inp['grads']):
        t = inp['t0'] + k + 1 - (1 if lag else 0)
        gi = g.astype(np.float64) * gs
        m = b1 * m + (1.0 - b1) * gi
        v = b2 * v + (1.0 - b2) * gi * gi
        p = p - (lr / (1.0 - b1 ** t)) * (m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps))
    return p, m, v


def _caught(flags):
    flags = list(flags)
    assert any(flags), 'no pinned case tells the mutant from the reference'
    return sum(flags)


def test_pinned_cases_catch_the_mutants():
    small = [c for c in dc.PARTITION_PINNED if int(np.prod(c['vol'])) < 5000]
    # 'symmetric' instead of 'reflect' padding
    _caught(not np.array_equal(dc.partition_brute(c, dc.volume_values(c), _symmetric_idx), dc.partition_ref(c, dc.volume_values(c))) for c in small)
    # vote ties to the largest label
    votes = [c for c in dc.VOTE_PINNED if int(np.prod(c['vol'])) < 5000]
    _caught(not np.array_equal(dc.vote_ref(c, dc.noisy_tiles(c), ties='largest'), dc.vote_ref(c, dc.noisy_tiles(c))) for c in votes)
    # taps not flipped; channel axes swapped with A != B
    def src_of(name, c):
        return dc.distinct(dc.LAYOUT[name][0](c['A'], c['B'], c['K3']), c['sd'])
    _caught(not np.array_equal(dc.layout_ref('da_w_iok_to_tio', src_of('da_w_iok_to_tio', c)), dc.layout_ref('da_w_iok_flip_to_tio', src_of('da_w_iok_to_tio', c)))
            for c in dc.LAYOUT_PINNED)
    _caught(not np.array_equal(dc.layout_ref('da_w_tio_to_iok', src_of('da_w_tio_to_iok_flip', c)), dc.layout_ref('da_w_tio_to_iok_flip', src_of('da_w_tio_to_iok_flip', c)))
            for c in dc.LAYOUT_PINNED)
    def swapped(name, c):                                  # the same memory read with the roles of the two channel axes exchanged
        other = name.replace('oik', 'iok')
        return dc.layout_ref(other, src_of(name, c).reshape(dc.LAYOUT[other][0](c['A'], c['B'], c['K3'])))
    for name in ('da_w_oik_to_tio', 'da_w_tio_to_oik'):
        n = _caught(c['A'] != c['B'] and swapped(name, c).tobytes() != dc.layout_ref(name, src_of(name, c)).tobytes() for c in dc.LAYOUT_PINNED)
        assert n >= 3                                      # (a channel count of 1 on either side makes the two readings coincide)
    # the clamp applied after the cast to float32; the narrowing to int32 ahead of the clamp (the defect SitkToTensor had)
    def clamp_late(a):
        with np.errstate(invalid='ignore', over='ignore'):
            return dc.clamp_ref(a.astype(np.float32))
    _caught(not dc.same_bits(clamp_late(dc.clamp_values(dc.CLAMP_DTYPES[c['code']], c['n'], c['sd'])), dc.clamp_ref(dc.clamp_values(dc.CLAMP_DTYPES[c['code']], c['n'], c['sd'])))
            for c in dc.CLAMP_PINNED if c['n'] < 1000)
    for dtype in (np.int64, np.uint32):
        cases = [c for c in dc.SITK_PINNED if c['dtype'] is dtype]
        assert cases
        for c in cases:
            a = dc.clamp_values(dtype, int(np.prod(c['vol'])), c['sd'])
            narrowed = torch.from_numpy(a).to(torch.int32).numpy()                            # wraps
            assert not dc.same_bits(dc.clamp_ref(narrowed), dc.clamp_ref(a)), dtype
    # Adam: beta1 and beta2 swapped; the bias correction of step t - 1
    tol = dc.CEIL['adam']
    for kw, cases in ((dict(swap=True), dc.ADAM_PINNED), (dict(lag=True), [c for c in dc.ADAM_PINNED if c['t0'] >= 1])):
        flags = []
        for c in [c for c in cases if c['n'] < 1000]:
            inp, hyper = dc.build_adam(c), dc.adam_hyper(c)
            ref = dc.adam_ref_path(inp, hyper)
            p, m, v = _adam_mutant(inp, hyper, **kw)
            flags.append(dc.adam_p_excess(p, inp['p0'], ref, c['steps']) > tol['p'] or dc.dist(m, ref[-1][1]) > tol['m'] or dc.dist(v, ref[-1][2]) > tol['v'])
        assert _caught(flags) >= 2
    # a cast that truncates instead of rounding to nearest even
    _caught(not dc.same_bf16((dc.cast_values(c).view(np.uint32) >> 16).astype(np.uint16), dc.bf16_bits_ref(dc.cast_values(c))) for c in dc.CAST_PINNED if c['n'] < 5000)
