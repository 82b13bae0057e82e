"""The kept-pack hand-over at the C ABI: da_conv3d_k3_prepack / _prepack_many fill caller-owned buffers, da_conv3d_k3_use_prepacked hands them to
the next matrix-core call of the thread on the same weights (include/deepatlas_hip.h).

Every assertion is torch.equal against the same entry called with no hand-over: the same kernel runs on the same operands, so the results are equal bit for
bit.  Split matrix mode, N = 2, 5 x 9 x 17 voxels unless stated: two 4 x 8 x 16 tiles per axis with a ragged last tile each (16 tiles: the tile table, the
persistent walk and the edge masks all matter).

Rule of this file: a kernel is only ever handed a buffer that da_conv3d_k3_prepack filled for that exact shape and direction (anything else carries a
garbage tile table).  The cases are built so that a wrong hand-over shows as a wrong VALUE: the buffers that must not be read hold a valid pack of other
weights of the same shape."""
import ctypes

import pytest
import torch

from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

DIMS = (2, 5, 9, 17)


def _nat():
    from deepatlas_amd import _native as nat
    return nat


class _split(object):
    def __init__(self, mode='fp32_split'):
        self.mode = mode

    def __enter__(self):
        from deepatlas_amd import ops
        self.prev = ops.set_matrix_precision(self.mode)

    def __exit__(self, *exc):
        from deepatlas_amd import ops
        try:
            _nat().lib().da_conv3d_k3_use_prepacked(None, None, 0, None, 0)       # nothing stays pending for the next test
        finally:
            ops.set_matrix_precision(self.prev)


def _rand(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev())


def _weights(seed, cin, cout):
    return _rand(seed, 27, cin, cout) * (27 * cin) ** -0.5


def _ws(dims, cin, cout):
    nat = _nat()
    return nat.workspace.get(nat.lib().da_conv3d_k3_ws_bytes(*dims, cin, cout, 1), dev())


def _pack_buf(dims, cin, cout):
    n = _nat().lib().da_conv3d_k3_pack_bytes(*dims, cin, cout)
    assert n > 0
    return torch.zeros(n, dtype=torch.uint8, device=dev())


def _prepack_rc(w, c1, c2, cout, dgrad, dims, b0, b1):
    nat = _nat()
    used = ctypes.c_int(-1)
    rc = nat.lib().da_conv3d_k3_prepack(nat.ptr(w), c1, c2, cout, dgrad, *dims, nat.ptr(b0), b0.numel() if b0 is not None else 0,
                                        nat.ptr(b1), b1.numel() if b1 is not None else 0, ctypes.byref(used), nat.stream())
    torch.cuda.synchronize()
    return rc, used.value


def _prepack(w, c1, c2, cout, dgrad, dims, b0, b1=None):
    rc, used = _prepack_rc(w, c1, c2, cout, dgrad, dims, b0, b1)
    assert rc == 0, rc
    return used


def _use(w, b0, b1=None):
    nat = _nat()
    nat.lib().da_conv3d_k3_use_prepacked(nat.ptr(w), nat.ptr(b0), b0.numel(), nat.ptr(b1), b1.numel() if b1 is not None else 0)


def _fwd(x, w, bias, cout, dims=DIMS, slope=0.01):
    nat = _nat()
    out = torch.full(dims + (cout,), float('nan'), device=dev())
    wp, wn = _ws(dims, x.shape[-1], cout)
    nat.call('da_conv3d_k3_fwd', nat.ptr(x), x.shape[-1], None, 0, nat.ptr(w), nat.ptr(bias), nat.ptr(out), *dims, cout, 1, slope, wp, wn, nat.stream())
    torch.cuda.synchronize()
    return out


def _fwd_bnstats(x, w, bias, cout, dims=DIMS):
    nat = _nat()
    out = torch.full(dims + (cout,), float('nan'), device=dev())
    part = torch.full((512, 2, cout), float('nan'), dtype=torch.float64, device=dev())
    nparts = ctypes.c_int(-1)
    wp, wn = _ws(dims, x.shape[-1], cout)
    nat.call('da_conv3d_k3_fwd_bnstats', nat.ptr(x), x.shape[-1], None, 0, nat.ptr(w), nat.ptr(bias), nat.ptr(out), *dims, cout, 1,
             nat.ptr(part), 512, ctypes.byref(nparts), wp, wn, nat.stream())
    torch.cuda.synchronize()
    return out, nparts.value, part[:max(nparts.value, 0)].clone()


def _fwd_pro(x, scale, shift, w, bias, cout, dims=DIMS):
    nat = _nat()
    out = torch.full(dims + (cout,), float('nan'), device=dev())
    wp, wn = _ws(dims, x.shape[-1], cout)
    nat.call('da_conv3d_k3_fwd_pro', nat.ptr(x), x.shape[-1], nat.ptr(scale), nat.ptr(shift), 0.01, None, 0, None, None, -1.0,
             nat.ptr(w), nat.ptr(bias), nat.ptr(out), *dims, cout, 0.01, None, 0, None, wp, wn, nat.stream())
    torch.cuda.synchronize()
    return out


def _dgrad(dy, w, c1, c2, dims=DIMS):
    nat = _nat()
    dx1 = torch.full(dims + (c1,), float('nan'), device=dev())
    dx2 = torch.full(dims + (c2,), float('nan'), device=dev()) if c2 else None
    wp, wn = _ws(dims, c1 + c2, dy.shape[-1])
    nat.call('da_conv3d_k3_dgrad', nat.ptr(dy), nat.ptr(w), nat.ptr(dx1), c1, nat.ptr(dx2), c2, *dims, dy.shape[-1], 1, wp, wn, nat.stream())
    torch.cuda.synchronize()
    return dx1, dx2


def _dgrad_bst(dy, w, c1, c2, y, stats4, dims=DIMS):
    nat = _nat()
    dx1 = torch.full(dims + (c1,), float('nan'), device=dev())
    dx2 = torch.full(dims + (c2,), float('nan'), device=dev()) if c2 else None
    bst = torch.full((512, 2, c1), float('nan'), dtype=torch.float64, device=dev())
    nb = ctypes.c_int(-1)
    wp, wn = _ws(dims, c1 + c2, dy.shape[-1])
    nat.call('da_conv3d_k3_dgrad_bst', nat.ptr(dy), nat.ptr(w), nat.ptr(dx1), c1, nat.ptr(dx2), c2, *dims, dy.shape[-1], nat.ptr(y), nat.ptr(stats4), 0.01,
             nat.ptr(bst), 512, ctypes.byref(nb), wp, wn, nat.stream())
    torch.cuda.synchronize()
    return dx1, dx2, nb.value, bst[:max(nb.value, 0)].clone()


def _same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, torch.Tensor):
            assert a.shape == b.shape and bool(torch.isfinite(b).all()) and torch.equal(a, b), i
        else:
            assert a == b, (i, a, b)


def test_forward_entries_read_the_kept_pack():
    """16 -> 16: prepack fills one region; da_conv3d_k3_fwd, _fwd_bnstats (output, nparts, partials) and _fwd_pro after use_prepacked equal the plain calls."""
    with _split():
        x, w, bias = _rand(1, *DIMS, 16), _weights(2, 16, 16), _rand(3, 16)
        scale, shift = _rand(4, 16).abs() + 0.5, _rand(5, 16)
        buf = _pack_buf(DIMS, 16, 16)
        assert _prepack(w, 16, 0, 16, 0, DIMS, buf) == 1
        assert int(buf.count_nonzero()) > 0
        plain = _fwd(x, w, bias, 16)
        assert bool(torch.isfinite(plain).all())
        _use(w, buf)
        assert torch.equal(_fwd(x, w, bias, 16), plain)
        plain_s = _fwd_bnstats(x, w, bias, 16)
        assert plain_s[1] > 0
        _use(w, buf)
        _same(_fwd_bnstats(x, w, bias, 16), plain_s)
        plain_p = _fwd_pro(x, scale, shift, w, bias, 16)
        assert not torch.equal(plain_p, plain)
        _use(w, buf)
        assert torch.equal(_fwd_pro(x, scale, shift, w, bias, 16), plain_p)


def test_hand_over_serves_one_call_only():
    """After a consumed hand-over the buffer is refilled with the pack of other weights of the same shape: a second call on the first weights, with no new
    use_prepacked, packs for itself."""
    with _split():
        x, wa, wb, bias = _rand(11, *DIMS, 16), _weights(12, 16, 16), _weights(13, 16, 16), _rand(14, 16)
        buf = _pack_buf(DIMS, 16, 16)
        plain = _fwd(x, wa, bias, 16)
        assert not torch.equal(plain, _fwd(x, wb, bias, 16))
        assert _prepack(wa, 16, 0, 16, 0, DIMS, buf) == 1
        _use(wa, buf)
        assert torch.equal(_fwd(x, wa, bias, 16), plain)
        assert _prepack(wb, 16, 0, 16, 0, DIMS, buf) == 1
        assert torch.equal(_fwd(x, wa, bias, 16), plain)


def test_call_on_other_weights_drops_the_hand_over():
    """use_prepacked(wA) followed by a forward on wB: wB's result, and the hand-over is gone -- a later forward on wA (the buffer then holds wC's pack) packs for itself."""
    with _split():
        x, bias = _rand(21, *DIMS, 16), _rand(22, 16)
        wa, wb, wc = _weights(23, 16, 16), _weights(24, 16, 16), _weights(25, 16, 16)
        buf = _pack_buf(DIMS, 16, 16)
        plain_a, plain_b = _fwd(x, wa, bias, 16), _fwd(x, wb, bias, 16)
        assert not torch.equal(plain_a, plain_b) and not torch.equal(plain_a, _fwd(x, wc, bias, 16))
        assert _prepack(wa, 16, 0, 16, 0, DIMS, buf) == 1
        _use(wa, buf)
        assert torch.equal(_fwd(x, wb, bias, 16), plain_b)
        assert _prepack(wc, 16, 0, 16, 0, DIMS, buf) == 1
        assert torch.equal(_fwd(x, wa, bias, 16), plain_a)


def test_two_regions_of_the_concat_data_gradient():
    """(32 + 16) -> 16, data gradient: two launches, two regions.  With the second region withheld on the use side the second launch packs for itself;
    withheld on the fill side, prepack returns DA_ERR_WS_SMALL and reports nothing kept."""
    with _split():
        dy, w = _rand(31, *DIMS, 16), _weights(32, 48, 16)
        b0, b1 = _pack_buf(DIMS, 48, 16), _pack_buf(DIMS, 48, 16)
        assert _prepack(w, 32, 16, 16, 1, DIMS, b0, b1) == 2
        assert int(b0.count_nonzero()) > 0 and int(b1.count_nonzero()) > 0
        plain = _dgrad(dy, w, 32, 16)
        _use(w, b0, b1)
        _same(_dgrad(dy, w, 32, 16), plain)
        _use(w, b0, None)
        _same(_dgrad(dy, w, 32, 16), plain)
        assert _prepack_rc(w, 32, 16, 16, 1, DIMS, _pack_buf(DIMS, 48, 16), None) == (-2, 0)


@pytest.mark.parametrize('c1,c2', [(16, 0), (32, 16)])
def test_dgrad_with_the_batchnorm_backward_epilogue(c1, c2):
    """da_conv3d_k3_dgrad_bst, single-input (16 <- 16) and concat ((32 + 16) <- 16) form, with and without a hand-over: dx1, dx2, bst_n and the partials."""
    with _split():
        dy, w = _rand(41, *DIMS, 16), _weights(42, c1 + c2, 16)
        y = _rand(43, *DIMS, c1)
        mean, var = y.reshape(-1, c1).mean(0), y.reshape(-1, c1).var(0, unbiased=False)
        rstd = (var + 1e-5).rsqrt()
        gamma, beta = _rand(44, c1).abs() + 0.5, _rand(45, c1)
        stats4 = torch.stack((mean, rstd, gamma * rstd, beta - mean * gamma * rstd)).contiguous()
        bufs = [_pack_buf(DIMS, c1 + c2, 16) for _ in range(2 if c2 else 1)]
        assert _prepack(w, c1, c2, 16, 1, DIMS, *bufs) == len(bufs)
        plain = _dgrad_bst(dy, w, c1, c2, y, stats4)
        assert plain[2] > 0
        _use(w, *bufs)
        _same(_dgrad_bst(dy, w, c1, c2, y, stats4), plain)


def _many(jobs):
    """jobs: (w, C1, C2, Cout, dgrad, dims).  One da_conv3d_k3_prepack_many call into zeroed buffers against one da_conv3d_k3_prepack call per job into zeroed twins."""
    nat = _nat()
    n = len(jobs)
    two = [(j[2] > 0 and j[4] == 1) for j in jobs]
    mk = lambda: [[_pack_buf(j[5], j[1] + j[2], j[3]) for _ in range(2 if t else 1)] for j, t in zip(jobs, two)]
    many, single = mk(), mk()
    IA, PA, SA = ctypes.c_int * n, ctypes.c_void_p * n, ctypes.c_size_t * n
    used = IA(*([-1] * n))
    nat.call('da_conv3d_k3_prepack_many', n, PA(*[j[0].data_ptr() for j in jobs]), IA(*[j[1] for j in jobs]), IA(*[j[2] for j in jobs]),
             IA(*[j[3] for j in jobs]), IA(*[j[4] for j in jobs]), IA(*[j[5][0] for j in jobs]), IA(*[j[5][1] for j in jobs]), IA(*[j[5][2] for j in jobs]),
             IA(*[j[5][3] for j in jobs]), PA(*[b[0].data_ptr() for b in many]), SA(*[b[0].numel() for b in many]),
             PA(*[(b[1].data_ptr() if len(b) > 1 else None) for b in many]), SA(*[(b[1].numel() if len(b) > 1 else 0) for b in many]), used, nat.stream())
    torch.cuda.synchronize()
    for i, (j, bs, bm) in enumerate(zip(jobs, single, many)):
        assert _prepack(j[0], j[1], j[2], j[3], j[4], j[5], *bs) == used[i] == len(bs), (i, used[i])
        for a, b in zip(bs, bm):
            assert int(a.count_nonzero()) > 0 and torch.equal(a, b), i


def test_prepack_many_fills_what_prepack_fills():
    """Forward 16 -> 16, data gradient (32 + 16) -> 16, forward 8 -> 32 on one 4 x 8 x 16 tile; then 49 jobs (more than the 48 regions of one launch) with the
    two-region data gradient across the boundary between the launches."""
    one = (1, 4, 8, 16)
    with _split():
        wcat = _weights(52, 48, 16)
        _many([(_weights(51, 16, 16), 16, 0, 16, 0, DIMS), (wcat, 32, 16, 16, 1, DIMS), (_weights(53, 8, 32), 8, 0, 32, 0, one)])
        w8 = [_weights(60 + i, 8, 8) for i in range(48)]
        _many([(w, 8, 0, 8, 0, one) for w in w8[:47]] + [(wcat, 32, 16, 16, 1, DIMS)] + [(w8[47], 8, 0, 8, 0, one)])


def test_nothing_is_kept_outside_the_split_mode():
    """'fp32' matrix mode: prepack reports used == 0, and a pending hand-over (a valid pack of this shape, filled in split mode) changes nothing."""
    x, w, bias = _rand(71, *DIMS, 16), _weights(72, 16, 16), _rand(73, 16)
    buf = _pack_buf(DIMS, 16, 16)
    with _split():
        assert _prepack(w, 16, 0, 16, 0, DIMS, buf) == 1
    with _split('fp32'):
        assert _prepack(w, 16, 0, 16, 0, DIMS, _pack_buf(DIMS, 16, 16)) == 0
        plain = _fwd(x, w, bias, 16)
        _use(w, buf)
        assert torch.equal(_fwd(x, w, bias, 16), plain)
