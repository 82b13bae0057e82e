"""Shared by tests/test_gpu_datapath_shapes.py (the kernels of optim.hip and datapath.hip on the device) and tests/test_datapath_reference.py (the
references and the case builders, no GPU): pinned cases, hypothesis strategies, builders, the references, and the launcher decisions restated.
TEST INFRASTRUCTURE ONLY: nothing here runs on the GPU.

Families: `adam` (da_adam_step, da_adam_step_dev, da_adam_host_state), `layout` (the nine da_w_* entry points), `clamp` (da_clamp01_to_f32), `crop`
(da_crop3d), `partition` / `assemble` / `vote` (da_partition_tiles, da_assemble_tiles), `cast` (da_cast_f32_to_bf16, da_cast_bf16_to_f32) and `synth`
(da_synth_volume).  Everything but Adam is a copy, a comparison or integer arithmetic and is compared bit for bit; Adam is compared with a float64
reference under the bound stated at adam_p_excess.

Conventions are those of tests/loss_cases.py: every family runs `run_cases` (seed 160950, the pinned cases first, then 60 derandomised cases, at least
90 % compared to the end); distances by `dist` / `note` into `WORST`.  With DA_DATAPATH_SHAPES_REPORT=<path> set, run_cases writes the worst distance
per family and quantity to that JSON file.  Device output buffers are prefilled (NaN, or 0xFF bytes for integer types) and carry GUARD elements behind
their end that must keep the prefill.

Plain module, no fixtures, no pytest settings."""
import json
import os

import numpy as np
import torch
from hypothesis import strategies as st

import loss_cases as lc
from loss_cases import WORST, _cyc, dist, note                 # noqa: F401  (re-exported for the two test files)
from oracle import datapath as dp

FAMILIES = ('adam', 'adam_f32', 'flatadam')        # the families with a distance to record (adam_f32: the CPU companion's restatement)
GUARD = 8                  # elements behind every device output that must keep their prefill


def run_cases(strategy, body, pinned=()):
    ran = lc.run_cases(strategy, body, pinned)
    write_report()
    return ran


def write_report():
    path = os.environ.get('DA_DATAPATH_SHAPES_REPORT')
    if path:
        with open(path, 'w') as f:
            json.dump({k: v for k, v in lc.WORST.items() if k.split('/')[0] in FAMILIES}, f, indent=1, sort_keys=True)


# ---- the launcher decisions, restated ---------------------------------------------------------------------------------------------
BLOCK = 256
GRID_CAP = 256 * 16        # common.h da_grid's default cap: optim.hip's Adam kernels and every kernel of datapath.hip
LAYOUT_CAP = 1024          # optim.hip DA_W_LAUNCH


def da_grid(work_items, block=BLOCK, cap=GRID_CAP):
    """common.h da_grid: ceil(work / block) blocks, at least 1, at most `cap`."""
    return max(1, min(cap, -(-int(work_items) // block)))


def second_trip(cap=GRID_CAP, block=BLOCK):
    """The smallest number of work items at which a thread of the grid-stride loop `for (i = tid; i < n; i += grid * block)` runs a second trip."""
    n = cap * block + 1
    assert da_grid(n, block, cap) * block < n and da_grid(n - 1, block, cap) * block >= n - 1
    return n


def cast_quads_grid(n):
    """datapath.hip da_cast_*: the grid is sized by the quad count, da_grid(n / 4 + 1, 256); the body walks n / 4 quads, the tail the n % 4 elements."""
    return da_grid(n // 4 + 1)


def cast_second_trip():
    """Smallest QUAD count at which the vector body takes a second trip (the + 1 of the grid's argument does not move it: the cap is reached first)."""
    q = second_trip()
    assert cast_quads_grid(4 * q) * BLOCK < q and cast_quads_grid(4 * (q - 1)) * BLOCK >= q - 1
    return q


TRIP = second_trip()                       # 1 048 577
LAYOUT_TRIP = second_trip(LAYOUT_CAP)      # 262 145


# ---- Adam -------------------------------------------------------------------------------------------------------------------------
# Reference: float64, with the hyper-parameters as the float32 values the C ABI receives and the bias corrections in double from those, as da_adam_step
# computes them.  (da_adam_step then rounds lr / bc1 and 1 / sqrt(bc2) to float32 for the kernel: that rounding belongs to the device and is inside TOL.)
ADAM_N = [1, 255, 256, 257]
ADAM_BIG_N = [TRIP, TRIP + 1, 2 * TRIP + 257]
ADAM_T0 = [0, 1, 999, 99999]               # first step t0 + 1 = 1, 2, 1000, 100 000
ADAM_LR = [1e-3, 3e-5]
ADAM_BETAS = [(0.9, 0.999), (0.5, 0.9)]
ADAM_EPS = [1e-8, 1e-3]
ADAM_GS = [1.0, 0.125, 1.0 / 3.0]
# |g| of an element is gmag 2^-u, u uniform in [0, 4], or exactly 0 (one in seven); with grad_scale >= 1 / 8 the product stays in [1.5e-12, 1e12]: g g
# neither underflows to a subnormal nor overflows
ADAM_GMAG = [2e-10, 1e-6, 1e-3, 1.0, 1e3, 1e6, 1e12]
ADAM_P0 = ['zero', 'lr', 'one']            # |p0| = 0, about lr (both make the displacement term of the bound the sharp one), about 1
ADAM = st.fixed_dictionaries(dict(
    n=st.one_of(st.sampled_from(ADAM_N), st.integers(1, 700)), t0=st.sampled_from(ADAM_T0), steps=st.integers(1, 5), p0=st.sampled_from(ADAM_P0),
    lr=st.sampled_from(ADAM_LR), betas=st.sampled_from(ADAM_BETAS), eps=st.sampled_from(ADAM_EPS), gs=st.sampled_from(ADAM_GS),
    gmag=st.sampled_from(ADAM_GMAG), sd=st.integers(0, 999)))


def _adam_case(i, n, steps=None):
    return dict(n=n, t0=_cyc(ADAM_T0, i), steps=steps or 1 + i % 5, p0=_cyc(ADAM_P0, i), lr=_cyc(ADAM_LR, i), betas=_cyc(ADAM_BETAS, i // 2),
                eps=_cyc(ADAM_EPS, i // 3), gs=_cyc(ADAM_GS, i), gmag=_cyc(ADAM_GMAG, i), sd=i)


# the four block-edge sizes, the three sizes beyond the second trip (built from second_trip(), 2 - 3 steps), and ten more small ones so that every value
# of every axis occurs and p0 = 0 / lr meets each gradient magnitude
ADAM_PINNED = ([_adam_case(i, n) for i, n in enumerate(ADAM_N)] + [_adam_case(4 + i, n, steps=2 + i % 2) for i, n in enumerate(ADAM_BIG_N)] +
               [_adam_case(7 + i, _cyc([67, 300, 513], i), steps=5) for i in range(10)])


def f32(x):
    return float(np.float32(x))


def adam_hyper(case, rounded=True):
    """(lr, beta1, beta2, eps, grad_scale) as float64 numbers: the float32 values the C ABI receives, or (rounded=False) Python's own."""
    h = (case['lr'], case['betas'][0], case['betas'][1], case['eps'], case['gs'])
    return tuple(f32(v) for v in h) if rounded else tuple(float(v) for v in h)


def build_adam(case):
    """fp32 arrays: p0, one gradient per step, and the moments the run starts from (zero at t0 = 0, of the gradients' magnitude otherwise)."""
    rng = np.random.default_rng(1000 + case['sd'])
    n, g0 = case['n'], case['gmag']
    scale = {'zero': 0.0, 'lr': case['lr'], 'one': 1.0}[case['p0']]
    p0 = (rng.uniform(-1, 1, n) * scale).astype(np.float32)
    grads = []
    for _ in range(case['steps']):
        g = g0 * np.exp2(-rng.uniform(0, 4, n)) * rng.choice([-1.0, 1.0], n)
        g[rng.integers(0, 7, n) == 0] = 0.0
        grads.append(g.astype(np.float32))
    if case['t0'] == 0:
        m0, v0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        gs = g0 * case['gs']
        m0 = (0.5 * gs * rng.uniform(-1, 1, n)).astype(np.float32)
        v0 = (gs * gs * rng.uniform(0.05, 1, n)).astype(np.float32)
    return dict(p0=p0, grads=grads, m0=m0, v0=v0, t0=case['t0'])


def adam_ref_path(inp, hyper):
    """float64 Adam (torch.optim.Adam's update, no weight decay, no amsgrad) from step t0 + 1 on: the list of (p, m, v) after every step."""
    lr, b1, b2, eps, gs = hyper
    p, m, v = (inp[k].astype(np.float64) for k in ('p0', 'm0', 'v0'))
    out = []
    for k, g in enumerate(inp['grads']):
        t = inp['t0'] + k + 1
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        gi = g.astype(np.float64) * gs
        m = b1 * m + (1.0 - b1) * gi
        v = b2 * v + (1.0 - b2) * gi * gi
        p = p - (lr / bc1) * (m / (np.sqrt(v) * (1.0 / np.sqrt(bc2)) + eps))
        out.append((p, m, v))
    return out


def adam_ref(inp, hyper):
    """-> p, m, v after the last step."""
    return adam_ref_path(inp, hyper)[-1]


def adam_f32_path(inp, hyper):
    """The kernel's expression order (optim.hip adam_update, contraction off) in numpy float32, every operation rounded once; the step's scalars as
    da_adam_step / da_adam_host_state compute them."""
    F = np.float32
    lr, b1, b2, eps, gs = (F(h) for h in hyper)
    p, m, v = inp['p0'].copy(), inp['m0'].copy(), inp['v0'].copy()
    out = []
    for k, g in enumerate(inp['grads']):
        s = adam_host_state(hyper, inp['t0'] + k + 1)
        gi = g * gs
        m = b1 * m + (F(1) - b1) * gi
        v = b2 * v + (F(1) - b2) * gi * gi
        denom = np.sqrt(v) * s[4] + eps
        p = p - s[0] * (m / denom)
        assert p.dtype == m.dtype == v.dtype == np.float32
        out.append((p, m, v))
    return out


def adam_host_state(hyper, step):
    """da_adam_host_state restated: {lr / bc1, beta1, beta2, eps, 1 / sqrt(bc2), grad_scale} as float32, bc in double from the float32 betas."""
    lr, b1, b2, eps, gs = (float(np.float32(h)) for h in hyper)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return np.array([lr / bc1, b1, b2, eps, 1.0 / np.sqrt(bc2), gs], dtype=np.float64).astype(np.float32)


def adam_p_excess(p_got, p0, path, k):
    """The bound on p after k steps from p0, with disp = p_ref - p0:
        |p_got - p_ref| <= TOL * max|disp| + k * 2^-24 * max|p|      (the last maximum over p0 and the reference's path)
    Second term: p is stored in fp32 once per step, a rounding of at most 2^-24 |p| each; derived, no margin.  First term: what the update itself, of
    the size of the displacement, is off by.  Returns the part the first term has to absorb, in units of max|disp| (0 when the store term alone covers the
    error; inf when there is no displacement and it does not)."""
    p_ref = path[k - 1][0]
    pmax = max(float(np.abs(p0).max()), max(float(np.abs(path[j][0]).max()) for j in range(k)))
    disp = float(np.abs(p_ref - p0.astype(np.float64)).max())
    got = np.asarray(p_got, dtype=np.float64)
    assert np.isfinite(got).all(), 'non-finite parameter'
    over = float(np.abs(got - p_ref).max()) - k * 2.0 ** -24 * pmax
    if over <= 0:
        return 0.0
    return over / disp if disp > 0 else float('inf')


def adam_hyper_dev(betas, lr):
    """How far Adam with the float32-rounded hyper-parameters is from Adam with Python's, by construction, relative to the quantity itself:
    (m, v, update).  m scales with 1 - beta1 and v with 1 - beta2 (the first step from zero moments, where the bias correction is about 1, shows it in full:
    t large); the update m / sqrt(v) with their quotient, and with lr."""
    d1 = abs((1.0 - f32(betas[0])) - (1.0 - betas[0])) / (1.0 - betas[0])
    d2 = abs((1.0 - f32(betas[1])) - (1.0 - betas[1])) / (1.0 - betas[1])
    return d1, d2, d1 + 0.5 * d2 + abs(f32(lr) - lr) / lr


# Tolerances.  CEIL: what the suite asserted before these files (test_adam_vs_oracle: 1e-6).  TOL follows tests/loss_cases.py's rule: max(4 x device worst,
# 8 x fp32-restatement worst), both against the float64 reference, rounded up to two digits where that is more than 10 x below the ceiling; else the ceiling.
# The figures are in the table of tests/test_gpu_datapath_shapes.py.
CEIL = {'adam': {'p': 1e-6, 'm': 1e-6, 'v': 1e-6}}
TOL = {'adam': {'p': 1e-6, 'm': 1e-6, 'v': 1e-6}}
assert all(TOL[f][k] <= CEIL[f][k] for f in CEIL for k in CEIL[f])


# ---- weight layouts ---------------------------------------------------------------------------------------------------------------
# entry -> (shape of src from (A, B, K3), reference).  *_to_tio read the parameter layout [A][B][K3]; tio_to_* read [K3][Cin][Cout], where 'oik' has
# (A, B) = (Cout, Cin) and 'iok' (A, B) = (Cin, Cout).  numpy transpose / flip only.
def _par(A, B, K):
    return (A, B, K)


LAYOUT = {
    'da_w_oik_to_tio': (_par, lambda s: s.transpose(2, 1, 0)),                                   # dst[k][ci][co] = src[co][ci][k]
    'da_w_iok_to_tio': (_par, lambda s: s.transpose(2, 0, 1)),                                   # dst[k][ci][co] = src[ci][co][k]
    'da_w_iok_flip_to_tio': (_par, lambda s: np.flip(s, 2).transpose(2, 0, 1)),                  # dst[K-1-k][ci][co] = src[ci][co][k]
    'da_w_tio_to_oik': (lambda A, B, K: (K, B, A), lambda s: s.transpose(2, 1, 0)),              # dst[co][ci][k] = src[k][ci][co]
    'da_w_tio_to_iok': (lambda A, B, K: (K, A, B), lambda s: s.transpose(1, 2, 0)),              # dst[ci][co][k] = src[k][ci][co]
    'da_w_tio_to_iok_flip': (lambda A, B, K: (K, A, B), lambda s: np.flip(s, 0).transpose(1, 2, 0)),
}
LAYOUT_ACC = ['da_w_tio_to_oik_acc', 'da_w_tio_to_iok_acc', 'da_w_tio_to_iok_flip_acc']       # dst_before + LAYOUT[name without _acc]: one fp32 add per element
LAYOUT_PINNED = [dict(A=A, B=B, K3=K, sd=i) for i, (A, B, K) in
                 enumerate([(1, 1, 1), (1, 7, 8), (16, 1, 27), (3, 5, 1), (48, 16, 27), (16, 48, 8), (100, 101, 27)])]
assert LAYOUT_PINNED[-1]['A'] * LAYOUT_PINNED[-1]['B'] * LAYOUT_PINNED[-1]['K3'] >= LAYOUT_TRIP
LAYOUT_CASES = st.fixed_dictionaries(dict(A=st.integers(1, 40), B=st.integers(1, 40), K3=st.sampled_from([1, 8, 27]), sd=st.integers(0, 999)))


def distinct(shape, sd, dtype=np.float32):
    """A tensor whose elements are pairwise distinct (its index plus noise below 1 / 2): any index permutation changes it."""
    n = int(np.prod(shape))
    assert n < 2 ** 22                                    # fp32 keeps the quarter steps apart
    rng = np.random.default_rng(sd)
    a = (np.arange(n) + 0.25 * rng.integers(0, 2, n)).astype(dtype)
    return a.reshape(shape)


def layout_ref(name, src, dst_before=None):
    if name.endswith('_acc'):
        return (dst_before + np.ascontiguousarray(LAYOUT[name[:-4]][1](src))).astype(np.float32)
    return np.ascontiguousarray(LAYOUT[name][1](src))


# ---- clamp ------------------------------------------------------------------------------------------------------------------------
CLAMP_DTYPES = [np.float32, np.float64, np.int16, np.uint8, np.int32]       # the kernel's dtype codes 0 ... 4 (ops.PREPROCESS_DTYPE_CODE)
CLAMP_SIZES = [1, 257, TRIP + 3]
_FLOAT_EDGES = [0.0, 1.0, -0.0, 0.5, float('nan'), float('inf'), -float('inf'), 1.0000001, 0.99999994, -1e-30, 1e-45, 3.0e38, -3.0e38, 2.0 ** 24 + 2]
_F64_EDGES = _FLOAT_EDGES + [1 + 1e-12, 1 - 1e-12, -1e-300, 5e-324, 1e300, -1e300]
_INT_EDGES = {np.int16: [0, 1, -1, 2, -32768, 32767, 255, 256], np.uint8: [0, 1, 2, 255, 128], np.int32: [0, 1, -1, 2, -2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, -2 ** 24 - 1],
              np.int8: [0, 1, -1, 2, -128, 127], np.uint16: [0, 1, 2, 65535, 32768], np.uint32: [0, 1, 2, 2 ** 31 + 5, 2 ** 32 - 1, 2 ** 31],
              np.int64: [0, 1, -1, 2, -2 ** 32 + 1, 2 ** 32, 2 ** 32 + 1, -2 ** 63, 2 ** 63 - 1, 2 ** 24 + 1], np.uint64: [0, 1, 2, 2 ** 63 + 1, 2 ** 32, 2 ** 64 - 1]}
SITK_DTYPES = [np.float16, np.bool_, np.int8, np.uint16, np.uint32, np.int64, np.uint64] + CLAMP_DTYPES      # what SitkToTensor is handed beyond the kernel's five


def clamp_values(dtype, n, sd):
    """n values of `dtype`: its edge values first (cyclically repeated at the end too, so that a long array ends on them), noise around [0, 1] between."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(sd)
    if dtype.kind == 'f':
        edges = np.array(_F64_EDGES if dtype == np.float64 else _FLOAT_EDGES, dtype=np.float64)
        with np.errstate(over='ignore'):
            edges = edges.astype(dtype)
        body = rng.uniform(-1.0, 2.0, n).astype(dtype)
    elif dtype.kind == 'b':
        edges, body = np.array([False, True]), rng.integers(0, 2, n).astype(bool)
    else:
        edges = np.array(_INT_EDGES[dtype.type], dtype=dtype)
        body = rng.integers(-2 if dtype.kind == 'i' else 0, 4, n).astype(dtype)
    k = min(n, edges.size)
    body[:k] = edges[:k]
    if n >= 2 * edges.size:
        body[-edges.size:] = edges
    return body


def clamp_ref(a):
    """oracle.datapath.sitk_to_tensor without the channel axis: the clamp in the source dtype, then the cast."""
    with np.errstate(invalid='ignore', over='ignore'):
        return dp.sitk_to_tensor(a)[0][0]


CLAMP = st.fixed_dictionaries(dict(code=st.integers(0, 4), n=st.integers(1, 700), sd=st.integers(0, 999)))
CLAMP_PINNED = [dict(code=c, n=n, sd=10 * c + i) for c in range(5) for i, n in enumerate(CLAMP_SIZES[:2])] + [dict(code=c, n=CLAMP_SIZES[2], sd=50 + c) for c in (1, 2)]
SITK = st.fixed_dictionaries(dict(dtype=st.sampled_from(SITK_DTYPES), vol=st.tuples(st.integers(1, 5), st.integers(1, 6), st.integers(1, 9)),
                                  as_tensor=st.sampled_from(['numpy', 'host', 'device']), sd=st.integers(0, 999)))
SITK_PINNED = [dict(dtype=d, vol=(2, 3, 5), as_tensor=_cyc(['numpy', 'device', 'host'], i + j), sd=i) for i, d in enumerate(SITK_DTYPES) for j in range(2)]


def same_bits(got, ref):
    """Bit equality of two arrays of one dtype and shape, except that a NaN only has to be a NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    if got.dtype.kind != 'f':
        return bool(np.array_equal(got, ref))
    nan = np.isnan(ref)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(bits)[~nan], ref.view(bits)[~nan]))


# ---- crop -------------------------------------------------------------------------------------------------------------------------
def _crop_case(c):
    lo = tuple(l % s for l, s in zip(c['lo'], c['vol']))
    hi = tuple(h % (s - l) for h, s, l in zip(c['hi'], c['vol'], lo))
    return dict(lead=c['lead'], vol=c['vol'], crop=lo + hi, bytes=c['bytes'], sd=c['sd'])


_dims = st.tuples(st.integers(1, 12), st.integers(1, 12), st.integers(1, 12))
CROP = st.fixed_dictionaries(dict(lead=st.integers(1, 3), vol=_dims, lo=st.tuples(*[st.integers(0, 11)] * 3), hi=st.tuples(*[st.integers(0, 11)] * 3),
                                  bytes=st.sampled_from([1, 4]), sd=st.integers(0, 999))).map(_crop_case)
CROP_BIG = dict(lead=3, vol=(74, 75, 76), crop=(1, 2, 0, 0, 1, 3), bytes=4, sd=9)
assert 3 * 73 * 72 * 73 >= TRIP
CROP_PINNED = [dict(lead=1, vol=(5, 6, 7), crop=(0, 0, 0, 0, 0, 0), bytes=4, sd=1),          # a zero crop
               dict(lead=2, vol=(5, 6, 7), crop=(2, 2, 3, 2, 3, 3), bytes=1, sd=2),          # one voxel left
               dict(lead=3, vol=(1, 1, 9), crop=(0, 0, 4, 0, 0, 4), bytes=4, sd=3),          # axes of length 1
               dict(lead=1, vol=(9, 11, 13), crop=(1, 2, 3, 1, 2, 3), bytes=1, sd=4),        # the 3-value form
               dict(lead=2, vol=(9, 11, 13), crop=(3, 0, 5, 0, 4, 1), bytes=4, sd=5),
               CROP_BIG]


def crop_values(shape, nbytes, sd):
    if nbytes == 4:
        return distinct(shape, sd)
    return np.random.default_rng(sd).integers(0, 256, shape).astype(np.uint8)


def crop_ref(a, crop):
    """oracle.datapath.crop_tensor on [lead][D][H][W]."""
    return np.ascontiguousarray(dp.crop_tensor(a, None, list(crop))[0])


def crop_out_shape(case):
    c, (D, H, W) = case['crop'], case['vol']
    return (case['lead'], D - c[0] - c[3], H - c[1] - c[4], W - c[2] - c[5])


# ---- partition / assemble / vote --------------------------------------------------------------------------------------------------
def reflect_idx(i, n):
    """datapath.hip reflect_idx: numpy.pad(mode='reflect'), mirror without repeating the edge, as often as the pad needs."""
    if n == 1:
        return 0
    period = 2 * (n - 1)
    m = i % period                                        # Python's % is already non-negative
    return m if m < n else period - m


def geom(case):
    """(effective sizes, tile grid) of a case; numpy order z, y, x."""
    eff = tuple(t - 2 * o for t, o in zip(case['tile'], case['ov']))
    assert min(eff) > 0
    return eff, tuple(-(-s // e) for s, e in zip(case['vol'], eff))


def cover_bound(case):
    """da_assemble_tiles' bound on the tiles that vote at one voxel: ceil(tz / ez) ceil(ty / ey) ceil(tx / ex); above 64 the entry declines."""
    eff, _ = geom(case)
    return int(np.prod([-(-t // e) for t, e in zip(case['tile'], eff)]))


def cover_max(case):
    """The largest number of tiles that do cover one voxel of the volume (padded coordinate p = z + o is covered by tile a iff a e <= p < a e + t)."""
    eff, grid = geom(case)
    out = 1
    for s, t, o, e, g in zip(case['vol'], case['tile'], case['ov'], eff, grid):
        out *= max(sum(1 for a in range(g) if a * e <= z + o < a * e + t) for z in range(s))
    return out


def _geom_case(c):
    return dict(vol=c['vol'], tile=c['tile'], ov=tuple(o % ((t - 1) // 2 + 1) for o, t in zip(c['ov'], c['tile'])), bytes=c['bytes'], sd=c['sd'])


_vol14 = st.tuples(st.integers(1, 14), st.integers(1, 14), st.integers(1, 14))
GEOM = st.fixed_dictionaries(dict(vol=_vol14, tile=st.tuples(*[st.integers(1, 10)] * 3), ov=st.tuples(*[st.integers(0, 4)] * 3),
                                  bytes=st.sampled_from([1, 4]), sd=st.integers(0, 999))).map(_geom_case)
GEOM_SMALL = [
    dict(vol=(1, 6, 7), tile=(3, 4, 5), ov=(1, 1, 2)),            # an axis of length 1 (with an overlap on it: every source index is 0)
    dict(vol=(3, 5, 4), tile=(9, 6, 7), ov=(4, 1, 2)),            # an overlap larger than the axis: the leading pad reflects more than once
    dict(vol=(2, 3, 11), tile=(9, 10, 9), ov=(1, 2, 0)),          # a trailing pad larger than the axis: the last tile hangs far past the volume
    dict(vol=(7, 9, 5), tile=(3, 4, 5), ov=(0, 0, 0)),            # overlap 0
    dict(vol=(6, 7, 8), tile=(6, 7, 8), ov=(0, 0, 0)),            # tile equal to the volume
    dict(vol=(4, 5, 3), tile=(8, 9, 10), ov=(1, 2, 3)),           # tile larger than the volume
    dict(vol=(7, 8, 9), tile=(8, 8, 8), ov=(3, 3, 3)),            # exactly 64 covering tiles
    dict(vol=(13, 14, 1), tile=(5, 4, 1), ov=(2, 1, 0)),
]
GEOM_DECLINE = dict(vol=(9, 10, 11), tile=(10, 10, 10), ov=(4, 4, 4))          # 125 covering tiles: the vote declines
PARTITION_BIG = dict(vol=(50, 60, 70), tile=(24, 24, 24), ov=(4, 4, 4))        # 80 tiles of 13 824 elements
ASSEMBLE_BIG = dict(vol=(102, 103, 107), tile=(40, 40, 40), ov=(3, 3, 3))
VOTE_BIG = dict(vol=(102, 103, 107), tile=(40, 40, 40), ov=(6, 6, 6))          # 4 x 4 x 4 tiles
assert int(np.prod(geom(PARTITION_BIG)[1])) * 24 ** 3 >= TRIP and 102 * 103 * 107 >= TRIP and int(np.prod(geom(VOTE_BIG)[1])) == 64
assert cover_bound(GEOM_SMALL[6]) == 64 and cover_bound(GEOM_DECLINE) == 125


def _with(cases, **kw):
    return [dict(c, bytes=_cyc([4, 1], i), sd=i, **kw) for i, c in enumerate(cases)]


PARTITION_PINNED = _with(GEOM_SMALL + [GEOM_DECLINE]) + [dict(c, bytes=1 + 3 * (i % 2), sd=20 + i) for i, c in enumerate(GEOM_SMALL)] + [dict(PARTITION_BIG, bytes=4, sd=40)]
ASSEMBLE_PINNED = _with(GEOM_SMALL + [GEOM_DECLINE]) + [dict(ASSEMBLE_BIG, bytes=4, sd=41), dict(ASSEMBLE_BIG, bytes=1, sd=42)]
# label sets: 0 .. L-1 (the reference's own definition applies) and gapped ones (the documented extension: most votes, ties to the smallest label)
LABEL_SETS = [(0, 1), (0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 3, 4), (0, 3, 7), (2, 5), (1, 2, 3, 255), (0, 255)]
VOTE_PINNED = ([dict(c, bytes=1, sd=i, labels=_cyc(LABEL_SETS, i)) for i, c in enumerate(GEOM_SMALL)] +
               [dict(GEOM_SMALL[6], bytes=1, sd=30, labels=(0, 3, 7)), dict(GEOM_SMALL[1], bytes=1, sd=31, labels=(0, 1)),
                dict(GEOM_DECLINE, bytes=1, sd=32, labels=(0, 1, 2)), dict(VOTE_BIG, bytes=1, sd=33, labels=(0, 1, 2, 3))])


def _vote_case(c):
    return dict(_geom_case(c), labels=c['labels'])


# GEOM's geometries with a label set.  A geometry declines only when the three overlaps are near (tile - 1) / 2 at once (cover bound above 64): the 60
# derandomised draws hold none, the CPU companion asserts at most VOTE_DECLINE_MAX
VOTE = st.fixed_dictionaries(dict(vol=_vol14, tile=st.tuples(*[st.integers(1, 10)] * 3), ov=st.tuples(*[st.integers(0, 4)] * 3),
                                  bytes=st.just(1), labels=st.sampled_from(LABEL_SETS), sd=st.integers(0, 999))).map(_vote_case)
VOTE_DECLINE_MAX = 6       # 10 % of the 60 drawn cases


def volume_values(case):
    if case['bytes'] == 4:
        return distinct(case['vol'], case['sd'])
    return np.random.default_rng(case['sd']).integers(0, 256, case['vol']).astype(np.uint8)


def _oracle_partition(case):
    return dp.Partition(tuple(reversed(case['tile'])), tuple(reversed(case['ov'])))          # (the reference takes SimpleITK order x, y, z and flips)


def partition_ref(case, vol):
    """oracle.datapath.Partition's tiles [T][tz][ty][tx]."""
    return np.ascontiguousarray(_oracle_partition(case).tiles(vol))


def partition_brute(case, vol, index=reflect_idx):
    """The definition per voxel: tiles[(i gy + j) gx + k][z][y][x] = vol[r(i ez + z - oz)][r(j ey + y - oy)][r(k ex + x - ox)], r = reflect_idx."""
    eff, grid = geom(case)
    src = [np.array([[index(a * e + z - o, s) for z in range(t)] for a in range(g)]) for s, t, o, e, g in zip(case['vol'], case['tile'], case['ov'], eff, grid)]
    out = vol[src[0][:, None, None, :, None, None], src[1][None, :, None, None, :, None], src[2][None, None, :, None, None, :]]
    return np.ascontiguousarray(out.reshape((-1,) + tuple(case['tile'])))


def assemble_ref(case, tiles):
    """oracle.datapath.Partition.assemble(is_vote=False) (float64 there), in the tiles' dtype."""
    part = _oracle_partition(case)
    part.tiles(np.zeros(case['vol'], dtype=np.uint8))                                        # (sets size / eff / grid)
    return np.ascontiguousarray(part.assemble(tiles).astype(tiles.dtype))


def label_volume(case):
    """A blocky label map over the case's label set."""
    D, H, W = case['vol']
    labs = np.array(case['labels'], dtype=np.uint8)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    return labs[((z // max(D // 3, 1)) * 2 + (y // max(H // 3, 1)) * 3 + x // max(W // 4, 1) + case['sd']) % labs.size]


def noisy_tiles(case):
    """The partition of label_volume with 20 % of the tile voxels relabelled at random within the label set: uint8 [T][tz][ty][tx]."""
    tiles = partition_brute(case, label_volume(case)).copy()
    rng = np.random.default_rng(77 + case['sd'])
    flip = rng.random(tiles.shape) < 0.2
    tiles[flip] = np.array(case['labels'], dtype=np.uint8)[rng.integers(0, len(case['labels']), int(flip.sum()))]
    return tiles


def vote_ref(case, tiles, ties='smallest'):
    """The vote: the label most of the covering tiles name, ties to the smallest label.  Where the labels present are exactly 0 .. L-1 this is
    oracle.datapath.Partition.assemble(is_vote=True) as it stands (it indexes its vote array by label value); any other set takes the same sums indexed by
    the label's rank, the documented extension."""
    present = np.unique(tiles)
    if ties == 'smallest' and np.array_equal(present, np.arange(present.size)):
        part = _oracle_partition(case)
        part.tiles(np.zeros(case['vol'], dtype=np.uint8))
        return np.ascontiguousarray(part.assemble(tiles, is_vote=True))
    eff, grid = geom(case)
    (tz, ty, tx), (oz, oy, ox), (D, H, W) = case['tile'], case['ov'], case['vol']
    votes = np.zeros((present.size,) + tuple(e * g + 2 * o for e, g, o in zip(eff, grid, case['ov'])), dtype=np.int64)
    for i in range(grid[0]):
        for j in range(grid[1]):
            for k in range(grid[2]):
                t = tiles[(i * grid[1] + j) * grid[2] + k]
                for r, lab in enumerate(present):
                    votes[r, i * eff[0]:i * eff[0] + tz, j * eff[1]:j * eff[1] + ty, k * eff[2]:k * eff[2] + tx] += (t == lab)
    if ties == 'largest':                                 # (the CPU companion's mutant)
        win = present[present.size - 1 - np.argmax(votes[::-1], 0)]
    else:
        win = present[np.argmax(votes, 0)]
    return np.ascontiguousarray(win[oz:oz + D, oy:oy + H, ox:ox + W].astype(np.uint8))


def vote_brute(case, tiles):
    """The vote by its definition, one voxel at a time; also returns the number of voxels whose winner was decided by a tie."""
    eff, grid = geom(case)
    (tz, ty, tx), (oz, oy, ox), (D, H, W) = case['tile'], case['ov'], case['vol']
    out = np.zeros((D, H, W), dtype=np.uint8)
    ties = 0
    cov = [[[a for a in range(g) if a * e <= z + o < a * e + t] for z in range(s)] for s, t, o, e, g in zip(case['vol'], case['tile'], case['ov'], eff, grid)]
    for z in range(D):
        for y in range(H):
            for x in range(W):
                count = {}
                for a in cov[0][z]:
                    for b in cov[1][y]:
                        for c in cov[2][x]:
                            lab = int(tiles[(a * grid[1] + b) * grid[2] + c, z + oz - a * eff[0], y + oy - b * eff[1], x + ox - c * eff[2]])
                            count[lab] = count.get(lab, 0) + 1
                top = max(count.values())
                winners = sorted(l for l, n in count.items() if n == top)
                ties += len(winners) > 1
                out[z, y, x] = winners[0]
    return out, ties


# ---- casts ------------------------------------------------------------------------------------------------------------------------
CAST_N = [1, 2, 3, 4, 5, 7, 1023, 4 * cast_second_trip() + 1203]
_CAST_EDGES = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 3.4028234663852886e38, -3.4028234663852886e38, 0.0, -0.0,
                        float('inf'), -float('inf'), float('nan'), 1.0, 1 + 2.0 ** -7, 3.3895313892515355e38, 2.0 ** -126, 1 + 2.0 ** -8 + 2.0 ** -23,
                        1 + 2.0 ** -8 - 2.0 ** -24], dtype=np.float32)
CAST = st.fixed_dictionaries(dict(n=st.integers(1, 3000), sd=st.integers(0, 999)))
CAST_PINNED = [dict(n=n, sd=i) for i, n in enumerate(CAST_N)] + [dict(n=40 + i, sd=20 + i) for i in range(4)]


def cast_values(case):
    """n NORMAL fp32 values over the whole exponent range (fp32 subnormals are left out: activations never hold them), the edge values first and,
    where there is room, again at the very end, so that the vector body and the scalar tail both meet them.  A short array takes its edges from position
    sd on, so that the sizes 1 ... 7 do not all see the same ones."""
    n = case['n']
    rng = np.random.default_rng(case['sd'])
    bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | (rng.integers(1, 255, n).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, n).astype(np.uint32)
    x = bits.view(np.float32).copy()
    e = np.roll(_CAST_EDGES, -case['sd'])
    k = min(n, e.size)
    x[:k] = e[:k]
    if n >= 2 * e.size:
        x[-e.size:] = e
    return x


def bf16_bits_ref(x):
    """torch on the CPU: x.bfloat16() (round to nearest even) as uint16 bit patterns."""
    return torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)


def bf16_values(case):
    """n bf16 bit patterns (any: subnormals, infinities and NaNs included -- the widening is a shift)."""
    rng = np.random.default_rng(500 + case['sd'])
    b = rng.integers(0, 1 << 16, case['n']).astype(np.uint16)
    e = bf16_bits_ref(_CAST_EDGES)
    k = min(case['n'], e.size)
    b[:k] = e[:k]
    return b


def f32_from_bf16_ref(bits):
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).float().numpy()


def same_bf16(got_bits, ref_bits):
    """Bit equality of bf16 patterns, except that a NaN only has to be a NaN."""
    nan = (ref_bits & 0x7FFF) > 0x7F80
    return bool(np.array_equal((got_bits & 0x7FFF) > 0x7F80, nan) and np.array_equal(got_bits[~nan], ref_bits[~nan]))


# ---- synthetic volumes ------------------------------------------------------------------------------------------------------------
def _synth_case(c):
    V = int(np.prod(c['vol']))
    s0 = c['sample0']
    if s0 == 'cross':                                     # (sample0 + n) V + v crosses 2^32 inside the batch: the hash input's high word changes
        s0 = max(2 ** 32 // V - (c['N'] - 1) // 2, 0) if V >= 3 else 0
    return dict(N=c['N'], vol=c['vol'], C=c['C'], mode=c['mode'], noise=c['noise'], seed=c['seed'], sample0=int(s0), which=c['which'])


_synth_raw = dict(N=st.integers(1, 3), vol=st.tuples(st.integers(1, 20), st.integers(1, 20), st.integers(1, 20)), C=st.sampled_from([1, 2, 32, 256]),
                  mode=st.sampled_from([0, 1]), noise=st.sampled_from([0.0, 0.1, 1.5]), seed=st.integers(0, 2 ** 32 - 1), sample0=st.sampled_from([0, 5, 'cross']),
                  which=st.sampled_from(['both', 'both', 'img', 'lab']))
SYNTH = st.fixed_dictionaries(_synth_raw).map(_synth_case)
SYNTH_PINNED = [_synth_case(dict(N=1 + i % 3, vol=_cyc([(5, 6, 7), (9, 16, 23), (3, 17, 8), (16, 7, 24)], i), C=C, mode=mode, noise=_cyc([0.0, 0.1, 1.5], i + mode),
                                 seed=_cyc([230, 0, 2 ** 32 - 1], i), sample0=_cyc(['cross', 0, 5], i + mode), which=_cyc(['both', 'img', 'lab'], i // 2)))
                for i, (C, mode) in enumerate((C, mode) for C in (1, 2, 32, 256) for mode in (0, 1))]
SYNTH_PINNED += [_synth_case(dict(N=3, vol=(5, 6, 7), C=32, mode=mode, noise=1.5, seed=7, sample0='cross', which='both')) for mode in (0, 1)]
SYNTH_PINNED += [_synth_case(dict(N=2, vol=(64, 96, 100), C=256, mode=mode, noise=0.1, seed=11, sample0=3, which='both')) for mode in (0, 1)]
assert 2 * 64 * 96 * 100 >= TRIP


def synth_crosses(case):
    V = int(np.prod(case['vol']))
    return case['sample0'] * V < 2 ** 32 <= (case['sample0'] + case['N']) * V - 1


def synth_ref(case):
    return dp.synth_volume(case['N'], case['vol'], case['C'], case['mode'], case['noise'], case['seed'], sample0=case['sample0'])
