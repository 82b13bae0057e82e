"""Cases, references and tolerances of the native-grid registration route (csrc/regapply.hip, ops.bspline_prefilter, ops.warp_to_grid).

References, float64:
  prefilter   scipy.ndimage.spline_filter(x.astype(float64), 3, mode='mirror')
  warp        warp_reference(): steps 1 - 6 of include/deepatlas_hip.h's da_warp_frames restated in numpy; order 3 is the 64-tap sum with
              mirrored indices over the float64 scipy coefficients.  scipy's mode='constant' returns cval on [-0.5, 0), which is not the
              inside rule here (-0.5 <= y < n - 0.5), so the inside test is the restatement's own.
The float32 restatements (prefilter_f32, warp_reference(..., dtype=float32)) evaluate the same formulas with the recursion and the coordinates
in float32; B[u] takes the normalised coordinate g = p / (size - 1) * 2 - 1 and un-normalises it again, as fieldinv.hip defines it, and the
float32 restatement forms it in float32.  Tolerance of a case: a kernel must be within TOL_FACTOR x the float32 restatement's own distance
(largest absolute difference) from the float64 reference on the same case, the project's margin for a different but equally valid float32
ordering, and never less than FLOOR x max |source|.
Guard band: a voxel whose REFERENCE sample position lies within GUARD of a decision boundary -- the inside-test edges -0.5 and n - 0.5 at
every order, the half-integers at order 0 -- is left out of the value comparison; at most GUARD_CAP of a case's voxels may be.
Grid rule: da_warp_frames walks the output voxels with a grid-stride loop of da_grid(V, 256) workgroups capped at 4096 (rounded down to a
multiple of 8): second_trip_voxels() is the smallest count at which a lane takes a second trip."""
import functools

import numpy as np

TOL_FACTOR = 4.0
FLOOR = 1e-6
GUARD = 1e-3
GUARD_CAP = 0.02
DEFAULT = -7            # what outside voxels get in the tests (a value no signed or float source holds; uint8 sources get 7)
BLOCK = 256
GRID_CAP = 256 * 16     # common.h da_grid
POLE = np.sqrt(3.0) - 2.0

PREFILTER_LINES = (1, 2, 3, 64, 65, 200)
RAGGED = ((5, 7, 67), (3, 130, 9))
DTYPES = ('uint8', 'int16', 'int32', 'float32')


def da_grid(work_items, block=BLOCK, cap=GRID_CAP):
    return int(min(max(-(-work_items // block), 1), cap))


def warp_blocks(V):
    g = da_grid(V)
    return g // 8 * 8 if g >= 8 else g


def second_trip_voxels():
    n = GRID_CAP * BLOCK + 1
    assert warp_blocks(n) * BLOCK < n and warp_blocks(n - 1) * BLOCK >= n - 1
    return n


def prefilter_shapes():
    """Every line length along every axis, the ragged volumes, and a volume longer than the row pass's workgroup on every axis."""
    shapes = []
    for n in PREFILTER_LINES:
        shapes += [(n, 3, 5), (3, n, 5), (2, 3, n)]
    return sorted(set(shapes + list(RAGGED) + [(1, 1, 1), (1, 1, 300)]))


# ---- prefilter --------------------------------------------------------------------------------------------------------------------------
def prefilter_ref64(x):
    from scipy import ndimage
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 4:
        return np.stack([prefilter_ref64(c) for c in x])
    return ndimage.spline_filter(x, 3, output=np.float64, mode='mirror')


def mirror(i, n):
    """Whole-sample mirror of integers onto 0 ... n - 1 (period 2 n - 2; n = 1: 0)."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    per = 2 * n - 2
    m = np.mod(i, per)
    return np.where(m < n, m, per - m)


def prefilter_f32(x, horizon=32):
    """The recursive filter in float32, axis by axis (W, H, D): c+[0] = 6 sum_k z^k x[mirror(k)] over `horizon` terms, c+[k] = 6 x[k] +
    z c+[k - 1], c[n - 1] = z / (z^2 - 1) (c+[n - 1] + z c+[n - 2]), c[k] = z (c[k + 1] - c+[k])."""
    f = np.float32
    z = f(POLE)
    c = np.array(x, dtype=np.float32)
    lead = c.ndim - 3
    for axis in (2, 1, 0):
        n = c.shape[lead + axis]
        if n == 1:
            continue
        v = np.moveaxis(c, lead + axis, 0).copy()
        idx = mirror(np.arange(horizon + 1), n)
        acc = v[idx[horizon]].copy()
        for k in range(horizon - 1, -1, -1):
            acc = (acc * z + v[idx[k]]).astype(f)
        cp = np.empty_like(v)
        cp[0] = (acc * f(6)).astype(f)
        for k in range(1, n):
            cp[k] = (f(6) * v[k] + z * cp[k - 1]).astype(f)
        out = np.empty_like(v)
        out[n - 1] = (f(POLE / (POLE * POLE - 1.0)) * (cp[n - 1] + z * cp[n - 2])).astype(f)
        for k in range(n - 2, -1, -1):
            out[k] = (z * (out[k + 1] - cp[k])).astype(f)
        c = np.moveaxis(out, 0, lead + axis)
    return np.ascontiguousarray(c)


# ---- warp -------------------------------------------------------------------------------------------------------------------------------
def sample_field_border(disp, p, dtype):
    """B[u] in voxels at continuous prepared indices p [3][...] ((D, H, W) order): disp [3][Dp][Hp][Wp] normalised, channel 0 = x (W axis).
    The index is clamped to [0, size - 1]; a tap of index `size` has weight 0 and is not read (so a NaN there does not spread)."""
    f = dtype
    size = disp.shape[1:]
    lo, frac = [], []
    for a in range(3):
        n = size[a]
        g = (p[a] / f(n - 1) * f(2) - f(1)).astype(f)
        r = (((g + f(1)) / f(2)) * f(n - 1)).astype(f)
        r = np.minimum(np.maximum(r, f(0)), f(n - 1))
        fl = np.floor(r)
        lo.append(np.clip(fl.astype(np.int64), 0, n - 1))
        frac.append((r - fl).astype(f))
    u = []
    for a, ch in ((0, 2), (1, 1), (2, 0)):                # axis D reads channel 2 (z), H channel 1, W channel 0
        acc = np.zeros(p[0].shape, dtype=f)
        for k in range(8):
            cz, cy, cx = k >> 2, (k >> 1) & 1, k & 1
            iz, iy, ix = lo[0] + cz, lo[1] + cy, lo[2] + cx
            ok = (iz < size[0]) & (iy < size[1]) & (ix < size[2])
            w = ((frac[2] if cx else (f(1) - frac[2])) * (frac[1] if cy else (f(1) - frac[1])) * (frac[0] if cz else (f(1) - frac[0]))).astype(f)
            val = disp[ch][np.minimum(iz, size[0] - 1), np.minimum(iy, size[1] - 1), np.minimum(ix, size[2] - 1)].astype(f)
            with np.errstate(invalid='ignore'):
                acc = np.where(ok, acc + val * w, acc).astype(f)
        u.append((acc * f((size[a] - 1) / 2.0)).astype(f))
    return u


def sample_positions(disp, out_size, fixed_frame, moving_frame, dtype=np.float64):
    """Steps 1 - 4: y [3][Do][Ho][Wo] on the moving file's grid, in `dtype`."""
    f = dtype
    disp = np.asarray(disp)
    grids = np.meshgrid(*[np.arange(n, dtype=f) for n in out_size], indexing='ij')
    p = [((grids[a] - f(fixed_frame[a][1])) / f(fixed_frame[a][0])).astype(f) for a in range(3)]
    u = sample_field_border(disp.astype(f) if f == np.float64 else disp.astype(np.float32), p, f)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([(f(moving_frame[a][0]) * (p[a] + u[a]).astype(f) + f(moving_frame[a][1])).astype(f) for a in range(3)])


def cubic_weights(t, f):
    t2, t3, s = t * t, t * t * t, f(1) - t
    return [(s * s * s / f(6)).astype(f), ((f(3) * t3 - f(6) * t2 + f(4)) / f(6)).astype(f),
            ((f(-3) * t3 + f(3) * t2 + f(3) * t + f(1)) / f(6)).astype(f), (t3 / f(6)).astype(f)]


def interpolate(src, y, order, dtype=np.float64):
    """Step 6 at positions y [3][...] that are inside: src [C][Dm][Hm][Wm] (order 3: the coefficients)."""
    f = dtype
    n = src.shape[1:]
    if order == 0:
        idx = [np.clip(np.floor(y[a] + f(0.5)).astype(np.int64), 0, n[a] - 1) for a in range(3)]
        return src[:, idx[0], idx[1], idx[2]]
    fl = [np.floor(y[a]) for a in range(3)]
    if order == 1:
        lo = [np.clip(fl[a].astype(np.int64), 0, n[a] - 1) for a in range(3)]
        hi = [np.minimum(lo[a] + 1, n[a] - 1) for a in range(3)]
        t = [np.where(y[a] < 0, f(0), y[a] - fl[a]).astype(f) for a in range(3)]
        s = src.astype(f)
        lerp = lambda a, b, w: (a + w * (b - a)).astype(f)
        planes = []
        for zi in (lo[0], hi[0]):
            rows = [lerp(s[:, zi, yi, lo[2]], s[:, zi, yi, hi[2]], t[2]) for yi in (lo[1], hi[1])]
            planes.append(lerp(rows[0], rows[1], t[1]))
        return lerp(planes[0], planes[1], t[0])
    w = [cubic_weights((y[a] - fl[a]).astype(f), f) for a in range(3)]
    ix = [[mirror(fl[a].astype(np.int64) - 1 + k, n[a]) for k in range(4)] for a in range(3)]
    s = src.astype(f)
    out = np.zeros((src.shape[0],) + y[0].shape, dtype=f)
    for i in range(4):
        sh = np.zeros_like(out)
        for j in range(4):
            sw = np.zeros_like(out)
            for k in range(4):
                sw = (sw + w[2][k] * s[:, ix[0][i], ix[1][j], ix[2][k]]).astype(f)
            sh = (sh + w[1][j] * sw).astype(f)
        out = (out + w[0][i] * sh).astype(f)
    return out


def warp_reference(src, disp, out_size, fixed_frame, moving_frame, order, default=DEFAULT, dtype=np.float64):
    """(out [C][Do][Ho][Wo], y [3][Do][Ho][Wo], inside, finite).  src [C][Dm][Hm][Wm]: the source (orders 0, 1) or the spline coefficients
    (order 3).  Order 0 returns the source dtype, the others `dtype`.  A position that is not finite or >= 1e9 gives NaN (floating-point
    output) or `default` (integer output)."""
    src = np.asarray(src)
    y = sample_positions(disp, out_size, fixed_frame, moving_frame, dtype)
    with np.errstate(invalid='ignore'):
        finite = np.all(np.abs(y) < 1e9, axis=0)
        n = src.shape[1:]
        inside = finite & np.all([(y[a] >= -0.5) & (y[a] < n[a] - 0.5) for a in range(3)], axis=0)
    ys = np.where(inside[None], y, 0)
    val = interpolate(src, ys, order, dtype)
    out_dtype = src.dtype if order == 0 else dtype
    out = np.where(inside[None], val, np.asarray(default).astype(out_dtype)).astype(out_dtype)
    if np.issubdtype(out_dtype, np.floating):
        out = np.where(finite[None], out, np.nan).astype(out_dtype)
    return out, y, inside, finite


def guard_mask(y, shape, order):
    """True where the reference position is within GUARD of a decision boundary."""
    with np.errstate(invalid='ignore'):
        near = np.zeros(y.shape[1:], dtype=bool)
        for a in range(3):
            near |= (np.abs(y[a] + 0.5) < GUARD) | (np.abs(y[a] - (shape[a] - 0.5)) < GUARD)
            if order == 0:
                near |= np.abs(y[a] - np.floor(y[a]) - 0.5) < GUARD
    return near


def world_reference(y, A_f, A_m):
    """d(x) = A_m (y, 1) - A_f (x, 1) in float64, [3][Do][Ho][Wo]; the affines act on (i, j, k) = (w, h, d)."""
    A_f, A_m = np.asarray(A_f, dtype=np.float64), np.asarray(A_m, dtype=np.float64)
    x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in y.shape[1:]], indexing='ij')
    out = []
    for r in range(3):
        m = A_m[r, 0] * y[2] + A_m[r, 1] * y[1] + A_m[r, 2] * y[0] + A_m[r, 3]
        fx = A_f[r, 0] * x[2] + A_f[r, 1] * x[1] + A_f[r, 2] * x[0] + A_f[r, 3]
        out.append(m - fx)
    return np.stack(out)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def make_source(shape, dtype, seed, channels=1):
    rng = np.random.RandomState(seed)
    if dtype == 'float32':
        return rng.standard_normal((channels,) + tuple(shape)).astype(np.float32)
    hi = {'uint8': 255, 'int16': 3000, 'int32': 100000}[dtype]
    lo = 0 if dtype == 'uint8' else -hi // 3
    return rng.randint(lo, hi + 1, size=(channels,) + tuple(shape)).astype(dtype)


def make_field(size, amp_vox, seed, push=None):
    """[3][Dp][Hp][Wp] float32, normalised, channel 0 = x: amp_vox x (0.7 smooth + 0.3 uniform noise) voxels per channel; push = (channel,
    voxels) adds a constant to one channel."""
    rng = np.random.RandomState(seed)
    z, y, x = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in size], indexing='ij')
    out = []
    for ch in range(3):
        ph = rng.uniform(0, 2 * np.pi, 3)
        smooth = np.sin(2 * np.pi * z + ph[0]) * np.cos(2 * np.pi * y + ph[1]) * np.sin(3 * np.pi * x + ph[2])
        vox = amp_vox * (0.7 * smooth + 0.3 * rng.uniform(-1, 1, size))
        if push is not None and push[0] == ch:
            vox = vox + push[1]
        out.append(vox / ((size[2 - ch] - 1) / 2.0))
    return np.stack(out).astype(np.float32)


IDENTITY = ((1.0, 0.0),) * 3


def default_of(dtype):
    return 7 if np.dtype(dtype) == np.uint8 else DEFAULT

# three different grids: scales 1 / 0.7, 1, 2.5 (and 0.7, 0.4 on the moving side), the moving D axis flipped, crop offsets on every axis
THREE = {'moving': (9, 20, 33), 'prepared': (8, 16, 24), 'fixed': (11, 18, 30),
         'fixed_frame': ((1.0 / 0.7, 0.3), (1.0, 1.0), (1.25, 0.5)), 'moving_frame': ((-0.7, 6.5), (1.0, 3.0), (1.0 / 2.5, 12.0))}


def warp_cases():
    """name -> dict(moving, prepared, fixed, fixed_frame, moving_frame, amp, seed, dtype, channels[, push])."""
    cases = {}
    for k, amp in enumerate((0.3, 2.0, 8.0)):
        cases['three_amp%g' % amp] = dict(THREE, amp=amp, seed=10 + k, dtype=DTYPES[k + 1], channels=1 + k % 2)
        for j, shape in enumerate(RAGGED):
            cases['ragged%d_amp%g' % (j, amp)] = dict(moving=shape, prepared=shape, fixed=shape, fixed_frame=IDENTITY, moving_frame=IDENTITY,
                                                      amp=amp, seed=20 + 3 * j + k, dtype=DTYPES[(k + j) % 4], channels=1)
    cases['three_uint8_c2'] = dict(THREE, amp=1.0, seed=30, dtype='uint8', channels=2)
    cases['push_third_out'] = dict(THREE, amp=0.5, seed=31, dtype='float32', channels=1, push=(1, 6.0))       # +6 voxels along H: y_H past 19.5 for about a third
    cases['moving_extent1'] = dict(THREE, moving=(1, 20, 33), moving_frame=((0.05, -0.1), (1.0, 3.0), (0.4, 12.0)), amp=1.0, seed=32, dtype='int16', channels=1)
    big = (64, 128, 131)
    assert int(np.prod(big)) >= second_trip_voxels()
    cases['second_trip'] = dict(THREE, fixed=big, fixed_frame=((64.0 / 7.5, 0.0), (128.0 / 15.5, 1.0), (131.0 / 23.5, 0.5)), amp=2.0, seed=33,
                                dtype='int16', channels=1)
    return cases


@functools.lru_cache(maxsize=None)
def build_case(name):
    """The arrays of a case, built once and shared: source, field, float64 coefficients."""
    c = dict(warp_cases()[name])
    c['name'] = name
    c['src'] = make_source(c['moving'], c['dtype'], c['seed'], c['channels'])
    c['disp'] = make_field(c['prepared'], c['amp'], c['seed'] + 100, c.get('push'))
    c['coef64'] = prefilter_ref64(c['src'])
    c['src'].setflags(write=False); c['disp'].setflags(write=False); c['coef64'].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case_reference(name, order):
    """(reference out, y, compare mask, tolerance, excluded share, float32 restatement's distance) of a case at an order."""
    c = build_case(name)
    src64 = c['coef64'] if order == 3 else c['src']
    dflt = default_of(c['dtype'])
    ref, y, inside, finite = warp_reference(src64, c['disp'], c['fixed'], c['fixed_frame'], c['moving_frame'], order, dflt)
    src32 = prefilter_f32(c['src']) if order == 3 else c['src']
    low, _, _, _ = warp_reference(src32, c['disp'], c['fixed'], c['fixed_frame'], c['moving_frame'], order, dflt, dtype=np.float32)
    keep = ~guard_mask(y, c['moving'], order) & finite
    dist = float(np.max(np.abs(low.astype(np.float64) - ref.astype(np.float64))[:, keep])) if keep.any() else 0.0
    tol = max(TOL_FACTOR * dist, FLOOR * float(np.max(np.abs(c['src'].astype(np.float64)))))
    return ref, y, keep, tol, 1.0 - float(keep.mean()), dist


def prefilter_tolerance(x):
    """(float64 reference, tolerance, float32 restatement's distance) of a prefilter input."""
    ref = prefilter_ref64(x)
    dist = float(np.max(np.abs(prefilter_f32(x).astype(np.float64) - ref)))
    return ref, max(TOL_FACTOR * dist, FLOOR * float(np.max(np.abs(np.asarray(x, dtype=np.float64))))), dist


# ---- the band-limited analytic image ------------------------------------------------------------------------------------------------------
ANALYTIC = {'moving': (24, 40, 48), 'prepared': (12, 20, 24), 'fixed': (20, 30, 40),
            'fixed_frame': ((1.5, 1.0), (1.5, 0.5), (1.6, 1.0)), 'moving_frame': ((2.0, 0.5), (2.0, 0.25), (2.0, 0.5))}
_WAVES = ((0.07, 0.05, 0.11, 0.3), (0.13, -0.04, 0.06, 1.1), (-0.05, 0.12, 0.09, 2.0), (0.02, 0.03, -0.15, 0.7))       # cycles per voxel (D, H, W), phase


def analytic_image(y):
    """A sum of sinusoids at continuous moving-grid positions y [3][...]: at most 0.15 cycles per voxel, far below Nyquist."""
    return sum(np.sin(2 * np.pi * (a * y[0] + b * y[1] + c * y[2]) + ph) for a, b, c, ph in _WAVES) * 100.0


def analytic_field():
    """A known smooth field on ANALYTIC's prepared grid, [3][Dp][Hp][Wp] float32 normalised: 1.5 voxels of low-frequency sinusoids."""
    size = ANALYTIC['prepared']
    z, y, x = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in size], indexing='ij')
    vox = [1.5 * np.sin(np.pi * z) * np.cos(2 * np.pi * y + 0.3), 1.5 * np.cos(np.pi * x + 0.2) * np.sin(np.pi * y), 1.5 * np.sin(2 * np.pi * x) * np.cos(np.pi * z)]
    return np.stack([vox[ch] / ((size[2 - ch] - 1) / 2.0) for ch in range(3)]).astype(np.float32)
