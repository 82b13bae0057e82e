"""CPU companion of tests/test_gpu_regapply.py: the float64 restatement of da_warp_frames against scipy, its inside rule against
ops.resample_axis_table, frame_of against what RecordedPreprocess did, the guard band's cap on every case, and the measured distances of the
float32 restatements (printed with -s; DESIGN.md 4.34 records them)."""
import numpy as np
import pytest
from scipy import ndimage

import regapply_cases as rc


def test_grid_rule():
    n = rc.second_trip_voxels()
    assert n == 256 * 16 * 256 + 1 and int(np.prod(rc.warp_cases()['second_trip']['fixed'])) >= n


def test_mirror_is_scipys():
    for n in (1, 2, 3, 7):
        x = np.arange(n, dtype=np.float64) * 3 + 1
        idx = np.arange(-3 * n - 2, 3 * n + 3)
        want = np.pad(x, (40, 40), mode='reflect')[idx + 40] if n > 1 else np.full(idx.shape, x[0])
        assert np.array_equal(x[rc.mirror(idx, n)], want)


@pytest.mark.parametrize('shape', [(5, 7, 9), (1, 6, 2), (3, 1, 200)])
def test_prefilter_f32_restatement(shape):
    x = np.random.RandomState(1).standard_normal(shape)
    ref, tol, dist = rc.prefilter_tolerance(x)
    print('prefilter %s: float32 restatement %.3g from scipy, tolerance %.3g' % (shape, dist, tol))
    assert dist < 1e-5 * np.abs(ref).max()
    # the same recursion in float64 is scipy's filter to rounding: the restated formulas are the right ones
    f64 = ref.copy()
    z = rc.POLE
    c = x.astype(np.float64)
    for axis in range(3):
        n = c.shape[axis]
        if n == 1:
            continue
        v = np.moveaxis(c, axis, 0)
        cp = np.empty_like(v)
        cp[0] = 6 * sum(z ** k * v[m] for k, m in enumerate(rc.mirror(np.arange(60), n)))
        for k in range(1, n):
            cp[k] = 6 * v[k] + z * cp[k - 1]
        out = np.empty_like(v)
        out[n - 1] = z / (z * z - 1) * (cp[n - 1] + z * cp[n - 2])
        for k in range(n - 2, -1, -1):
            out[k] = z * (out[k + 1] - cp[k])
        c = np.moveaxis(out, 0, axis)
    assert np.max(np.abs(c - f64)) < 1e-12 * np.abs(f64).max()


@pytest.mark.parametrize('order', [0, 1, 3])
def test_interpolation_equals_map_coordinates(order):
    """Inside points of a 5 x 7 x 9 volume: the restated step 6 is scipy's map_coordinates (mirror boundaries at order 3, edge-clamped taps =
    'nearest' at orders 0 and 1)."""
    rng = np.random.RandomState(2)
    src = rng.standard_normal((1, 5, 7, 9))
    y = np.stack([rng.uniform(-0.5, n - 0.5, 200) for n in src.shape[1:]])
    if order == 0:
        y = y[:, np.all(np.abs(y - np.floor(y) - 0.5) > 1e-6, axis=0)]
    coef = rc.prefilter_ref64(src) if order == 3 else src
    got = rc.interpolate(coef, y, order)[0]
    want = ndimage.map_coordinates(src[0], y, order=order, mode='mirror' if order == 3 else 'nearest')
    assert np.max(np.abs(got - want)) < 1e-13


def test_zero_field_is_resample_axis_table():
    """With a zero field the warp is an axis-aligned resample: scale a_m / a_f, offset b_m - a_m b_f / a_f; inside and the nearest / linear
    taps are ops.resample_axis_table's."""
    from deepatlas_amd import ops
    c = dict(rc.THREE, moving_frame=((-0.7, 6.5), (1.0, 6.0), (0.4, 12.0)))          # H: y = x + 5 leaves the 20 rows of the moving grid
    src = rc.make_source(c['moving'], 'int16', 3)
    zero = np.zeros((3,) + c['prepared'], dtype=np.float32)
    tabs = {}
    for interp in ('nearest', 'linear'):
        tabs[interp] = [ops.resample_axis_table(c['moving'][a], c['fixed'][a], c['moving_frame'][a][0] / c['fixed_frame'][a][0],
                                                c['moving_frame'][a][1] - c['moving_frame'][a][0] * c['fixed_frame'][a][1] / c['fixed_frame'][a][0], interp)
                        for a in range(3)]
    for order, interp in ((0, 'nearest'), (1, 'linear')):
        out, y, inside, finite = rc.warp_reference(src, zero, c['fixed'], c['fixed_frame'], c['moving_frame'], order)
        t = tabs[interp]
        keep = ~rc.guard_mask(y, c['moving'], order)
        ins = t[0][3][:, None, None] & t[1][3][None, :, None] & t[2][3][None, None, :]
        assert finite.all() and np.array_equal(ins[keep], inside[keep]) and inside.any() and not inside.all()
        lo = src[0][t[0][0][:, None, None], t[1][0][None, :, None], t[2][0][None, None, :]]
        if order == 0:
            want = np.where(ins, lo, rc.DEFAULT)
            assert np.array_equal(out[0][keep], want[keep])
        else:
            s = src[0].astype(np.float64)
            f = [t[a][2].astype(np.float64) for a in range(3)]
            g = lambda iz, iy, ix: s[t[0][iz][:, None, None], t[1][iy][None, :, None], t[2][ix][None, None, :]]
            fz, fy, fx = f[0][:, None, None], f[1][None, :, None], f[2][None, None, :]
            rows = [[g(iz, iy, 0) + fx * (g(iz, iy, 1) - g(iz, iy, 0)) for iy in (0, 1)] for iz in (0, 1)]
            planes = [rows[iz][0] + fy * (rows[iz][1] - rows[iz][0]) for iz in (0, 1)]
            want = np.where(ins, planes[0] + fz * (planes[1] - planes[0]), rc.DEFAULT)
            assert np.max(np.abs(out[0] - want)[keep]) < 1e-3          # (the table's fraction is float32)


@pytest.mark.parametrize('name', sorted(rc.warp_cases()))
def test_cases_stay_within_the_guard_cap(name):
    for order in (0, 1, 3):
        ref, y, keep, tol, excluded, dist = rc.case_reference(name, order)
        print('%s order %d: float32 restatement %.3g from the reference, tolerance %.3g, %.2f %% in the guard band' % (name, order, dist, tol, 100 * excluded))
        assert excluded <= rc.GUARD_CAP and keep.any()
    c = rc.build_case(name)
    if name == 'push_third_out':
        inside = rc.warp_reference(c['src'], c['disp'], c['fixed'], c['fixed_frame'], c['moving_frame'], 1)[2]
        assert 0.2 < 1.0 - inside.mean() < 0.6


def test_analytic_image_cubic_beats_linear():
    """The reference's own interpolation error on the band-limited image: cubic below linear, which the GPU test relies on."""
    a = rc.ANALYTIC
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in a['moving']], indexing='ij'))
    src = rc.analytic_image(grid)[None].astype(np.float32)
    disp = rc.analytic_field()
    errs = {}
    for order in (1, 3):
        s = rc.prefilter_ref64(src) if order == 3 else src
        out, y, inside, finite = rc.warp_reference(s, disp, a['fixed'], a['fixed_frame'], a['moving_frame'], order)
        # away from the faces, where the mirror extension is not the image's own continuation
        core = inside & np.all([(y[k] >= 4) & (y[k] <= a['moving'][k] - 5) for k in range(3)], axis=0)
        assert core.mean() > 0.3
        errs[order] = float(np.max(np.abs(out[0] - rc.analytic_image(y))[core]))
    print('analytic image: reference error linear %.3g, cubic %.3g (amplitude 400)' % (errs[1], errs[3]))
    assert errs[3] < 0.25 * errs[1]


def _record_cases():
    yield {'native_size': (10, 16, 12), 'native_spacing': (1.5, 0.75, 1.25), 'steps': []}, (10, 16, 12)
    yield {'native_size': (10, 16, 12), 'native_spacing': (1.5, 0.75, 1.25),
           'steps': [('resample', (10, 16, 12), (1.5, 0.75, 1.25), (1.0, 1.0, 1.0)), ('flip',)]}, (13, 12, 18)
    yield {'native_size': (10, 16, 12), 'native_spacing': (1.5, 0.75, 1.25),
           'steps': [('resample', (10, 16, 12), (1.5, 0.75, 1.25), (1.0, 1.0, 1.0)), ('flip',), ('crop', (13, 12, 18), (2, 1, 3, 3, 3, 7))]}, (8, 8, 8)
    yield {'native_size': (9, 9, 9), 'native_spacing': (1.0, 1.0, 1.0), 'steps': [('flip',), ('crop', (9, 9, 9), (1, 0, 2, 0, 1, 0)), ('flip',)]}, (8, 8, 7)


@pytest.mark.parametrize('k', range(4))
def test_frame_of_inverts_the_record(k):
    """Integer round trips: a volume holding its own native index, pushed through the record's steps on the host (nearest neighbour), reads at
    prepared index p the native index round(a p + b) wherever that lies inside."""
    from deepatlas_amd.lib.inference import frame_of
    record, prepared = list(_record_cases())[k]
    frame = frame_of(record, prepared)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in record['native_size']], indexing='ij')).astype(np.float64)
    cur = idx
    for step in record['steps']:
        if step[0] == 'flip':
            cur = cur[:, ::-1]
        elif step[0] == 'crop':
            c = step[2]
            cur = cur[:, c[0]:cur.shape[1] - c[3], c[1]:cur.shape[2] - c[4], c[2]:cur.shape[3] - c[5]]
        else:
            _, before, sp_b, sp_a = step
            size = tuple(int(np.floor(before[a] * sp_b[2 - a] / sp_a[2 - a] + 0.5)) for a in range(3))
            take = [np.clip(np.floor(np.arange(size[a]) * sp_a[2 - a] / sp_b[2 - a] + 0.5).astype(int), 0, before[a] - 1) for a in range(3)]
            cur = cur[:, take[0][:, None, None], take[1][None, :, None], take[2][None, None, :]]
    assert cur.shape[1:] == tuple(prepared)
    for a in range(3):
        p = np.arange(prepared[a], dtype=np.float64)
        n = frame[a][0] * p + frame[a][1]
        assert isinstance(frame[a][0], np.float64) and isinstance(frame[a][1], np.float64)
        want = np.clip(np.floor(n + 0.5), 0, record['native_size'][a] - 1)
        got = np.moveaxis(cur[a], a, 0).reshape(prepared[a], -1)[:, 0]
        tie = np.abs(n - np.floor(n) - 0.5) < 1e-9
        assert np.array_equal(got[~tie], want[~tie])
    assert (frame[0][0] < 0) == (sum(1 for s in record['steps'] if s[0] == 'flip') % 2 == 1)


def test_frame_of_refuses_a_record_that_does_not_fit():
    from deepatlas_amd.lib.inference import frame_of
    record = {'native_size': (10, 16, 12), 'native_spacing': (1, 1, 1), 'steps': [('crop', (10, 16, 11), (1, 1, 1, 1, 1, 1))]}
    with pytest.raises(ValueError):
        frame_of(record, (8, 14, 9))
    with pytest.raises(ValueError):
        frame_of({'native_size': (4, 4, 4), 'native_spacing': (1, 1, 1), 'steps': [('shear',)]}, (4, 4, 4))
