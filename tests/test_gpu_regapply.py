"""regapply.hip on the device (da_bspline3_prefilter, da_warp_frames) through ops.bspline_prefilter / ops.warp_to_grid,
lib/inference.py's RegistrationPredictor and predict_reg.py end to end.  Cases, the float64 references, the float32 restatements, the
tolerance and the guard band: tests/regapply_cases.py (their CPU companion: tests/test_regapply_reference.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import regapply_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0) if torch.cuda.is_available() else None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def field(disp):
    """[3][D][H][W] numpy -> 1 x 3 x D x H x W on the device."""
    return dev(disp)[None]


def warp(src, disp, out_size, ff, mf, **kw):
    from deepatlas_amd import ops
    out = ops.warp_to_grid(dev(src), field(disp), out_size, ff, mf, **kw)
    return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()


# ---- 1. the prefilter -------------------------------------------------------------------------------------------------------------------
def check_prefilter(x):
    from deepatlas_amd import ops
    ref, tol, dist = rc.prefilter_tolerance(x)
    got = ops.bspline_prefilter(dev(x))
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(x.shape)
    err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - ref)))
    print('prefilter %s %s: kernel %.3g, float32 restatement %.3g, tolerance %.3g' % (x.shape, x.dtype, err, dist, tol))
    assert err <= tol
    return got


@pytest.mark.parametrize('shape', rc.prefilter_shapes(), ids=lambda s: 'x'.join(str(v) for v in s))
def test_prefilter_noise_every_shape(shape):
    x = np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32)
    a = check_prefilter(x)
    from deepatlas_amd import ops
    assert torch.equal(a, ops.bspline_prefilter(dev(x)))                      # bit-identical repeats


def test_prefilter_impulses_constant_int16_channels():
    shape = (5, 7, 67)
    for corner in np.ndindex(3, 3, 3):                                        # every face, edge and corner (and the centre)
        x = np.zeros(shape, dtype=np.float32)
        x[tuple((0, n // 2, n - 1)[c] for c, n in zip(corner, shape))] = 1.0
        check_prefilter(x)
    check_prefilter(np.full((3, 130, 9), 2.5, dtype=np.float32))
    check_prefilter(np.random.RandomState(5).randint(-3000, 3000, size=(3, 130, 9)).astype(np.int16))
    check_prefilter(np.random.RandomState(6).randint(0, 256, size=(2, 5, 7, 67)).astype(np.uint8))      # C = 2


def test_prefilter_single_axes_compose():
    """axes=(k,) filters one axis; the three in the kernel's order give the full prefilter's bits."""
    from deepatlas_amd import ops
    x = dev(np.random.RandomState(7).standard_normal((6, 70, 65)).astype(np.float32))
    step = ops.bspline_prefilter(ops.bspline_prefilter(ops.bspline_prefilter(x, axes=(2,)), axes=(1,)), axes=(0,))
    assert torch.equal(step, ops.bspline_prefilter(x))
    one = ops.bspline_prefilter(x, axes=(1,)).cpu().numpy()
    from scipy import ndimage
    ref = ndimage.spline_filter1d(x.cpu().numpy().astype(np.float64), 3, axis=1, mode='mirror')
    assert np.max(np.abs(one - ref)) <= rc.prefilter_tolerance(x.cpu().numpy())[1]


def test_interpolation_property():
    """Order 3 with a zero field and identity frames returns the source."""
    for shape in rc.RAGGED + ((1, 20, 33),):
        src = np.random.RandomState(8).standard_normal((1,) + shape).astype(np.float32)
        got = warp(src, np.zeros((3,) + tuple(max(n, 2) for n in shape), dtype=np.float32), shape, rc.IDENTITY, rc.IDENTITY, order=3)
        # the identity frame of an axis of extent 1 has a prepared extent of 2: position 0 either way
        ref, tol, dist = rc.prefilter_tolerance(src)
        # evaluating at the nodes sums three coefficients per axis with weights (1, 4, 1) / 6: the coefficients' error passes through unamplified
        assert np.max(np.abs(got - src)) <= tol


# ---- 2. the warp against the float64 reference -------------------------------------------------------------------------------------------
WARP_CASES = sorted(rc.warp_cases())


@pytest.mark.parametrize('name', WARP_CASES)
@pytest.mark.parametrize('order', [0, 1, 3])
def test_warp_against_reference(name, order):
    from deepatlas_amd import ops
    c = rc.build_case(name)
    ref, y, keep, tol, excluded, dist = rc.case_reference(name, order)
    assert excluded <= rc.GUARD_CAP
    dflt = rc.default_of(c['dtype'])
    got = warp(c['src'], c['disp'], c['fixed'], c['fixed_frame'], c['moving_frame'], order=order, default=dflt)
    assert got.shape == ref.shape and got.dtype == (c['src'].dtype if order == 0 else np.float32)
    err = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64))[:, keep]))
    print('%s order %d: kernel %.3g, float32 restatement %.3g, tolerance %.3g' % (name, order, err, dist, tol))
    assert err <= tol
    again = warp(c['src'], c['disp'], c['fixed'], c['fixed_frame'], c['moving_frame'], order=order, default=dflt)
    assert np.array_equal(got, again, equal_nan=True)
    if order == 3:                                                            # prefiltered=True takes the coefficients as they are
        coef = ops.bspline_prefilter(dev(c['src']))
        pre = ops.warp_to_grid(coef, field(c['disp']), c['fixed'], c['fixed_frame'], c['moving_frame'], order=3, default=dflt, prefiltered=True)
        assert np.array_equal(pre.cpu().numpy(), got)


# ---- 3. exact cases ---------------------------------------------------------------------------------------------------------------------
# extents 2^k + 1: (size - 1) / 2 is a power of two, so the normalised coordinate of a node, its way back and a whole-voxel displacement are
# exact in float32 and the sample position is the integer itself -- the premise of "bit for bit"
EXACT = (9, 17, 33)


@pytest.mark.parametrize('dtype', rc.DTYPES)
def test_zero_field_identity_is_the_source(dtype):
    src = rc.make_source(EXACT, dtype, 40, channels=2)
    zero = np.zeros((3,) + EXACT, dtype=np.float32)
    assert np.array_equal(warp(src, zero, EXACT, rc.IDENTITY, rc.IDENTITY, order=0, default=rc.default_of(dtype)), src)
    lin = warp(src, zero, EXACT, rc.IDENTITY, rc.IDENTITY, order=1, default=rc.DEFAULT)
    assert lin.dtype == np.float32 and np.array_equal(lin, src.astype(np.float32))


@pytest.mark.parametrize('shift', [(2, -3, 5), (-1, 4, 0)])
def test_whole_voxel_translation(shift):
    src = rc.make_source(EXACT, 'int16', 41)
    disp = np.stack([np.full(EXACT, shift[2 - ch] / ((EXACT[2 - ch] - 1) / 2.0), dtype=np.float32) for ch in range(3)])
    want = np.full(src.shape, rc.DEFAULT, dtype=np.int16)
    dst = tuple(slice(max(0, -s), min(n, n - s)) for s, n in zip(shift, EXACT))
    frm = tuple(slice(max(0, s), min(n, n + s)) for s, n in zip(shift, EXACT))
    want[(slice(None),) + dst] = src[(slice(None),) + frm]
    assert np.array_equal(warp(src, disp, EXACT, rc.IDENTITY, rc.IDENTITY, order=0, default=rc.DEFAULT), want)
    assert np.array_equal(warp(src, disp, EXACT, rc.IDENTITY, rc.IDENTITY, order=1, default=rc.DEFAULT), want.astype(np.float32))


def test_pure_resample_frame_is_resample_volume():
    from deepatlas_amd import ops
    c = rc.THREE
    src = rc.make_source(c['moving'], 'int16', 42)
    zero = np.zeros((3,) + c['prepared'], dtype=np.float32)
    ff, mf = ((1.3, 0.0), (0.9, 0.0), (1.0, 0.0)), ((0.8, 0.0), (1.1, 0.0), (1.43, 0.0))
    got = warp(src, zero, c['fixed'], ff, mf, order=0, default=rc.DEFAULT)
    want = ops.resample_volume(dev(src), c['fixed'], tuple(m[0] / f[0] for m, f in zip(mf, ff)), (0.0, 0.0, 0.0), 'nearest', rc.DEFAULT).cpu().numpy()
    _, y, _, _ = rc.warp_reference(src, zero, c['fixed'], ff, mf, 0)
    keep = ~rc.guard_mask(y, c['moving'], 0)
    assert keep.mean() >= 1 - rc.GUARD_CAP and np.array_equal(got[:, keep], want[:, keep]) and (got == rc.DEFAULT).any()


def test_identity_frames_linear_is_warpfn():
    """Where all eight taps of the warp lie inside, border and zeros padding agree: ops.WarpFn within the case's tolerance."""
    from deepatlas_amd import ops
    name = 'ragged0_amp2'
    c = rc.build_case(name)
    ref, y, keep, tol, _, _ = rc.case_reference(name, 1)
    src = c['src'].astype(np.float32)
    got = warp(src, c['disp'], c['fixed'], rc.IDENTITY, rc.IDENTITY, order=1, default=0)
    wf = ops.WarpFn.apply(dev(src)[None], field(c['disp']))[0].cpu().numpy()[0]
    inner = keep & np.all([(y[a] >= 0) & (y[a] <= c['moving'][a] - 1) for a in range(3)], axis=0)
    assert inner.mean() > 0.3
    # WarpFn forms its coordinate from identity + disp in normalised float32 units: the float32 restatement's kind of rounding
    assert np.max(np.abs(got - wf)[:, inner]) <= tol


# ---- 4. non-finite field voxels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_non_finite_field_voxel_marks_its_own_taps(bad):
    """The field taps of an output voxel are, per axis, floor(r) and floor(r) + 1 where that is below the extent, r = the prepared index clamped
    to the grid.  A voxel within 1e-4 of a node (the frame keeps all but a few off them) may read either neighbour: it must hold the clean
    value or the mark, every other voxel exactly what the rule says."""
    c = dict(rc.build_case('three_amp0.3'))
    ff = ((1.0 / 0.7, 0.3), (1.0, 0.37), (1.25, 0.45))
    disp = c['disp'].copy()
    at = (3, 7, 11)
    disp[1][at] = bad
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in c['fixed']], indexing='ij')
    hit, unsure = np.ones(c['fixed'], dtype=bool), np.zeros(c['fixed'], dtype=bool)
    for a in range(3):
        n = c['prepared'][a]
        p = (grids[a] - ff[a][1]) / ff[a][0]
        lo = np.floor(np.clip(p, 0, n - 1)).astype(int)
        hit &= (lo == at[a]) | ((lo + 1 == at[a]) & (lo + 1 < n))
        unsure |= (np.abs(p - np.round(p)) < 1e-4) & (p > -1e-4) & (p < n - 1 + 1e-4)
    sure = ~unsure
    assert (hit & sure).sum() >= 8 and unsure.mean() <= rc.GUARD_CAP
    src_f = c['src'].astype(np.float32)
    clean_f = warp(src_f, c['disp'], c['fixed'], ff, c['moving_frame'], order=1, default=rc.DEFAULT)[0]
    got_f = warp(src_f, disp, c['fixed'], ff, c['moving_frame'], order=1, default=rc.DEFAULT)[0]
    assert not np.isnan(clean_f).any()
    assert np.array_equal(np.isnan(got_f)[sure], hit[sure]) and np.array_equal(got_f[~hit & sure], clean_f[~hit & sure])
    assert (np.isnan(got_f[unsure]) | (got_f[unsure] == clean_f[unsure])).all()
    cub = warp(src_f, disp, c['fixed'], ff, c['moving_frame'], order=3, default=rc.DEFAULT)[0]
    assert np.array_equal(np.isnan(cub)[sure], hit[sure])
    clean_i = warp(c['src'], c['disp'], c['fixed'], ff, c['moving_frame'], order=0, default=rc.DEFAULT)[0]
    got_i = warp(c['src'], disp, c['fixed'], ff, c['moving_frame'], order=0, default=rc.DEFAULT)[0]
    assert got_i.dtype == c['src'].dtype and (got_i[hit & sure] == rc.DEFAULT).all() and np.array_equal(got_i[~hit & sure], clean_i[~hit & sure])
    assert ((got_i[unsure] == rc.DEFAULT) | (got_i[unsure] == clean_i[unsure])).all()


# ---- 5. the world displacement ----------------------------------------------------------------------------------------------------------
def test_world_displacement():
    """Frames and a field that are exact in float32 (extents 2^k + 1, displacements in quarter voxels, scales 0.5 and 2, integer crop offsets):
    y is exact in double, so what is measured is the affine part.  Bound per voxel: 4 x float32 rounding (2^-24) of |d(x)|, plus the double
    evaluation's own rounding, 64 x 2^-53 x the largest world coordinate (six products and sums of magnitudes up to that)."""
    prepared, fixed, moving = EXACT, (12, 30, 20), (20, 16, 70)
    ff, mf = ((1.0, 2.0), (2.0, -1.0), (0.5, 3.0)), ((2.0, 1.0), (-1.0, 15.0), (2.0, 4.0))
    disp = np.stack([np.full(prepared, q / ((prepared[2 - ch] - 1) / 2.0), dtype=np.float32) for ch, q in enumerate((1.25, -0.5, 0.75))])
    A_f = np.array([[0.7, 0.0, 0.0, -200.0], [0.0, -0.8, 0.0, 200.0], [0.0, 0.0, 2.5, 150.0], [0, 0, 0, 1]])
    A_m = np.array([[0.31, 0.0, 0.0, 200.0], [0.0, 1.1, 0.0, -200.0], [0.0, 0.0, -1.3, -120.0], [0, 0, 0, 1]])
    src = rc.make_source(moving, 'float32', 43)
    out, world = warp(src, disp, fixed, ff, mf, order=1, default=0, world=(A_f, A_m))
    y = rc.sample_positions(disp, fixed, ff, mf)
    want = rc.world_reference(y, A_f, A_m)
    assert world.shape == (3,) + fixed and world.dtype == np.float32
    mag = np.sqrt((want ** 2).sum(0))
    big = max(np.abs(A_f[:3]).sum(1).max() * max(fixed), np.abs(A_m[:3]).sum(1).max() * max(moving), 200.0)
    bound = 4 * 2.0 ** -24 * mag + 64 * 2.0 ** -53 * big
    err = np.abs(world.astype(np.float64) - want).max(0)
    print('world displacement: largest error %.3g mm at |d| up to %.1f mm' % (err.max(), mag.max()))
    assert (err <= bound).all() and mag.max() > 300


# ---- 6. the band-limited analytic image through RegistrationPredictor ----------------------------------------------------------------------
class KnownField(torch.nn.Module):
    """Stand-in for a registration net: returns exactly the field it was given."""

    def __init__(self, disp):
        super(KnownField, self).__init__()
        self.disp = disp

    def forward(self, moving, fixed):
        return self.disp, None, None


def test_analytic_image_each_order():
    from deepatlas_amd.lib.inference import RegistrationPredictor
    a = rc.ANALYTIC
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in a['moving']], indexing='ij'))
    src = rc.analytic_image(grid)[None].astype(np.float32)
    disp = rc.analytic_field()
    predictor = RegistrationPredictor(KnownField(field(disp)))
    got_field = predictor.field(torch.zeros((1,) + a['prepared'], device=DEV), torch.zeros((1,) + a['prepared'], device=DEV))
    assert torch.equal(got_field, field(disp))
    errs = {}
    from deepatlas_amd import ops
    for order in (0, 1, 3):
        got = ops.warp_to_grid(dev(src), got_field, a['fixed'], a['fixed_frame'], a['moving_frame'], order=order, default=0).cpu().numpy()
        s64 = rc.prefilter_ref64(src) if order == 3 else src
        ref, y, inside, finite = rc.warp_reference(s64, disp, a['fixed'], a['fixed_frame'], a['moving_frame'], order, default=0)
        s32 = rc.prefilter_f32(src) if order == 3 else src
        low = rc.warp_reference(s32, disp, a['fixed'], a['fixed_frame'], a['moving_frame'], order, default=0, dtype=np.float32)[0]
        core = inside & ~rc.guard_mask(y, a['moving'], order) & np.all([(y[k] >= 4) & (y[k] <= a['moving'][k] - 5) for k in range(3)], axis=0)
        truth = rc.analytic_image(y)
        tol = max(rc.TOL_FACTOR * float(np.max(np.abs(low.astype(np.float64) - ref)[0][core])), rc.FLOOR * float(np.abs(src).max()))
        ref_err = float(np.max(np.abs(ref[0] - truth)[core]))
        errs[order] = float(np.max(np.abs(got[0] - truth)[core]))
        print('analytic image order %d: kernel %.4g from the analytic values, reference %.4g, tolerance %.3g' % (order, errs[order], ref_err, tol))
        assert errs[order] <= ref_err + tol
    assert errs[3] < errs[1] < errs[0]


def test_predictor_apply_uses_the_records():
    """apply() = warp_to_grid with frame_of's frames: records with a resample, a flip and a crop."""
    from deepatlas_amd import ops
    from deepatlas_amd.lib.inference import RegistrationPredictor, frame_of
    from deepatlas_amd.lib.nifti import Volume
    rec_m = {'native_size': (10, 16, 12), 'native_spacing': (1.5, 0.75, 1.25),
             'steps': [('resample', (10, 16, 12), (1.5, 0.75, 1.25), (1.0, 1.0, 1.0)), ('flip',), ('crop', (13, 12, 18), (2, 1, 3, 3, 3, 7))]}
    rec_f = {'native_size': (9, 9, 9), 'native_spacing': (1.0, 1.0, 1.0), 'steps': [('crop', (9, 9, 9), (1, 0, 1, 0, 1, 0))]}
    src = rc.make_source(rec_m['native_size'], 'int16', 44)[0]
    disp = field(rc.make_field((8, 8, 8), 1.0, 45))
    vm = Volume(src, rec_m['native_spacing'], np.diag([1.5, 0.75, 1.25, 1.0]), {})
    vf = Volume(np.zeros((9, 9, 9), np.int16), (1, 1, 1), np.eye(4), {})
    got, world = RegistrationPredictor(KnownField(disp)).apply(dev(src), disp, vf, rec_f, vm, rec_m, order=3, world=True)
    want, w2 = ops.warp_to_grid(dev(src), disp, (9, 9, 9), frame_of(rec_f, (8, 8, 8)), frame_of(rec_m, (8, 8, 8)), order=3, world=(vf.affine, vm.affine))
    assert torch.equal(got, want) and torch.equal(world, w2) and tuple(got.shape) == (9, 9, 9)


def test_argument_errors_before_any_launch():
    from deepatlas_amd import ops
    src, disp = dev(np.zeros((4, 4, 4), np.int16)), torch.zeros((1, 3, 4, 4, 4), device=DEV)
    I = rc.IDENTITY
    for kw in (dict(order=2), dict(order=0, default=1e6), dict(order=0, default=0.5), dict(prefiltered=True), dict(world=(np.eye(4),)), dict(world=(np.eye(2), np.eye(4)))):
        with pytest.raises(ValueError):
            ops.warp_to_grid(src, disp, (4, 4, 4), I, I, **kw)
    for args in ((src, disp[:, :2], (4, 4, 4), I, I), (src, disp.double(), (4, 4, 4), I, I), (src, disp, (4, 4), I, I), (src, disp, (4, 4, 0), I, I),
                 (src, disp, (4, 4, 4), ((0.0, 0.0),) * 3, I), (src, disp, (4, 4, 4), I, ((1.0, np.nan),) * 3), (src, disp, (4, 4, 4), I, I[:2]),
                 (src.long(), disp, (4, 4, 4), I, I), (src, disp[:, :, :1], (4, 4, 4), I, I)):
        with pytest.raises(ValueError):
            ops.warp_to_grid(*args)
    with pytest.raises(ValueError):
        ops.bspline_prefilter(src, axes=(3,))
    with pytest.raises(ValueError):
        ops.bspline_prefilter(src.long())


# ---- 7. predict_reg.py end to end -------------------------------------------------------------------------------------------------------
# prepared at 1 mm: both files 18 x 18 x 34, cropped by one voxel per side to 16 x 16 x 32 (the registration smoke's shape); every spacing and product is exact
SCANS = {'kneeLEFT0': ((12, 24, 17), (2.0, 0.75, 1.5), (-90.0, 120.0, -60.0)), 'kneeRIGHT1': ((9, 18, 68), (0.5, 1.0, 2.0), (75.0, -110.0, 40.0))}
N_CLASS = 4


def write_pair_files(root):
    from deepatlas_amd.lib.nifti import write_nifti
    os.makedirs(str(root), exist_ok=True)
    for k, (name, (shape, spacing, origin)) in enumerate(sorted(SCANS.items())):
        z, y, x = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing='ij')
        lab = (1 + (x > 0.1 * k) + (y > -0.2)) * ((x ** 2 + y ** 2 + z ** 2) < 0.8)
        img = (lab * 200 + 50 * np.sin(3 * x + k) * np.cos(2 * y) + np.random.RandomState(k).uniform(0, 40, size=shape)).astype(np.int16)
        affine = np.diag(list(spacing) + [1.0])
        affine[:3, 3] = origin
        write_nifti(os.path.join(str(root), name + '_image.nii.gz'), img, spacing=spacing, affine=affine)
        write_nifti(os.path.join(str(root), name + '_masks.nii.gz'), lab.astype(np.uint8), spacing=spacing, affine=affine)
    listing = os.path.join(str(root), 'pairs.txt')
    with open(listing, 'w') as f:
        f.write('kneeLEFT0 kneeRIGHT1\nkneeRIGHT1, kneeLEFT0\n')
    return listing


def write_checkpoint(folder, extra=None):
    from deepatlas_amd.lib.network_factory import get_network
    os.makedirs(str(folder), exist_ok=True)
    torch.manual_seed(3)
    model = get_network('voxel_morph_cvpr')()
    model.weights_init()
    ckpt = os.path.join(str(folder), 'checkpoint.pth.tar')
    torch.save({'epoch': 0, 'model_state_dict': model.state_dict(), 'best_score': 0.0}, ckpt)
    cfg = {'data': 'OAI', 'model': 'voxel_morph_cvpr', 'model_settings': {}, 'n_classes': N_CLASS, 'crop_size': [1, 1, 1],
           'preprocess': [['resample', {'voxel_size': [1.0, 1.0, 1.0]}], ['percentile_rescale', {'lo': 0.5, 'hi': 99.5}], ['left_to_right', {}]]}
    cfg.update(extra or {})
    with open(os.path.join(str(folder), 'train_config.json'), 'w') as f:
        json.dump(cfg, f)
    return ckpt


def run_script(argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'predict_reg.py')] + argv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          universal_newlines=True, timeout=240)


def test_predict_reg_end_to_end(tmp_path):
    import predict_reg
    from deepatlas_amd.lib.nifti import read_nifti, read_nifti_field
    root = tmp_path / 'scans'
    listing = write_pair_files(root)
    ckpt = write_checkpoint(tmp_path / 'ckpt')
    out_dir = tmp_path / 'out'
    run = run_script(['--ckpt', ckpt, '--output-dir', str(out_dir), '--data-dir', str(root), '--pair-list', listing, '--label-dir', str(root), '--save-field'])
    assert run.returncode == 0, run.stdout
    lines = run.stdout.splitlines()
    dices = []
    for m, f in (('kneeLEFT0', 'kneeRIGHT1'), ('kneeRIGHT1', 'kneeLEFT0')):
        stem = os.path.join(str(out_dir), '%s_to_%s' % (m, f))
        fixed = read_nifti(os.path.join(str(root), f + '_image.nii.gz'))
        moving = read_nifti(os.path.join(str(root), m + '_image.nii.gz'))
        warped, seg, fld = read_nifti(stem + '_warped.nii.gz'), read_nifti(stem + '_seg.nii.gz'), read_nifti_field(stem + '_field.nii.gz')
        for got, dtype in ((warped, np.float32), (seg, np.uint8)):
            assert got.array.shape == fixed.array.shape and got.array.dtype == dtype and got.spacing == fixed.spacing and np.array_equal(got.affine, fixed.affine)
        assert fld.array.shape == (3,) + fixed.array.shape and fld.array.dtype == np.float32 and np.array_equal(fld.affine, fixed.affine)
        assert fld.header['dim'][0] == 5 and tuple(fld.header['dim'][1:6]) == tuple(reversed(fixed.array.shape)) + (1, 3) and fld.header['intent_code'] == 1007
        assert np.isfinite(fld.array).all() and np.abs(fld.array).max() > 1.0
        # the warped file from the field file: y = A_m^-1 (d + A_f (x, 1)), the numpy reference's cubic interpolation of the moving file
        x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in fixed.array.shape], indexing='ij')
        world = [fixed.affine[r, 0] * x[2] + fixed.affine[r, 1] * x[1] + fixed.affine[r, 2] * x[0] + fixed.affine[r, 3] + fld.array[r].astype(np.float64) for r in range(3)]
        inv = np.linalg.inv(moving.affine)
        ijk = [inv[r, 0] * world[0] + inv[r, 1] * world[1] + inv[r, 2] * world[2] + inv[r, 3] for r in range(3)]
        y = np.stack([ijk[2], ijk[1], ijk[0]])
        n = moving.array.shape
        src = moving.array[None]
        keep = ~rc.guard_mask(y, n, 3)
        inside = np.all([(y[a] >= -0.5) & (y[a] < n[a] - 0.5) for a in range(3)], axis=0)
        ys = np.where(inside[None], y, 0)
        ref = np.where(inside, rc.interpolate(rc.prefilter_ref64(src), ys, 3)[0], 0.0)
        low = np.where(inside, rc.interpolate(rc.prefilter_f32(src), ys.astype(np.float32), 3, np.float32)[0], 0.0)
        # positions come back through a float32 field: |world coordinate| <= 256 mm rounds by 2^-24 x 256 mm, over a spacing of at least 0.5 mm,
        # on three axes; an intensity moves by at most the largest difference of neighbouring voxels per voxel of position (x 1.5: cubic overshoot)
        steep = max(float(np.abs(np.diff(moving.array.astype(np.float64), axis=a)).max()) for a in range(3))
        tol = rc.TOL_FACTOR * float(np.max(np.abs(low - ref)[keep])) + 1.5 * steep * 3 * (2.0 ** -24 * 256 / 0.5) + rc.FLOOR * float(np.abs(src).max())
        err = float(np.max(np.abs(warped.array - ref)[keep]))
        print('%s: warped file %.3g from the reference through the field file, tolerance %.3g' % (stem, err, tol))
        assert keep.mean() >= 1 - rc.GUARD_CAP and inside.mean() > 0.5 and err <= tol
        truth = read_nifti(os.path.join(str(root), f + '_masks.nii.gz')).array
        dices.append(predict_reg.native_dice(dev(seg.array), dev(truth), N_CLASS))
        line = [l for l in lines if l.startswith('%s_to_%s: ' % (m, f))]
        assert len(line) == 1 and line[0].startswith('%s_to_%s: Dice Avg: %.6f (identity ' % (m, f, dices[-1])) and 'det J mean' in line[0] and 'folds' in line[0]
    assert any(l.startswith('mean over 2 pairs: Dice Avg: %.6f (identity ' % float(np.nanmean(dices))) for l in lines)


def test_predict_reg_affine_init_and_files(tmp_path):
    """A config with affine_init: the run completes, one composed field; --moving / --fixed with --interp linear and no labels."""
    from deepatlas_amd.lib.nifti import read_nifti
    root = tmp_path / 'scans'
    write_pair_files(root)
    ckpt = write_checkpoint(tmp_path / 'ckpt', {'affine_init': 'rigid', 'affine_settings': {'levels': [2, 1], 'iters': [3, 3]}})
    out_dir = tmp_path / 'out'
    image = lambda n: os.path.join(str(root), n + '_image.nii.gz')
    run = run_script(['--ckpt', ckpt, '--output-dir', str(out_dir), '--moving', image('kneeLEFT0'), '--fixed', image('kneeRIGHT1'), '--interp', 'linear', '--save-field'])
    assert run.returncode == 0, run.stdout
    assert [l for l in run.stdout.splitlines() if l.startswith('kneeLEFT0_to_kneeRIGHT1: det J mean')]
    got = read_nifti(os.path.join(str(out_dir), 'kneeLEFT0_to_kneeRIGHT1_warped.nii.gz'))
    assert got.array.shape == (9, 18, 68) and np.isfinite(got.array).all() and got.array.std() > 0
    assert sorted(os.listdir(str(out_dir))) == ['kneeLEFT0_to_kneeRIGHT1_field.nii.gz', 'kneeLEFT0_to_kneeRIGHT1_warped.nii.gz']


def test_predict_reg_refuses_unequal_prepared_shapes(tmp_path):
    """Without the common resample the two prepared shapes differ: nifti_data.check_shapes' ValueError."""
    import predict_reg
    from deepatlas_amd.lib.inference import prepare
    from deepatlas_amd.models import nifti_data
    root = tmp_path / 'scans'
    write_pair_files(root)
    cfg = {'data': 'OAI', 'model': 'voxel_morph_cvpr', 'preprocess': []}
    a = prepare(os.path.join(str(root), 'kneeLEFT0_image.nii.gz'), 'kneeLEFT0', cfg)[1]
    b = prepare(os.path.join(str(root), 'kneeRIGHT1_image.nii.gz'), 'kneeRIGHT1', cfg)[1]
    with pytest.raises(ValueError, match='do not share one shape'):
        nifti_data.check_shapes([[(a, None, 'kneeLEFT0'), (b, None, 'kneeRIGHT1')]], [cfg['model']])
    ckpt = write_checkpoint(tmp_path / 'ckpt', {'preprocess': [], 'crop_size': None})
    run = run_script(['--ckpt', ckpt, '--output-dir', str(tmp_path / 'out'), '--data-dir', str(root), '--pair-list', os.path.join(str(root), 'pairs.txt')])
    assert run.returncode != 0 and 'do not share one shape' in run.stdout
