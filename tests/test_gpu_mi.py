"""GPU: the mutual-information kernels (mi.hip) against the float64 reference of tests/mi_cases.py, and the selectable similarity of the
registration and joint steps.  Every bound comes from mi_cases.bounds(): 4 x the float32 torch evaluation's own distance from float64,
floors 5e-7 (loss) and 2e-6 (gradient, max norm over the gradient's max)."""
import math

import pytest
import torch

import mi_cases as mc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def _loss_module(name):
    from deepatlas_amd.lib.loss import MutualInformationLoss
    _, _, bins, sr, (vmin, vmax), _, _ = mc.CASES[name]
    return MutualInformationLoss(num_bins=bins, sigma_ratio=sr, minval=vmin, maxval=vmax)


def _run(name, grad_x=True, grad_y=True):
    x, y = mc.inputs(name)
    x, y = x.to(dev()).requires_grad_(grad_x), y.to(dev()).requires_grad_(grad_y)
    loss = _loss_module(name)(x, y)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad, y.grad


@pytest.mark.parametrize('name', mc.IDS)
def test_mi_matches_the_float64_reference(name):
    loss, dx, dy = _run(name)
    l64, dx64, dy64 = mc.reference(name)
    lb, xb, yb = mc.bounds(name)
    x, _ = mc.inputs(name)
    assert dx.shape == x.shape and dy.shape == x.shape and dx.dtype == torch.float32
    dl = abs(float(loss) - l64)
    ex, ey = mc.rel_max(dx.cpu(), dx64), mc.rel_max(dy.cpu(), dy64)
    print('%s: loss %.9f (float64 %.9f) |d| %.2e (bound %.1e); dx %.2e (bound %.1e) dy %.2e (bound %.1e)' % (name, float(loss), l64, dl, lb, ex, xb, ey, yb))
    assert dl <= lb
    if name in mc.GRAD_CASES:
        assert ex <= xb and ey <= yb
    else:
        # one image constant: the gradient is a cancellation residue (float32 torch is 1 % - 6000 % off); finite and negligible
        ref_max = max(float(g.abs().max()) for g in mc.reference('tiny')[1:])
        for g in (dx, dy):
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) < 1e-3 * ref_max


@pytest.mark.parametrize('which', ['dx_only', 'dy_only'])
def test_mi_one_sided_gradient(which):
    gx = which == 'dx_only'
    loss, dx, dy = _run('ragged', grad_x=gx, grad_y=not gx)
    l64, dx64, dy64 = mc.reference('ragged')
    lb, xb, yb = mc.bounds('ragged')
    assert abs(float(loss) - l64) <= lb
    if gx:
        assert dy is None and mc.rel_max(dx.cpu(), dx64) <= xb
    else:
        assert dx is None and mc.rel_max(dy.cpu(), dy64) <= yb


@pytest.mark.parametrize('name', ['ragged', 'capped'])
def test_mi_is_bit_identical_from_run_to_run(name):
    a, b = _run(name), _run(name)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_mi_nan_poisons_the_loss_and_inf_is_clamped():
    from deepatlas_amd.lib.loss import MutualInformationLoss
    crit = MutualInformationLoss()
    x, y = mc.inputs('ragged')                               # N = 3
    x, y = x.to(dev()), y.to(dev())
    base = crit(x, y)
    xn = x.clone(); xn[1].view(-1)[100] = float('nan')
    assert math.isnan(float(crit(xn, y))) and math.isnan(float(crit(y, xn)))
    xi, xc = x.clone(), x.clone()
    xi[2].view(-1)[5], xi[0].view(-1)[692] = float('inf'), float('-inf')
    xc[2].view(-1)[5], xc[0].view(-1)[692] = 1.0, 0.0
    xi.requires_grad_(True)
    li = crit(xi, y)
    li.backward()
    assert torch.equal(li.detach(), crit(xc, y)) and not torch.equal(li.detach(), base)
    g = xi.grad
    assert bool(torch.isfinite(g).all()) and float(g[2].view(-1)[5]) == 0.0 and float(g[0].view(-1)[692]) == 0.0
    # values beyond the range: zero gradient there, non-zero inside
    xo, yo = mc.inputs('range5')
    xo = xo.to(dev()).requires_grad_(True)
    _loss_module('range5')(xo, yo.to(dev())).backward()
    out = (xo.detach() < -0.5) | (xo.detach() > 2.0)
    assert bool(out.any()) and bool((xo.grad[out] == 0).all()) and bool((xo.grad[~out] != 0).float().mean() > 0.99)


def test_mi_unsupported_arguments_raise_before_any_launch():
    from deepatlas_amd import _native as nat, ops
    x, y = mc.inputs('tiny')
    x, y = x.to(dev()).reshape(1, -1), y.to(dev()).reshape(1, -1)
    V = x.shape[1]
    loss = torch.full((1,), -7.0, device=dev())
    stats = torch.full((1, ops.MI_STATS_FLOATS), -7.0, device=dev())
    dx = torch.full_like(x, -7.0)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    gl = torch.ones(1, device=dev())
    for bins, vmin, vmax, sr in ((1, 0.0, 1.0, 1.0), (33, 0.0, 1.0, 1.0), (32, 1.0, 0.0, 1.0), (32, 0.5, 0.5, 1.0), (32, 0.0, 1.0, 0.0), (32, 0.0, 1.0, -1.0)):
        with pytest.raises(nat.NativeError):
            nat.call('da_mi_fwd', nat.ptr(x), nat.ptr(y), 1, V, bins, vmin, vmax, sr, nat.ptr(loss), nat.ptr(stats), nat.ptr(ws), ws.numel(), nat.stream())
        with pytest.raises(nat.NativeError):
            nat.call('da_mi_bwd', nat.ptr(x), nat.ptr(y), nat.ptr(stats), nat.ptr(gl), nat.ptr(dx), None, 1, V, bins, vmin, vmax, sr, nat.stream())
        with pytest.raises(nat.NativeError):
            ops.MIFn.apply(x, y, bins, sr, vmin, vmax)
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all()) and bool((stats == -7.0).all()) and bool((dx == -7.0).all())
    with pytest.raises(ValueError):
        ops.MIFn.apply(x, y[:, :-1])
    with pytest.raises(ValueError):
        ops.MIFn.apply(x.double(), y.double())
    with pytest.raises(ValueError):
        ops.MIFn.apply(x.reshape(1, 2, 3, 2, 5), y.reshape(1, 2, 3, 2, 5))          # two channels


def test_mi_is_smallest_at_zero_shift_of_a_folded_copy():
    """A smooth volume against its |2 x - 1| copy translated by s voxels: the loss has its minimum at s = 0 (tests/test_mi_reference.py
    shows the float64 reference has it, by a margin of > 0.1), and follows the reference at every shift."""
    from deepatlas_amd.lib.loss import MutualInformationLoss
    crit = MutualInformationLoss()
    vol = mc.shift_volume()
    got = {s: float(crit(vol.to(dev()), mc.shifted_fold(vol, s).to(dev()))) for s in mc.SHIFTS}
    want = {s: mc.evaluate(vol, mc.shifted_fold(vol, s), 32, 1.0, 0.0, 1.0, torch.float64)[0] for s in mc.SHIFTS}
    print(got)
    assert min(got, key=got.get) == 0 and got[0] < min(v for s, v in got.items() if s != 0) - 0.1
    for s in mc.SHIFTS:
        y = mc.shifted_fold(vol, s)
        d32 = abs(mc.evaluate(vol, y, 32, 1.0, 0.0, 1.0, torch.float32)[0] - want[s])          # the yardstick, as for the cases
        assert abs(got[s] - want[s]) <= max(mc.FACTOR * d32, mc.LOSS_FLOOR), (s, got[s], want[s], d32)


# ---- the steps -------------------------------------------------------------------------------------------------------------------------
SHAPE, C = (16, 16, 32), 8


def _nets():
    from oracle import nets
    from deepatlas_amd.lib.network_factory import get_network, unets
    spec = nets.UNET_TINY
    seg_sd = nets.closed_form_fill(nets.unet_param_shapes(1, C, spec['encoders'], spec['decoders']), seed=1)
    reg_sd = nets.closed_form_fill(nets.voxelmorph_param_shapes(), seed=4)
    seg = unets.UNet_generator(encoders=spec['encoders'], decoders=spec['decoders'], act='LeakyReLU')(in_channel=1, n_classes=C, bias=True, BN=True)
    seg.load_state_dict({k: v.clone() for k, v in seg_sd.items()}, strict=True)
    reg = get_network('voxel_morph_cvpr')()
    reg.load_state_dict({k: v.clone() for k, v in reg_sd.items()}, strict=True)
    return seg.to(dev()), reg.to(dev()), reg_sd


def _pair():
    """A fixed image and a moving image of the other 'modality' (fold remap), with label maps."""
    from oracle import nets
    from deepatlas_amd.lib.datasets import SyntheticRegDataset
    im_t = nets.closed_form_volume((1, 1) + SHAPE, seed=6).clamp(0, 1)
    im_m = SyntheticRegDataset.remap_intensity(nets.closed_form_volume((1, 1) + SHAPE, seed=5).clamp(0, 1), 'fold')
    sm, st_ = nets.closed_form_labels((1,) + SHAPE, C, seed=7), nets.closed_form_labels((1,) + SHAPE, C, seed=8)
    return im_m.to(dev()), im_t.to(dev()), sm.to(dev()), st_.to(dev())


@pytest.mark.parametrize('sim_loss,settings', [('mi', {}), ('mi', {'num_bins': 16, 'sigma_ratio': 0.5}), ('lncc', {})], ids=['mi', 'mi16', 'lncc'])
def test_registration_step_with_a_chosen_similarity(sim_loss, settings):
    from deepatlas_amd.models.joint import RegistrationStep, make_sim_loss
    from deepatlas_amd.optim import FlatAdam
    _, reg, _ = _nets()
    im_m, im_t, _, _ = _pair()
    opt = FlatAdam(reg.parameters(), lr=1e-3)
    before = opt.flat_p.detach().clone()
    step = RegistrationStep(reg, opt, sim_loss=sim_loss, sim_settings=settings)
    loss, (disp, warped, deform), (sim, bend) = step(im_m, im_t)
    torch.cuda.synchronize()
    again = make_sim_loss(sim_loss, settings).to(dev())(warped, im_t)
    assert torch.equal(sim, again.detach()), (float(sim), float(again))
    assert float(loss) == float(sim + bend)
    for t in (loss, disp, warped, sim, bend, opt.flat_p):
        assert bool(torch.isfinite(t).all())
    assert not torch.equal(before, opt.flat_p)
    if sim_loss == 'mi':
        assert float(sim) < 0.0                           # -MI of two structured images


def test_joint_step_with_mutual_information():
    from deepatlas_amd.models.joint import DeepAtlasJointStep
    from deepatlas_amd.lib.loss import MutualInformationLoss
    from deepatlas_amd.lib.network_factory import get_network
    from deepatlas_amd.optim import FlatAdam
    seg, reg, reg_sd = _nets()
    im_m, im_t, sm, st_ = _pair()
    so, ro = FlatAdam(seg.parameters(), lr=1e-3), FlatAdam(reg.parameters(), lr=1e-3)
    before = (so.flat_p.detach().clone(), ro.flat_p.detach().clone())
    step = DeepAtlasJointStep(seg, so, reg, ro, C, sim_loss='mi')
    r = step(im_m, im_t, sm, st_)
    torch.cuda.synchronize()
    # the step returns no warped image: it is formed again by a twin of the registration net in its state before the step
    twin = get_network('voxel_morph_cvpr')()
    twin.load_state_dict({k: v.clone() for k, v in reg_sd.items()}, strict=True)
    twin.to(dev()).train()
    with torch.no_grad():
        _, warped, _ = twin(im_m, im_t)
    want = MutualInformationLoss()(warped, im_t)
    assert abs(float(r['sim']) - float(want)) <= 1e-6, (float(r['sim']), float(want))
    for k, v in r.items():
        assert bool(torch.isfinite(v).all()), k
    assert float(r['sim']) < 0.0
    assert not torch.equal(before[0], so.flat_p) and not torch.equal(before[1], ro.flat_p)
    assert bool(torch.isfinite(so.flat_p).all()) and bool(torch.isfinite(ro.flat_p).all())
    # the pair whose fixed image is unlabelled takes the same similarity
    r2 = step(im_m, im_t, sm, None)
    torch.cuda.synchronize()
    assert float(r2['sim']) < 0.0 and all(bool(torch.isfinite(v).all()) for v in r2.values())


@pytest.mark.parametrize('which', ['reg', 'joint'])
def test_mi_step_replays_as_a_hip_graph(which):
    """The MI kernels use the workspace only (no allocation, no synchronisation): the step with sim_loss='mi' captured by graphs.GraphedStep
    trains like the eager one, bit for bit (deterministic mode for the warp's adjoint scatter)."""
    from deepatlas_amd import ops
    from deepatlas_amd.graphs import GraphedStep
    from deepatlas_amd.models.joint import DeepAtlasJointStep, RegistrationStep
    from deepatlas_amd.optim import FlatAdam
    prev = ops.set_deterministic(True)
    results = []
    try:
        for graph in (False, True):
            seg, reg, _ = _nets()
            im_m, im_t, sm, st_ = _pair()
            so, ro = FlatAdam(seg.parameters(), lr=1e-3), FlatAdam(reg.parameters(), lr=1e-3)
            if which == 'reg':
                segments, between, opts = RegistrationStep(reg, ro, sim_loss='mi').segments(im_m, im_t)
            else:
                segments, between, opts = DeepAtlasJointStep(seg, so, reg, ro, C, sim_loss='mi').segments(im_m, im_t, sm, st_)
            g = GraphedStep(segments, opts, between=between, warmup=1 if graph else 10 ** 9)
            sims = [float(g()['sim'].item()) for _ in range(4)]            # graphed: 1 eager, capture + replay, 2 replays
            assert (g.graphs is not None) == graph
            torch.cuda.synchronize()
            results.append((sims, torch.cat([o.flat_p.detach().cpu() for o in opts])))
            g.close()
    finally:
        ops.set_deterministic(prev)
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert all(math.isfinite(v) and v < 0.0 for v in results[0][0]) and len(set(results[0][0])) == 4
    assert torch.equal(results[0][1], results[1][1])
