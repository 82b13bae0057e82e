"""CPU: mutual-information similarity, everything that needs no GPU -- the loss is registered, the three C entries are declared, built and
refuse bad arguments before touching a device; the selectable similarity and the moving-image remap reach the configs and leave the defaults
exactly as they were; and the cases of tests/mi_cases.py are what test_gpu_mi.py assumes: guard band kept, float32 distances as recorded,
the analytic backward pass the kernels implement equal to autograd, the shift property true of the float64 reference."""
import argparse
import os

import pytest
import torch

import mi_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ns(**kw):
    base = dict(device='0', debug=False, num_samples=4, num_epochs=3, lr=1e-3, test_only=False, data_root='./data', log_root='./logs',
                shape=[16, 16, 32])
    base.update(kw)
    return argparse.Namespace(**base)


# ---- registry, C ABI -----------------------------------------------------------------------------------------------------------------
def test_mi_is_in_the_loss_registry():
    from deepatlas_amd.lib.loss import get_loss_function, get_available_losses, get_extension_losses, loss_dict, MutualInformationLoss
    assert loss_dict['mi'] is MutualInformationLoss and get_loss_function('mi') is MutualInformationLoss
    assert get_extension_losses() == ['mi'] and 'mi' not in get_available_losses()            # (that list stays the reference's registry)
    with pytest.raises(KeyError):
        get_loss_function('nmi')
    m = get_loss_function('mi')()
    assert (m.num_bins, m.sigma_ratio, m.minval, m.maxval) == (32, 1.0, 0.0, 1.0)
    for bad in (dict(num_bins=1), dict(num_bins=33), dict(minval=1.0, maxval=1.0), dict(minval=2.0, maxval=1.0), dict(sigma_ratio=0.0),
                dict(sigma_ratio=-1.0)):
        with pytest.raises(ValueError):
            MutualInformationLoss(**bad)


def test_mi_entries_are_declared_and_built():
    import __graft_entry__ as ge
    assert 'mi.hip' in ge.HIP_SOURCES
    ge.build()
    from deepatlas_amd import _native, ops
    L = _native.lib()
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    for name in ('da_mi_ws_bytes', 'da_mi_fwd', 'da_mi_bwd'):
        assert name + '(' in header, name
        assert name in _native.SIGNATURES and hasattr(L, name), name
    assert '#define DA_MI_STATS_FLOATS %d' % ops.MI_STATS_FLOATS in header
    blob = open(ge.LIB, 'rb').read()
    for kernel in (b'mi_partial_kernel', b'mi_reduce_kernel', b'mi_finalize_kernel', b'mi_bwd_kernel'):
        assert kernel in blob, kernel


def test_mi_c_abi_rejects_bad_arguments_before_touching_the_device():
    from ctypes import c_void_p
    from deepatlas_amd import _native
    L = _native.lib()
    fake = c_void_p(0x1000)          # never dereferenced on the host
    BAD, SMALL = -1, -2
    need = L.da_mi_ws_bytes(2, 1000, 32)
    assert need >= 2 * 1024 * 8 * 2                                   # at least one double partial and one sum per sample
    assert L.da_mi_ws_bytes(2, 1000, 1) == 0 and L.da_mi_ws_bytes(2, 1000, 33) == 0 and L.da_mi_ws_bytes(0, 1000, 32) == 0
    assert L.da_mi_ws_bytes(1, 0, 32) == 0
    fwd, bwd = L.da_mi_fwd, L.da_mi_bwd
    ok = (2, 1000, 32, 0.0, 1.0, 1.0)
    for args in ((2, 1000, 1, 0.0, 1.0, 1.0), (2, 1000, 33, 0.0, 1.0, 1.0), (2, 1000, 32, 1.0, 1.0, 1.0), (2, 1000, 32, 1.0, 0.0, 1.0),
                 (2, 1000, 32, 0.0, 1.0, 0.0), (2, 1000, 32, 0.0, 1.0, -0.5), (2, 1000, 32, 0.0, float('inf'), 1.0),
                 (2, 1000, 32, float('nan'), 1.0, 1.0), (2, 1000, 32, 0.0, 1.0, float('nan')), (0, 1000, 32, 0.0, 1.0, 1.0),
                 (2, 0, 32, 0.0, 1.0, 1.0)):
        assert fwd(fake, fake, *args, fake, fake, fake, 1 << 30, None) == BAD, args
        assert bwd(fake, fake, fake, fake, fake, fake, *args, None) == BAD, args
    assert fwd(None, fake, *ok, fake, fake, fake, need, None) == BAD
    assert fwd(fake, None, *ok, fake, fake, fake, need, None) == BAD
    assert fwd(fake, fake, *ok, None, fake, fake, need, None) == BAD                 # null loss
    assert fwd(fake, fake, *ok, fake, None, fake, need, None) == BAD                 # null stats
    assert fwd(fake, fake, *ok, fake, fake, None, need, None) == BAD                 # null workspace
    assert fwd(fake, fake, *ok, fake, fake, fake, need - 1, None) == SMALL
    assert bwd(fake, fake, None, fake, fake, fake, *ok, None) == BAD                 # null stats
    assert bwd(fake, fake, fake, None, fake, fake, *ok, None) == BAD                 # null dloss
    assert bwd(fake, fake, fake, fake, None, None, *ok, None) == 0                   # no gradient asked for: nothing to do, nothing launched


def test_mi_op_fails_loudly_on_cpu_tensors_and_wrong_shapes():
    from deepatlas_amd import _native, ops
    x = torch.rand(1, 1, 4, 4, 4)
    with pytest.raises(_native.NativeError):
        ops.MIFn.apply(x, x)
    with pytest.raises(_native.NativeError):
        ops.MIFn.apply(x.reshape(1, -1), x.reshape(1, -1))


# ---- selectable similarity, remapped moving image ------------------------------------------------------------------------------------
def test_sim_loss_and_moving_remap_reach_the_configs():
    import train_reg
    import train_joint
    from deepatlas_amd.models.registration import RegistrationExperiment, check_sim_loss
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    # a Namespace without the new attributes (what every earlier caller builds): the defaults
    for mod in (train_reg, train_joint):
        c = mod.build_config(_ns())
        assert c['sim_loss'] == 'ncc' and c['sim_settings'] == {} and 'moving_remap' not in c and 'mi_bins' not in c
        assert check_sim_loss(c) == ('ncc', {})
    # the flags parse and arrive
    args = train_reg.add_common_arguments(argparse.ArgumentParser()).parse_args(['--sim-loss', 'mi', '--mi-bins', '16', '--moving-remap', 'fold'])
    assert (args.sim_loss, args.mi_bins, args.moving_remap) == ('mi', 16, 'fold')
    for mod in (train_reg, train_joint):
        c = mod.build_config(args)
        assert c['sim_loss'] == 'mi' and c['sim_settings'] == {'num_bins': 16} and c['moving_remap'] == 'fold' and 'mi_bins' not in c
        assert check_sim_loss(c) == ('mi', {'num_bins': 16})
    args = train_reg.add_common_arguments(argparse.ArgumentParser()).parse_args(['--sim-loss', 'lncc', '--mi-bins', '16', '--moving-remap', 'invert'])
    c = train_reg.build_config(args)
    assert c['sim_loss'] == 'lncc' and c['sim_settings'] == {} and c['moving_remap'] == 'invert'        # --mi-bins belongs to 'mi' only
    args = train_reg.add_common_arguments(argparse.ArgumentParser()).parse_args([])
    assert (args.sim_loss, args.mi_bins, args.moving_remap) == ('ncc', None, None)
    with pytest.raises(SystemExit):
        train_reg.add_common_arguments(argparse.ArgumentParser()).parse_args(['--sim-loss', 'nope'])
    with pytest.raises(SystemExit):
        train_reg.add_common_arguments(argparse.ArgumentParser()).parse_args(['--moving-remap', 'nope'])
    # names: the default keeps today's, a choice shows
    c0 = train_reg.build_config(_ns())
    assert RegistrationExperiment.experiment_name(c0) == 'Reg_voxel_morph_cvpr_synthetic_4samples_batch_1_3epochs_ncc_bending_1.0_lr_0.001_scheduler_multiStep'
    c1 = train_reg.build_config(_ns(sim_loss='mi', moving_remap='fold'))
    assert RegistrationExperiment.experiment_name(c1) == 'Reg_voxel_morph_cvpr_synthetic_4samples_batch_1_3epochs_mi_bending_1.0_lr_0.001_scheduler_multiStep_movingfold'
    legacy = {k: v for k, v in c0.items() if k not in ('sim_loss', 'sim_settings')}                      # a config written before the keys existed
    assert RegistrationExperiment.experiment_name(legacy) == RegistrationExperiment.experiment_name(c0)
    j0, j1 = train_joint.build_config(_ns()), train_joint.build_config(_ns(sim_loss='mi', moving_remap='invert'))
    name0 = DeepAtlasExperiment.experiment_name(j0)
    assert name0 == 'Joint_UNet_light_voxel_morph_cvpr_synthetic_4samples_4labeled_3epochs_sim1.0_reg1.0_anat1.0_sp1.0_lr_0.001_scheduler_multiStep'
    assert DeepAtlasExperiment.experiment_name(j1) == name0 + '_mi_movinginvert'


def test_unknown_sim_loss_raises():
    import train_reg
    import train_joint
    from deepatlas_amd.models.joint import RegistrationStep, DeepAtlasJointStep, make_sim_loss, SIM_LOSSES
    from deepatlas_amd.models.registration import RegistrationExperiment
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    from deepatlas_amd.lib.loss import NormalizedCrossCorrelationLoss, VoxelMorphLNCC, MutualInformationLoss
    assert SIM_LOSSES == {'ncc': NormalizedCrossCorrelationLoss, 'lncc': VoxelMorphLNCC, 'mi': MutualInformationLoss}
    assert type(make_sim_loss()) is NormalizedCrossCorrelationLoss                              # the default constructs what was constructed before
    assert type(make_sim_loss('lncc')) is VoxelMorphLNCC and make_sim_loss('lncc', {'filter_size': 5}).filter_size == 5
    mi = make_sim_loss('mi', {'num_bins': 16, 'sigma_ratio': 0.5})
    assert type(mi) is MutualInformationLoss and (mi.num_bins, mi.sigma_ratio) == (16, 0.5)
    with pytest.raises(ValueError):
        make_sim_loss('nope')
    with pytest.raises(ValueError):
        RegistrationStep(None, None, sim_loss='nope')
    with pytest.raises(ValueError):
        DeepAtlasJointStep(None, None, None, None, 8, sim_loss='nope')
    with pytest.raises(ValueError):
        RegistrationExperiment(train_reg.build_config(_ns(sim_loss='nope')))
    with pytest.raises(ValueError):
        DeepAtlasExperiment(train_joint.build_config(_ns(sim_loss='nope')))
    assert type(RegistrationStep(None, None).sim) is NormalizedCrossCorrelationLoss
    assert type(DeepAtlasJointStep(None, None, None, None, 8).sim) is NormalizedCrossCorrelationLoss


def test_moving_remap_touches_the_moving_image_only():
    from deepatlas_amd.lib.datasets import SyntheticRegDataset, SyntheticSegDataset
    shape, C, n = (6, 8, 10), 4, 3
    vols = SyntheticSegDataset(n, shape, C, seed=230)
    plain = SyntheticRegDataset(n, shape, C, seed=230)
    none = SyntheticRegDataset(n, shape, C, seed=230, moving_remap=None)
    inv = SyntheticRegDataset(n, shape, C, seed=230, moving_remap='invert')
    fold = SyntheticRegDataset(n, shape, C, seed=230, moving_remap='fold', labeled=[0, 2], pairs='all')
    assert len(plain) == len(none) == len(inv) == n * (n - 1)
    for i, (m, f) in enumerate(plain.pairs):
        a, b, c = plain[i], none[i], inv[i]
        # default and None: the samples of before, bit for bit (the volumes of the SyntheticSegDataset, untouched)
        assert torch.equal(a[0], vols[m][0]) and torch.equal(a[1], vols[f][0]) and torch.equal(a[2], vols[m][1]) and torch.equal(a[3], vols[f][1])
        for u, v in zip(a[:4], b[:4]):
            assert torch.equal(u, v)
        assert a[4:] == b[4:]
        assert torch.equal(c[0], 1.0 - vols[m][0]) and torch.equal(c[1], vols[f][0])
        assert torch.equal(c[2], a[2]) and torch.equal(c[3], a[3]) and c[4:] == a[4:]
    for i, (m, f) in enumerate(fold.pairs):
        s = fold[i]
        assert torch.equal(s[0], (2.0 * vols[m][0] - 1.0).abs()) and torch.equal(s[1], vols[f][0]) and len(s) == 7
        assert float(s[0].min()) >= 0.0 and float(s[0].max()) <= 1.0
    with pytest.raises(ValueError):
        SyntheticRegDataset(n, shape, C, moving_remap='nope')


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', mc.IDS)
def test_cases_keep_the_guard_band_and_cover_what_they_name(name):
    N, shape, bins, sr, (vmin, vmax), kind, branch = mc.CASES[name]
    x, y = mc.inputs(name)
    assert x.dtype == torch.float32 and x.shape == y.shape and x.shape[0] == N and branch
    assert x.dim() == (5 if len(shape) == 3 else 2)
    assert not bool(mc.in_guard_band(x, vmin, vmax).any()) and not bool(mc.in_guard_band(y, vmin, vmax).any())
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    if kind == 'outside':
        for t in (x, y):
            assert bool((t < vmin - mc.GUARD).any()) and bool((t > vmax + mc.GUARD).any())
    else:
        assert bool(((x > vmin) & (x < vmax)).all())           # (the related pairs' noise may carry a few y beyond an end: allowed, never in the band)
    if kind == 'constant':
        assert float(x.max()) == float(x.min())


def test_cases_cover_the_launcher():
    V = {k: int(torch.tensor(c[1]).prod()) for k, c in mc.CASES.items()}
    tiles = {k: -(-v // 256) for k, v in V.items()}
    assert V['tiny'] < 256 and V['ragged'] % 4 != 0 and V['ragged'] % 256 != 0 and mc.CASES['ragged'][0] == 3
    assert V['aligned'] % 256 == 0 and mc.CASES['aligned'][0] == 2 and tiles['aligned'] >= 4           # several workgroups, two tiles each
    assert (tiles['capped'] + 1) // 2 > 512 and tiles['capped'] / 512 > 4 and V['capped'] < 1 << 20      # above the cap, past the flush period
    assert {c[2] for c in mc.CASES.values()} >= {32, 16, 5} and {c[3] for c in mc.CASES.values()} >= {0.5, 1.0}
    assert any(c[4] != (0.0, 1.0) for c in mc.CASES.values()) and any(len(c[1]) == 1 for c in mc.CASES.values())
    assert {c[5] for c in mc.CASES.values()} >= {'related', 'independent', 'outside', 'constant'}


@pytest.mark.parametrize('name', mc.IDS)
def test_float32_distance_is_as_recorded(name):
    """The float32 torch evaluation against the float64 reference: re-measured here, it must itself fit the bound the kernels are given
    (4 x the recorded distance, or the floor) -- a recorded figure that were too small would fail this before it fails the kernels."""
    loss_d, dx_d, dy_d = mc.measure_fp32(name)
    lb, xb, yb = mc.bounds(name)
    print('%s: float32 loss %.2e dx %.2e dy %.2e (recorded %s)' % (name, loss_d, dx_d, dy_d, mc.FP32_DISTANCE[name]))
    assert loss_d <= lb
    if name in mc.GRAD_CASES:
        assert dx_d <= xb and dy_d <= yb
        assert mc.FP32_DISTANCE[name][1] <= 2e-6 and mc.FP32_DISTANCE[name][2] <= 2e-6      # the well-conditioned cases: a few ulp
    else:
        assert dx_d > 1e-3 or dy_d > 1e-3                                                   # ill-conditioned: why it is held on the loss only
        ref_max = max(float(g.abs().max()) for g in mc.reference('tiny')[1:])
        assert max(float(g.abs().max()) for g in mc.reference(name)[1:]) < 1e-3 * ref_max


def _analytic(x, y, bins, sr, vmin, vmax):
    """The backward pass as the kernels form it (float64): marginals as row / column sums of P, G, H, ga, gb, then per voxel."""
    N = x.shape[0]
    x, y = x.double().reshape(N, -1), y.double().reshape(N, -1)
    V = x.shape[1]
    c = torch.linspace(vmin, vmax, bins, dtype=torch.float64)
    p = 1.0 / (2.0 * ((vmax - vmin) / (bins - 1) * sr) ** 2)

    def weights(t):
        th = t.clamp(vmin, vmax)
        e = torch.exp(-p * (th.unsqueeze(-1) - c) ** 2)
        return e / e.sum(-1, keepdim=True), -2.0 * p * (th.unsqueeze(-1) - c), ((t > vmin) & (t < vmax)).double()
    wx, dxc, inx = weights(x)
    wy, dyc, iny = weights(y)
    P = torch.bmm(wx.transpose(1, 2), wy) / V
    a, b = P.sum(2), P.sum(1)
    Q = a.unsqueeze(2) * b.unsqueeze(1) + 1e-6
    R = P / Q + 1e-6
    mi = (P * torch.log(R)).sum((1, 2))
    G = torch.log(R) + P / (R * Q)
    H = -P * P / (R * Q * Q)
    ga, gb = torch.einsum('nij,nj->ni', H, b), torch.einsum('nij,ni->nj', H, a)
    ux = torch.einsum('nij,nvj->nvi', G, wy) + ga.unsqueeze(1)
    uy = torch.einsum('nij,nvi->nvj', G, wx) + gb.unsqueeze(1)
    gx = (wx * dxc * (ux - (wx * ux).sum(-1, keepdim=True))).sum(-1) / V * inx
    gy = (wy * dyc * (uy - (wy * uy).sum(-1, keepdim=True))).sum(-1) / V * iny
    return float(-mi.mean()), -gx / N, -gy / N


@pytest.mark.parametrize('name', [k for k in mc.IDS if k != 'capped'])
def test_analytic_backward_equals_autograd(name):
    _, _, bins, sr, (vmin, vmax), _, _ = mc.CASES[name]
    x, y = mc.inputs(name)
    loss, dx, dy = mc.reference(name)
    l2, gx, gy = _analytic(x, y, bins, sr, vmin, vmax)
    assert abs(l2 - loss) < 1e-12
    scale = max(float(dx.abs().max()), float(dy.abs().max()))
    assert float((gx - dx.reshape(gx.shape)).abs().max()) < 1e-9 * scale + 1e-16
    assert float((gy - dy.reshape(gy.shape)).abs().max()) < 1e-9 * scale + 1e-16


def test_reference_follows_nan_and_clamps_inf():
    x, y = mc.inputs('tiny')
    bins, sr, (vmin, vmax) = mc.CASES['tiny'][2], mc.CASES['tiny'][3], mc.CASES['tiny'][4]
    base = float(mc.mi_loss(x.double(), y.double(), bins, sr, vmin, vmax))
    xn = x.clone(); xn.view(-1)[7] = float('nan')
    assert torch.isnan(mc.mi_loss(xn.double(), y.double(), bins, sr, vmin, vmax))
    xi, xc = x.clone(), x.clone()
    xi.view(-1)[7], xi.view(-1)[9] = float('inf'), float('-inf')
    xc.view(-1)[7], xc.view(-1)[9] = vmax, vmin
    li = float(mc.mi_loss(xi.double(), y.double(), bins, sr, vmin, vmax))
    assert li == float(mc.mi_loss(xc.double(), y.double(), bins, sr, vmin, vmax)) and li != base


def test_reference_has_the_shift_property():
    """MI of a smooth volume against its 'fold'-remapped copy translated by s voxels is largest (the loss smallest) at s = 0, by a margin the
    kernels' tolerance cannot blur; NCC of the same pair is blind (|2 x - 1| is not a linear function of x)."""
    vol = mc.shift_volume()
    losses = {s: mc.evaluate(vol, mc.shifted_fold(vol, s), 32, 1.0, 0.0, 1.0, torch.float64)[0] for s in mc.SHIFTS}
    others = [v for s, v in losses.items() if s != 0]
    assert losses[0] < min(others) - 0.1, losses
    a, b = vol.double().reshape(-1), mc.shifted_fold(vol, 0).double().reshape(-1)
    ncc = float(((a - a.mean()) * (b - b.mean())).mean() / (a.std(unbiased=False) * b.std(unbiased=False)))
    assert abs(ncc) < 0.5, ncc
