"""CPU: registration evaluation and the registration / joint experiments, everything that needs no GPU -- the build compiles regeval.hip and
its entries resolve and refuse bad arguments before touching a device; the pairwise dataset enumerates the reference's order
(lib/datasets.py:344-359); train_reg / train_joint configs; the test oracles of tests/regeval_cases.py are self-consistent and the
GPU tests' inputs are conditioned the way their exclusion rule assumes."""
import argparse
import os

import numpy as np
import pytest
import torch

import regeval_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_compiles_regeval_and_symbols_resolve():
    import __graft_entry__ as ge
    assert 'regeval.hip' in ge.HIP_SOURCES
    ge.build()
    from deepatlas_amd import _native
    L = _native.lib()
    for name in ('da_warp_labels_nearest_counts', 'da_jacobian_det', 'da_jacobian_det_ws_bytes'):
        assert name in _native.SIGNATURES and hasattr(L, name), name
    assert L.da_jacobian_det_ws_bytes(2, 16, 16, 16) >= 2 * 5 * 8
    # the device code object of the new file is in the library (the kernels' names survive in the gfx950 code object's symbol table)
    blob = open(ge.LIB, 'rb').read()
    assert b'warp_nearest_counts_kernel' in blob and b'jacobian_det_kernel' in blob


def test_regeval_c_abi_rejects_bad_arguments_before_touching_the_device():
    from ctypes import c_void_p
    from deepatlas_amd import _native
    L = _native.lib()
    fake = c_void_p(0x1000)          # never dereferenced on the host
    BAD, SMALL = -1, -2
    warp = L.da_warp_labels_nearest_counts
    assert warp(None, 1, fake, 1, fake, 1, 8, 8, 8, 4, fake, fake, None) == BAD          # null moving labels
    assert warp(fake, 1, fake, 1, None, 1, 8, 8, 8, 4, fake, fake, None) == BAD          # null displacement
    assert warp(fake, 1, fake, 1, fake, 1, 8, 8, 8, 4, None, None, None) == BAD          # neither output
    assert warp(fake, 1, None, 1, fake, 1, 8, 8, 8, 4, fake, None, None) == BAD          # counts without target labels
    assert warp(fake, 4, fake, 1, fake, 1, 8, 8, 8, 4, fake, None, None) == BAD          # label_bytes 4
    assert warp(fake, 1, fake, 2, fake, 1, 8, 8, 8, 4, fake, None, None) == BAD
    assert warp(fake, 1, fake, 1, fake, 1, 8, 8, 8, 0, fake, None, None) == BAD          # C = 0 with counts
    for dims in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0)):
        assert warp(fake, 1, fake, 1, fake, dims[0], dims[1], dims[2], dims[3], 4, fake, fake, None) == BAD
    jac = L.da_jacobian_det
    need = L.da_jacobian_det_ws_bytes(1, 8, 8, 8)
    assert need > 0
    assert jac(None, 1, 8, 8, 8, fake, None, fake, need, None) == BAD                    # null field
    assert jac(fake, 1, 8, 8, 8, None, None, fake, need, None) == BAD                    # null statistics
    assert jac(fake, 1, 8, 8, 8, fake, None, None, need, None) == BAD                    # null workspace
    for dims in ((0, 8, 8, 8), (1, 1, 8, 8), (1, 8, 1, 8), (1, 8, 8, 1)):                # every extent >= 2
        assert jac(fake, dims[0], dims[1], dims[2], dims[3], fake, None, fake, need, None) == BAD
    assert jac(fake, 1, 8, 8, 8, fake, None, fake, need - 1, None) == SMALL


def test_new_ops_fail_loudly_on_cpu_tensors():
    from deepatlas_amd import ops, _native
    lab = torch.zeros((1, 4, 4, 4), dtype=torch.uint8)
    disp = torch.zeros((1, 3, 4, 4, 4))
    with pytest.raises(_native.NativeError):
        ops.warp_labels_nearest(lab, disp)
    with pytest.raises(_native.NativeError):
        ops.reg_label_counts(lab, lab, disp, 4)
    with pytest.raises(_native.NativeError):
        ops.jacobian_det(disp)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_pair_enumeration_is_the_references(n):
    from deepatlas_amd.lib.datasets import SyntheticRegDataset, get_reg_dataset
    assert get_reg_dataset('synthetic') is SyntheticRegDataset
    ds = SyntheticRegDataset(n, (4, 4, 4), 4, seed=1)
    assert len(ds) == n * (n - 1)
    want = []
    for i in range(n * (n - 1)):                      # lib/datasets.py:350-353
        fixed_ind, moving_ind = i // (n - 1), i % (n - 1)
        if moving_ind >= fixed_ind:
            moving_ind += 1
        want.append((moving_ind, fixed_ind))
    assert ds.pairs == want
    assert len(set(ds.pairs)) == n * (n - 1) and all(m != f for m, f in ds.pairs)
    assert set(ds.pairs) == {(m, f) for m in range(n) for f in range(n) if m != f}
    im, it, sm, st_, has, name = ds[0]
    m, f = ds.pairs[0]
    assert torch.equal(im, ds.seg[m][0]) and torch.equal(it, ds.seg[f][0]) and torch.equal(sm, ds.seg[m][1]) and torch.equal(st_, ds.seg[f][1])
    assert has is True and name == 'synthetic_%d_to_synthetic_%d' % (m, f)


def test_pair_enumeration_with_a_labelled_subset():
    from deepatlas_amd.lib.datasets import SyntheticRegDataset, get_reg_dataset
    n, labeled = 5, [1, 3]
    ds = SyntheticRegDataset(n, (4, 4, 4), 4, seed=1, labeled=labeled)
    full = SyntheticRegDataset(n, (4, 4, 4), 4, seed=1)
    assert ds.pairs == [p for p in full.pairs if p[1] in labeled]            # exactly the pairs with a labelled fixed volume, same order
    assert len(ds) == len(labeled) * (n - 1)
    flags = [ds[i][4] for i in range(len(ds))]
    assert flags == [m in labeled for m, _ in ds.pairs] and True in flags and False in flags
    for i, (m, f) in enumerate(ds.pairs):
        sample = ds[i]
        assert torch.equal(sample[3], full.seg[f][1])
        if m in labeled:
            assert torch.equal(sample[2], full.seg[m][1])
        else:
            assert int(sample[2].max()) == 0                                  # placeholder; the flag says so
    from torch.utils.data import DataLoader
    batch = next(iter(DataLoader(ds, batch_size=2, shuffle=False)))          # default collation works (no None in the sample)
    assert batch[4].dtype == torch.bool and batch[4].tolist() == flags[:2]
    with pytest.raises(KeyError):
        get_reg_dataset('nope')
    with pytest.raises(ValueError):
        SyntheticRegDataset(1, (4, 4, 4), 4)


def _ns(**kw):
    base = dict(device='0', debug=False, num_samples=4, num_epochs=3, lr=1e-3, test_only=False, data_root='./data', log_root='./logs',
                shape=[16, 16, 32])
    base.update(kw)
    return argparse.Namespace(**base)


def test_train_reg_build_config():
    import train_reg
    c = train_reg.build_config(_ns())
    for k in ('debug_mode', 'resume_dir', 'random_seed', 'data', 'n_epochs', 'samples_per_epoch', 'batch_size', 'print_batch_period', 'valid_epoch_period',
              'save_ckpts_epoch_period', 'model', 'n_classes', 'lambda_reg', 'learning_rate', 'lr_mode', 'milestones', 'gamma', 'synthetic_shape',
              'data_dir', 'log_dir', 'device', 'num_samples'):
        assert k in c, k
    assert c['model'] == 'voxel_morph_cvpr' and c['lambda_reg'] == 1.0 and c['random_seed'] == 230 and c['batch_size'] == 1
    assert c['samples_per_epoch'] == 12 and c['synthetic_shape'] == (16, 16, 32) and c['device'] == 'cuda:0' and 'matrix_precision' not in c
    assert train_reg.build_config(_ns(lambda_reg=0.25, matrix_precision='fp32'))['lambda_reg'] == 0.25
    assert train_reg.build_config(_ns(matrix_precision='fp32'))['matrix_precision'] == 'fp32'
    from deepatlas_amd.models.registration import RegistrationExperiment
    name = RegistrationExperiment.experiment_name(c)
    assert name.startswith('Reg_voxel_morph_cvpr_synthetic_4samples') and name.endswith('_scheduler_multiStep')


def test_train_joint_build_config():
    import train_joint
    c = train_joint.build_config(_ns())
    for k in ('resume_dir', 'seg_resume_dir', 'reg_resume_dir', 'model', 'model_settings', 'reg_model', 'n_classes', 'lambda_sim', 'lambda_reg',
              'lambda_anat', 'lambda_sp', 'num_labeled', 'learning_rate', 'lr_mode', 'synthetic_shape', 'log_dir', 'device'):
        assert k in c, k
    assert (c['lambda_sim'], c['lambda_reg'], c['lambda_anat'], c['lambda_sp']) == (1.0, 1.0, 1.0, 1.0)
    assert c['model'] == 'UNet_light' and c['reg_model'] == 'voxel_morph_cvpr' and c['num_labeled'] == 4
    assert c['seg_resume_dir'] == '' and c['reg_resume_dir'] == ''
    assert train_joint.build_config(_ns(num_labeled=2))['num_labeled'] == 2
    assert train_joint.build_config(_ns(num_labeled=99))['num_labeled'] == 4                # clamped to the number of volumes
    assert train_joint.build_config(_ns(num_labeled=-3))['num_labeled'] == 0
    c2 = train_joint.build_config(_ns(seg_ckpt='a.pth.tar', reg_ckpt='b.pth.tar', lambda_anat=0.5))
    assert c2['seg_resume_dir'] == 'a.pth.tar' and c2['reg_resume_dir'] == 'b.pth.tar' and c2['lambda_anat'] == 0.5 and 'seg_ckpt' not in c2
    from deepatlas_amd.models.deepatlas import DeepAtlasExperiment
    sub = DeepAtlasExperiment.labeled_subset(6, 2, 230)
    assert len(sub) == 2 and sub == DeepAtlasExperiment.labeled_subset(6, 2, 230) and set(sub) <= set(range(6))
    assert DeepAtlasExperiment.labeled_subset(6, 9, 230) == list(range(6))
    with pytest.raises(ValueError):
        DeepAtlasExperiment(train_joint.build_config(_ns(num_labeled=0)))


# ---- the oracles of regeval_cases.py are self-consistent (numpy / torch-CPU fp64) ---------------------------------------------
def test_oracle_nearest_warp_with_zero_displacement_is_the_identity():
    for shape in ((5, 6, 7), (8, 3, 9)):
        lab = rc.random_labels(shape, 2, torch.int64, seed=3)
        out, excluded = rc.nearest_oracle(lab, torch.zeros((2, 3) + shape))
        assert torch.equal(out, lab)
        assert not bool(excluded.any())


def test_oracle_nearest_warp_of_an_integer_translation_is_a_shift():
    shape = (6, 7, 8)
    lab = rc.random_labels(shape, 1, torch.int64, seed=4)
    u = torch.zeros((1, 3) + shape, dtype=torch.float64)
    u[:, 0] = 2.0; u[:, 1] = -1.0; u[:, 2] = 3.0                  # target (d, h, w) reads moving (d + 3, h - 1, w + 2)
    out, _ = rc.nearest_oracle(lab, rc.to_normalised(u).float())
    want = torch.zeros_like(lab)
    want[:, :3, 1:, :6] = lab[:, 3:, :6, 2:]
    assert torch.equal(out, want)


def test_oracle_jacobian_of_affine_and_zero_fields():
    shape = (6, 9, 7)
    det = rc.jacobian_np(torch.zeros((2, 3) + shape))
    assert det.shape == (2,) + shape and np.all(det == 1.0)
    rng = np.random.default_rng(0)
    for _ in range(3):
        A = rng.standard_normal((3, 3)) * 0.2
        u = rc.affine_field(shape, A).double()
        det = rc.jacobian_np(u)
        want = np.linalg.det(np.eye(3) + A)
        assert np.abs(det - want).max() < 1e-6 * max(1.0, abs(want))           # everywhere, faces / edges / corners included (the field is fp32-rounded)
    det64, bound, yard = rc.jacobian_bound(rc.smooth_field(shape, 1, 1.5, seed=1))
    assert 0 < yard < 1e-5 * np.abs(det64).max() and bound == 4 * yard


def test_counts_oracle_matches_a_direct_count():
    p = np.array([[0, 1, 1, 2, 7, 3]]); t = np.array([[0, 1, 2, 2, 7, 9]])
    c = rc.counts_np(p, t, 4)
    assert c[0, :, 0].tolist() == [1, 2, 1, 1] and c[0, :, 1].tolist() == [1, 1, 2, 0] and c[0, :, 2].tolist() == [1, 1, 1, 0]


@pytest.mark.parametrize('shape,n,sigma,dtype', rc.WARP_CASES, ids=rc.WARP_IDS)
def test_gpu_warp_inputs_are_conditioned_as_the_exclusion_rule_assumes(shape, n, sigma, dtype):
    """On the very inputs test_gpu_regeval.py uses: (1) the share of voxels within 1e-4 voxels of a rounding boundary is far below the 0.2 %
    cap (measured 4.5e-4 - 7.3e-4), so the cap cannot hide a wrong kernel; (2) torch's own fp32 CPU path differs from its fp64 path only
    inside that band, and on a handful of voxels -- an fp32 evaluation of the coordinate is good enough everywhere else."""
    disp = rc.smooth_field(shape, n, sigma, seed=11)
    lab = rc.random_labels(shape, n, dtype, seed=12)
    out64, excluded = rc.nearest_oracle(lab, disp)
    share = float(excluded.double().mean())
    print('excluded share %.3e' % share)
    assert share <= rc.MAX_EXCLUDED / 2
    out32, _ = rc.nearest_oracle(lab, disp, dtype=torch.float32)
    differ = out32 != out64
    print('fp32 path differs on %d voxels' % int(differ.sum()))
    assert not bool((differ & ~excluded).any())
    assert int(differ.sum()) <= 4 * n
    assert float((out64 == 0).double().mean()) < 0.5                    # the field stays mostly inside the volume: a real gather
