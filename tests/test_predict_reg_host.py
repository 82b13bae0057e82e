"""Host side of the registration predictor (no GPU): frame_of on every step kind, the displacement-field files of lib/nifti.py, and
predict_reg.py's argument errors."""
import os

import numpy as np
import pytest


def test_frame_of_every_step_kind():
    from deepatlas_amd.lib.inference import frame_of
    rec = {'native_size': (10, 16, 12), 'native_spacing': (1.5, 0.75, 1.25), 'steps': []}
    assert frame_of(rec, (10, 16, 12)) == ((1.0, 0.0),) * 3
    rec['steps'] = [('resample', (10, 16, 12), (1.5, 0.75, 1.25), (1.0, 1.0, 1.0))]
    assert frame_of(rec, (13, 12, 18)) == ((1.0 / 1.25, 0.0), (1.0 / 0.75, 0.0), (1.0 / 1.5, 0.0))
    rec['steps'].append(('flip',))                                            # p -> 12 - p along D, then the resample
    assert frame_of(rec, (13, 12, 18)) == ((-1.0 / 1.25, (1.0 / 1.25) * 12.0), (1.0 / 0.75, 0.0), (1.0 / 1.5, 0.0))
    rec['steps'].append(('crop', (13, 12, 18), (2, 1, 3, 3, 3, 7)))           # p -> p + c first
    got = frame_of(rec, (8, 8, 8))
    assert got == ((-1.0 / 1.25, (1.0 / 1.25) * (12.0 - 2.0)), (1.0 / 0.75, (1.0 / 0.75) * 1.0), (1.0 / 1.5, (1.0 / 1.5) * 3.0))
    assert all(isinstance(v, np.float64) for pair in got for v in pair)
    with pytest.raises(ValueError):
        frame_of(rec, (8, 8, 9))                                              # does not lead back to the crop's size
    with pytest.raises(ValueError):
        frame_of(rec, (8, 8))


def test_prepare_is_shared():
    import predict_seg
    from deepatlas_amd.lib import inference
    assert callable(inference.prepare) and predict_seg.prepare.__doc__ and 'lib/inference.py' in predict_seg.prepare.__doc__


@pytest.mark.parametrize('ext', ['.nii', '.nii.gz'])
def test_field_file_round_trip(tmp_path, ext):
    from deepatlas_amd.lib.nifti import Volume, read_nifti, read_nifti_field, write_nifti, write_nifti_field
    rng = np.random.RandomState(0)
    arr = rng.standard_normal((3, 4, 5, 6)).astype(np.float32)
    affine = np.array([[0.5, 0, 0, -200.0], [0, 0.75, 0, 120.0], [0, 0, -2.0, 33.0], [0, 0, 0, 1.0]])
    like = Volume(np.zeros((4, 5, 6), np.int16), (0.5, 0.75, 2.0), affine, {})
    path = write_nifti_field(str(tmp_path / ('field' + ext)), arr, like=like)
    got = read_nifti_field(path)
    assert got.array.dtype == np.float32 and np.array_equal(got.array, arr) and got.spacing == like.spacing and np.array_equal(got.affine, affine)
    assert tuple(got.header['dim'][:6]) == (5, 6, 5, 4, 1, 3) and got.header['intent_code'] == 1007 and got.header['datatype'] == 16
    with pytest.raises(ValueError, match='every extent beyond the third must be 1'):
        read_nifti(path)                                                      # still one 3-D volume per file
    plain = write_nifti(str(tmp_path / ('plain' + ext)), arr[0], like=like)
    assert read_nifti(plain).header['intent_code'] == 0
    with pytest.raises(ValueError, match='not a displacement field'):
        read_nifti_field(plain)
    for bad in (arr[0], arr[:2], arr.astype(np.float64)):
        with pytest.raises(ValueError):
            write_nifti_field(str(tmp_path / ('bad' + ext)), bad, like=like)
    with pytest.raises(ValueError):
        write_nifti(str(tmp_path / ('bad' + ext)), arr)                       # write_nifti keeps refusing 4-D arrays


def test_field_file_truncated(tmp_path):
    from deepatlas_amd.lib.nifti import read_nifti_field, write_nifti_field
    path = write_nifti_field(str(tmp_path / 'f.nii'), np.zeros((3, 2, 2, 2), np.float32))
    with open(path, 'rb') as f:
        raw = f.read()
    with open(path, 'wb') as f:
        f.write(raw[:-8])
    with pytest.raises(ValueError, match='truncated'):
        read_nifti_field(path)


def _args(*argv):
    import predict_reg
    return predict_reg.build_parser().parse_args(['--ckpt', 'c', '--output-dir', 'o'] + list(argv))


def test_predict_reg_argument_errors(tmp_path):
    import predict_reg
    cfg = {'data': 'OAI'}
    assert _args().interp == 'bspline' and predict_reg.INTERP_ORDER == {'linear': 1, 'bspline': 3}
    with pytest.raises(SystemExit):
        _args('--interp', 'cubic')
    listing = str(tmp_path / 'pairs.txt')
    with open(listing, 'w') as f:
        f.write('a b\n\nc, d\n')
    for argv in ([], ['--moving', 'a.nii'], ['--fixed', 'a.nii'], ['--moving', 'a.nii', 'b.nii', '--fixed', 'c.nii'],
                 ['--moving', 'a.nii', '--fixed', 'b.nii', '--pair-list', listing, '--data-dir', 'd'], ['--pair-list', listing],
                 ['--moving', 'a.nii', '--fixed', 'b.nii', '--moving-labels', 'x.nii', 'y.nii'], ['--moving', 'a.nii', '--fixed', 'b.nii', '--fixed-labels', 'x.nii', 'y.nii'],
                 ['--moving', 'a.nii', '--fixed', 'b.nii', '--label-dir', 'l'], ['--pair-list', listing, '--data-dir', 'd', '--moving-labels', 'x.nii']):
        with pytest.raises(ValueError):
            predict_reg.resolve_pairs(_args(*argv), cfg)
    rows = predict_reg.resolve_pairs(_args('--pair-list', listing, '--data-dir', 'd', '--label-dir', 'l'), cfg)
    assert rows[0] == ('a_to_b', 'a', os.path.join('d', '', 'a_image.nii.gz'), 'b', os.path.join('d', '', 'b_image.nii.gz'),
                       os.path.join('l', '', 'a_masks.nii.gz'), os.path.join('l', '', 'b_masks.nii.gz')) and rows[1][0] == 'c_to_d'
    rows = predict_reg.resolve_pairs(_args('--moving', 'x/m_image.nii.gz', '--fixed', 'y/f.nii', '--moving-labels', 'lm.nii'), cfg)
    assert rows == [('m_to_f', 'm', 'x/m_image.nii.gz', 'f', 'y/f.nii', 'lm.nii', None)]
    for text in ('a\n', 'a b c\n', '\n'):
        with open(listing, 'w') as f:
            f.write(text)
        with pytest.raises(ValueError):
            predict_reg.read_pair_list(listing)
    with pytest.raises(ValueError, match='no config'):
        predict_reg.main(['--ckpt', str(tmp_path / 'none.pth.tar'), '--output-dir', str(tmp_path / 'o'), '--moving', 'a.nii', '--fixed', 'b.nii'])


def test_format_pair():
    import predict_reg
    jac = {'mean': 1.0, 'std': 0.25, 'folds': 3}
    assert predict_reg.format_pair('a_to_b', jac) == 'a_to_b: det J mean 1.0000 std 0.2500 folds 3'
    assert predict_reg.format_pair('a_to_b', jac, 0.5, 0.25) == 'a_to_b: Dice Avg: 0.500000 (identity 0.250000), det J mean 1.0000 std 0.2500 folds 3'
