"""CPU: the NIfTI-1 reader / writer (lib/nifti.py), the list-file and pairwise datasets (lib/datasets.py), the resample tables
(ops.resample_axis_table) and the host side of the preprocessing entry points (symbols, argument checks, command line).  No GPU; every file is
built in tmp_path."""
import argparse
import ctypes
import gzip
import math
import os
import re
import struct

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREPROCESS_SYMBOLS = ['da_resample_axes', 'da_volume_moments_ws_bytes', 'da_volume_moments', 'da_volume_percentiles_ws_bytes',
                      'da_volume_percentiles', 'da_affine_intensity_to_f32', 'da_label_lut']
# code -> numpy type character: the datatypes the issue lists
CODES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 256: 'i1', 512: 'u2', 768: 'u4', 1024: 'i8', 1280: 'u8'}


def raw_nifti(array, order='<', code=None, vox_offset=352, dim=None, pixdim=(1.0, 1.0, 1.0, 1.0), slope=0.0, inter=0.0, sform=None, qform=None,
              magic=b'n+1\0', sizeof_hdr=348, pad=0):
    """A NIfTI-1 byte string assembled from the standard's field offsets, independent of lib/nifti.py's writer.  array: (nz, ny, nx)."""
    nz, ny, nx = array.shape
    code = code if code is not None else {v: k for k, v in CODES.items()}[array.dtype.str.lstrip('<>|=')]
    buf = bytearray(vox_offset)
    struct.pack_into(order + 'i', buf, 0, sizeof_hdr)
    struct.pack_into(order + '8h', buf, 40, *(dim if dim is not None else (3, nx, ny, nz, 1, 1, 1, 1)))
    struct.pack_into(order + 'hh', buf, 70, code, array.dtype.itemsize * 8)
    struct.pack_into(order + '8f', buf, 76, pixdim[0], pixdim[1], pixdim[2], pixdim[3], 1.0, 1.0, 1.0, 1.0)
    struct.pack_into(order + 'f', buf, 108, float(vox_offset))
    struct.pack_into(order + 'ff', buf, 112, slope, inter)
    if qform is not None:                                        # (b, c, d, qoffset_x, qoffset_y, qoffset_z)
        struct.pack_into(order + 'h', buf, 252, 1)
        struct.pack_into(order + '6f', buf, 256, *qform)
    if sform is not None:                                        # 3 x 4
        struct.pack_into(order + 'h', buf, 254, 2)
        struct.pack_into(order + '12f', buf, 280, *np.asarray(sform, dtype=np.float64).reshape(-1))
    buf[344:348] = magic
    data = array.astype(array.dtype.newbyteorder(order)).tobytes()
    return bytes(buf) + data + b'\0' * pad


def put(tmp_path, name, raw):
    p = str(tmp_path / name)
    if name.endswith('.gz'):
        with gzip.open(p, 'wb') as f:
            f.write(raw)
    else:
        with open(p, 'wb') as f:
            f.write(raw)
    return p


def sample_array(kind, shape=(2, 3, 4)):
    n = int(np.prod(shape))
    dt = np.dtype(kind)
    if dt.kind == 'f':
        return (np.arange(n, dtype=np.float64) * 0.37 - 3.1).astype(dt).reshape(shape)
    lo = np.iinfo(dt).min if dt.kind == 'i' else 0
    vals = np.arange(n, dtype=np.int64) * 5 - (7 if lo < 0 else 0)
    vals[-1] = np.iinfo(dt).max if dt.itemsize < 8 else 2 ** 53 + 1          # the top of the range survives the round trip
    return vals.astype(dt).reshape(shape)


@pytest.mark.parametrize('order', ['<', '>'])
@pytest.mark.parametrize('ext', ['.nii', '.nii.gz'])
def test_reader_every_datatype_both_byte_orders(tmp_path, order, ext):
    from deepatlas_amd.lib.nifti import read_nifti
    for code, kind in CODES.items():
        a = sample_array(kind)
        v = read_nifti(put(tmp_path, 'v%d%s' % (code, ext), raw_nifti(a, order=order, pixdim=(1.0, 0.5, 0.0, -2.0))))
        assert v.array.dtype == np.dtype(kind) and v.array.dtype.isnative and v.array.flags['C_CONTIGUOUS'], (code, order)
        assert v.array.shape == (2, 3, 4) and np.array_equal(v.array, a), (code, order)
        assert v.spacing == (0.5, 1.0, 2.0)                    # |pixdim|, 0 replaced by 1
        assert v.header['datatype'] == code and v.header['dim'][:4] == (3, 4, 3, 2)


def test_reader_offset_dim4_and_scaling(tmp_path):
    from deepatlas_amd.lib.nifti import read_nifti
    a = sample_array('i2')
    v = read_nifti(put(tmp_path, 'off.nii', raw_nifti(a, vox_offset=1024)))
    assert np.array_equal(v.array, a)
    v = read_nifti(put(tmp_path, 'd4.nii', raw_nifti(a, dim=(4, 4, 3, 2, 1, 1, 1, 1), pad=9)))
    assert np.array_equal(v.array, a)
    v = read_nifti(put(tmp_path, 'scl.nii', raw_nifti(a, slope=0.5, inter=-3.0)))
    assert v.array.dtype == np.float32 and np.array_equal(v.array, a.astype(np.float32) * np.float32(0.5) + np.float32(-3.0))
    v = read_nifti(put(tmp_path, 'scl64.nii', raw_nifti(sample_array('f8'), slope=2.0, inter=1.0)))
    assert v.array.dtype == np.float64 and np.array_equal(v.array, sample_array('f8') * 2.0 + 1.0)
    for slope, inter in ((0.0, 5.0), (1.0, 0.0), (float('nan'), 1.0), (float('inf'), 0.0)):           # no scaling: the file's own dtype
        v = read_nifti(put(tmp_path, 'noscl.nii', raw_nifti(a, slope=slope, inter=inter)))
        assert v.array.dtype == np.int16 and np.array_equal(v.array, a)


def test_reader_affine_from_sform_qform_and_neither(tmp_path):
    from deepatlas_amd.lib.nifti import read_nifti
    a = sample_array('u1')
    S = [[0.0, -1.5, 0.0, 3.0], [0.5, 0.0, 0.0, -2.0], [0.0, 0.0, 2.0, 7.0]]
    # sform wins over a qform that says something else
    v = read_nifti(put(tmp_path, 's.nii', raw_nifti(a, sform=S, qform=(0.0, 0.0, 0.0, 9.0, 9.0, 9.0), pixdim=(1.0, 0.5, 1.5, 2.0))))
    assert v.affine.dtype == np.float64 and np.array_equal(v.affine, np.array(S + [[0.0, 0.0, 0.0, 1.0]]))
    # qform: 90 degrees about z (a = d = sqrt(1/2)) with qfac = -1 and pixdim (0.5, 1.5, 2): x -> +y, y -> -x, z -> -z
    d = math.sqrt(0.5)
    v = read_nifti(put(tmp_path, 'q.nii', raw_nifti(a, qform=(0.0, 0.0, d, 3.0, -2.0, 7.0), pixdim=(-1.0, 0.5, 1.5, 2.0))))
    want = np.array([[0.0, -1.5, 0.0, 3.0], [0.5, 0.0, 0.0, -2.0], [0.0, 0.0, -2.0, 7.0], [0.0, 0.0, 0.0, 1.0]])
    assert np.abs(v.affine - want).max() < 1e-6               # the quaternion is stored as float32
    assert v.spacing == (0.5, 1.5, 2.0)
    # the same quaternion with qfac = +1 keeps z
    v = read_nifti(put(tmp_path, 'q2.nii', raw_nifti(a, qform=(0.0, 0.0, d, 0.0, 0.0, 0.0), pixdim=(1.0, 0.5, 1.5, 2.0))))
    assert abs(v.affine[2, 2] - 2.0) < 1e-6
    v = read_nifti(put(tmp_path, 'n.nii', raw_nifti(a, pixdim=(0.0, 0.5, 1.5, 2.0))))
    assert np.array_equal(v.affine, np.diag([0.5, 1.5, 2.0, 1.0]))


def test_reader_refusals_carry_their_own_message(tmp_path):
    from deepatlas_amd.lib.nifti import read_nifti
    a = sample_array('i2')
    cases = [('n2.nii', raw_nifti(a, sizeof_hdr=540), 'NIfTI-2'),
             ('pair.nii', raw_nifti(a, magic=b'ni1\0'), 'ni1'),
             ('magic.nii', raw_nifti(a, magic=b'abc\0'), 'bad magic'),
             ('rgb.nii', raw_nifti(a, code=128), r'datatype 128 \(RGB24\)'),
             ('cplx.nii', raw_nifti(a, code=32), 'datatype 32'),
             ('short.nii', raw_nifti(a)[:-5], 'truncated data'),
             ('hdr.nii', raw_nifti(a)[:100], 'truncated header'),
             ('t2.nii', raw_nifti(np.concatenate([a, a]), dim=(4, 4, 3, 2, 2, 1, 1, 1)), 'beyond the third must be 1'),
             ('d2.nii', raw_nifti(a, dim=(2, 4, 3, 1, 1, 1, 1, 1)), r'dim\[0\] = 2'),
             ('nohdr.nii', raw_nifti(a, sizeof_hdr=1234), 'not a NIfTI-1 file')]
    for name, raw, message in cases:
        with pytest.raises(ValueError, match=message):
            read_nifti(put(tmp_path, name, raw))
    with pytest.raises(ValueError, match='truncated'):
        p = put(tmp_path, 'cut.nii.gz', raw_nifti(a))
        blob = open(p, 'rb').read()
        open(p, 'wb').write(blob[:len(blob) - 12])
        read_nifti(p)


@pytest.mark.parametrize('ext', ['.nii', '.nii.gz'])
def test_writer_reader_round_trip_is_bit_exact(tmp_path, ext):
    from deepatlas_amd.lib.nifti import read_nifti, write_nifti
    A = np.array([[0.0, -1.5, 0.0, 3.0], [0.5, 0.0, 0.0, -2.0], [0.0, 0.0, -2.0, 7.0], [0.0, 0.0, 0.0, 1.0]])       # (float32-exact entries)
    for kind in CODES.values():
        a = sample_array(kind, (3, 4, 5))
        p = write_nifti(str(tmp_path / ('w' + ext)), a, spacing=(0.5, 1.5, 2.0), affine=A)
        v = read_nifti(p)
        assert v.array.dtype == a.dtype and np.array_equal(v.array, a), kind
        assert v.spacing == (0.5, 1.5, 2.0) and np.array_equal(v.affine, A)
        assert v.header['vox_offset'] == 352.0 and v.header['sform_code'] > 0 and v.header['qform_code'] > 0
        # the qform says the same as the sform (quaternion in float32)
        h = dict(v.header, sform_code=0)
        from deepatlas_amd.lib.nifti import header_affine
        assert np.abs(header_affine(h) - A).max() < 1e-6
    raw = open(write_nifti(str(tmp_path / 'le.nii'), sample_array('i2')), 'rb').read()
    assert struct.unpack('<i', raw[:4])[0] == 348 and raw[344:348] == b'n+1\0'
    # `like` hands the input's geometry on; spacing alone gives a diagonal affine
    v = read_nifti(write_nifti(str(tmp_path / 'like.nii'), np.zeros((3, 4, 5), dtype=np.uint8), like=v))
    assert v.spacing == (0.5, 1.5, 2.0) and np.array_equal(v.affine, A)
    v = read_nifti(write_nifti(str(tmp_path / 'sp.nii'), np.zeros((3, 4, 5), dtype=np.uint8), spacing=(0.25, 1.0, 3.0)))
    assert v.spacing == (0.25, 1.0, 3.0) and np.array_equal(v.affine, np.diag([0.25, 1.0, 3.0, 1.0]))
    with pytest.raises(ValueError):
        write_nifti(str(tmp_path / 'bad.nii'), np.zeros((3, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        write_nifti(str(tmp_path / 'bad.nii'), np.zeros((3, 4, 5), dtype=np.complex64))


# ---- list files ----------------------------------------------------------------------------------------------------------------------
def write_list(tmp_path, name, names):
    p = str(tmp_path / name)
    with open(p, 'w') as f:
        f.write(''.join(n + '\n' for n in names))
    return p


def test_list_file_paths_of_the_four_families(tmp_path):
    from deepatlas_amd.lib import datasets as ds
    lst = write_list(tmp_path, 'a.txt', ['s1', 's2_LEFT'])
    j = os.path.join
    want = {ds.SegDataSetOAIZIB: (j('root', 's1_image.nii.gz'), j('root', 's1_masks.nii.gz')),
            ds.SegDataSetOASIS: (j('root', 's1_image.nii.gz'), j('root', 's1_seg.nii.gz')),
            ds.SegDataSetBrains: (j('root', 'brain_affine_icbm_hist_matched', 's1.nii'), j('root', 'label_affine_icbm_reID', 's1.nii')),
            ds.SegDataSetMindBoggle: (j('root', 'image_in_MNI152_normalized', 's1.nii.gz'), j('root', 'label_31_reID_merged', 's1.nii.gz'))}
    for cls, (img, seg) in want.items():
        d = cls(lst, 'root')
        assert len(d) == 2 and d.name_list == ['s1', 's2_LEFT'] and d.image_list[0] == img and d.segmentation_list[0] == seg
    names = {'OAI': ds.SegDataSetOAIZIB, 'OASIS': ds.SegDataSetOASIS, 'LPBA40': ds.SegDataSetBrains, 'CUMC12': ds.SegDataSetBrains,
             'IBSR18': ds.SegDataSetBrains, 'MGH10': ds.SegDataSetBrains, 'MindBoggle': ds.SegDataSetMindBoggle}
    for name, cls in names.items():
        assert ds.get_seg_dataset(name) is cls and callable(ds.get_reg_dataset(name))
    assert ds.get_seg_dataset('synthetic') is ds.SyntheticSegDataset and ds.get_reg_dataset('synthetic') is ds.SyntheticRegDataset
    for getter in (ds.get_seg_dataset, ds.get_reg_dataset):
        with pytest.raises(KeyError, match='MindBoggle'):
            getter('nope')


def test_n_samples_and_several_list_files(tmp_path):
    from deepatlas_amd.lib import datasets as ds
    a = write_list(tmp_path, 'a.txt', ['a0', 'a1', 'a2'])
    b = write_list(tmp_path, 'b.txt', ['b0', 'b1'])
    for cls in (ds.SegDataSetOAIZIB, ds.SegDataSetOASIS, ds.SegDataSetBrains, ds.SegDataSetMindBoggle):
        assert cls([a, b], 'r').name_list == ['a0', 'a1', 'a2', 'b0', 'b1']
        assert cls((a, b), 'r', n_samples=None).name_list == ['a0', 'a1', 'a2', 'b0', 'b1']
        assert cls([a, b], 'r', n_samples=4).name_list == ['a0', 'a1', 'a2', 'b0']                 # counted over all files
        assert cls([a, b], 'r', n_samples=0).name_list == []
        assert cls([a, b], 'r', n_samples=[0, 3, 4]).name_list == ['a0', 'b0', 'b1']               # skipped lines are counted (OAI rule)
        assert cls([a, b], 'r', n_samples=(4, 1)).name_list == ['a1', 'b1']
        assert cls(a, 'r', n_samples=range(1, 3)).name_list == ['a1', 'a2']
        for bad in (2.0, {1}, 'a'):
            with pytest.raises(TypeError):
                cls([a, b], 'r', n_samples=bad)


def make_pairs_on_disk(tmp_path, names, shape=(2, 3, 4)):
    from deepatlas_amd.lib.nifti import write_nifti
    for k, n in enumerate(names):
        write_nifti(str(tmp_path / (n + '_image.nii.gz')), (np.arange(int(np.prod(shape))).reshape(shape) + 100 * k).astype(np.int16), spacing=(1.0, 1.0, 2.0))
        write_nifti(str(tmp_path / (n + '_masks.nii.gz')), np.full(shape, k + 1, dtype=np.uint8), spacing=(1.0, 1.0, 2.0))


def test_samples_transforms_and_missing_files(tmp_path):
    from deepatlas_amd.lib import datasets as ds
    names = ['v0', 'v1', 'v2']
    make_pairs_on_disk(tmp_path, names)
    lst = write_list(tmp_path, 'l.txt', names)
    seen = []

    def pre(sample):
        seen.append(('pre', sample['name'], sorted(sample), sample['spacing'], type(sample['image'])))
        return dict(sample, image=torch.from_numpy(sample['image'].astype(np.float32))[None], segmentation=torch.from_numpy(sample['segmentation']))

    def running(sample):
        seen.append(('run', sample['name']))
        return dict(sample, image=sample['image'] + 1)
    d = ds.SegDataSetOAIZIB(lst, str(tmp_path), pre_transform=pre, running_transform=running)
    assert seen == []                                                                               # nothing is read before an access
    item = d[1]
    assert isinstance(item, tuple) and len(item) == 3 and item[2] == 'v1'
    assert seen == [('pre', 'v1', ['image', 'name', 'segmentation', 'spacing'], (1.0, 1.0, 2.0), np.ndarray), ('run', 'v1')]
    assert item[0].shape == (1, 2, 3, 4) and float(item[0][0, 0, 0, 0]) == 101.0 and int(item[1][0, 0, 0]) == 2
    del seen[:]
    d = ds.SegDataSetOAIZIB(lst, str(tmp_path), preload=True, pre_transform=pre, running_transform=running)
    assert [s[:2] for s in seen] == [('pre', 'v0'), ('pre', 'v1'), ('pre', 'v2')]                  # prepared once, at construction
    first, again = d[2], d[2]
    assert [s for s in seen[3:]] == [('run', 'v2'), ('run', 'v2')] and torch.equal(first[0], again[0])      # the kept tensors are not modified
    assert float(first[0][0, 0, 0, 0]) == 201.0
    img, seg, name = ds.SegDataSetOAIZIB(lst, str(tmp_path), with_seg=False)[0]
    assert seg.numel() == 0 and img.shape == (2, 3, 4) and img.dtype == np.int16
    os.remove(str(tmp_path / 'v1_masks.nii.gz'))
    with pytest.raises(ValueError, match='v1_masks.nii.gz not exist'):
        ds.SegDataSetOAIZIB(lst, str(tmp_path))[1]
    with pytest.raises(ValueError, match='not exist'):
        ds.SegDataSetOAIZIB(lst, str(tmp_path), preload=True)
    with pytest.raises(ValueError, match='ghost_image.nii.gz not exist'):
        ds.SegDataSetOAIZIB(write_list(tmp_path, 'g.txt', ['ghost']), str(tmp_path))[0]


class ListSeg(torch.utils.data.Dataset):
    """The (image, segmentation, name) samples of SyntheticSegDataset behind the interface NiftiRegDataset wraps."""

    def __init__(self, n):
        from deepatlas_amd.lib.datasets import SyntheticSegDataset
        self.inner = SyntheticSegDataset(n, (4, 4, 8), 5, seed=7)

    def __len__(self):
        return len(self.inner)

    def __getitem__(self, i):
        return self.inner[i]


@pytest.mark.parametrize('pairs', ['fixed_labeled', 'any_labeled', 'all'])
@pytest.mark.parametrize('labeled', [None, [0, 2]])
def test_pairs_and_tuples_equal_the_synthetic_class(pairs, labeled):
    from deepatlas_amd.lib.datasets import NiftiRegDataset, SyntheticRegDataset
    n = 4
    ref = SyntheticRegDataset(n, (4, 4, 8), 5, seed=7, labeled=labeled, pairs=pairs, moving_remap='invert')
    got = NiftiRegDataset(ListSeg(n), labeled=labeled, pairs=pairs, moving_remap='invert')
    assert isinstance(got, SyntheticRegDataset) and len(got) == len(ref) and got.pairs == ref.pairs
    if labeled is None:
        assert got.pairs == [SyntheticRegDataset.pair_of(i, n) for i in range(n * (n - 1))]
    for i in range(len(ref)):
        a, b = got[i], ref[i]
        assert len(a) == len(b) == (6 if pairs == 'fixed_labeled' else 7)
        for x, y in zip(a, b):
            assert torch.equal(x, y) if torch.is_tensor(x) else x == y
    with pytest.raises(ValueError):
        NiftiRegDataset(ListSeg(1))
    with pytest.raises(ValueError):
        NiftiRegDataset(ListSeg(3), pairs='some')
    with pytest.raises(ValueError):
        NiftiRegDataset(ListSeg(3), moving_remap='other')


def test_reg_factory_has_the_list_file_signature(tmp_path):
    from deepatlas_amd.lib import datasets as ds
    names = ['v0', 'v1', 'v2']
    make_pairs_on_disk(tmp_path, names)
    lst = write_list(tmp_path, 'l.txt', names)
    to_t = lambda s: dict(s, image=torch.from_numpy(s['image'].astype(np.float32))[None], segmentation=torch.from_numpy(s['segmentation']))
    d = ds.get_reg_dataset('OAI')(lst, str(tmp_path), preload=True, pre_transform=to_t, n_samples=3, labeled=[0], pairs='any_labeled')
    assert isinstance(d, ds.NiftiRegDataset) and d.pairs == [(1, 0), (2, 0), (0, 1), (0, 2)]
    im, it, sm, st_, has, name, has_fixed = d[2]
    assert name == 'v0_to_v1' and has and not has_fixed and int(st_.max()) == 0 and int(sm.max()) == 1


# ---- resample tables -----------------------------------------------------------------------------------------------------------------
def brute_table(n_in, n_out, scale, offset, interpolator):
    lo, hi, fr, ins = [], [], [], []
    for o in range(n_out):
        q = float(scale) * float(o) + float(offset)
        ins.append(-0.5 <= q < n_in - 0.5)
        if interpolator == 'nearest':
            k = min(max(int(math.floor(q + 0.5)), 0), n_in - 1)
            lo.append(k), hi.append(k), fr.append(np.float32(0))
        else:
            f = math.floor(q)
            a = min(max(int(f), 0), n_in - 1)
            lo.append(a), hi.append(min(a + 1, n_in - 1)), fr.append(np.float32(0.0 if q < 0 else q - f))
    return np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32), np.array(fr, dtype=np.float32), np.array(ins, dtype=bool)


TABLE_CASES = [(5, 10, 0.5, 0.0), (7, 5, 1.5, 0.0), (9, 14, 2.0 / 3.0, 0.0), (3, 14, 0.25, 0.0), (6, 6, -1.0, 5.0), (1, 4, 0.5, 0.0), (1, 1, 1.0, 0.0),
               (8, 8, 1.0, 0.0), (10, 7, 1.0 / 0.7, 0.0), (5, 9, 0.7, -0.8), (4, 6, -0.5, 3.25)]


@pytest.mark.parametrize('interpolator', ['nearest', 'linear'])
def test_resample_axis_table_against_a_brute_force_loop(interpolator):
    from deepatlas_amd import ops
    for n_in, n_out, scale, offset in TABLE_CASES:
        got = ops.resample_axis_table(n_in, n_out, scale, offset, interpolator)
        want = brute_table(n_in, n_out, scale, offset, interpolator)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and got[3].dtype == bool
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (n_in, n_out, scale, offset)


def test_resample_axis_table_pinned_cases():
    from deepatlas_amd import ops
    T = ops.resample_axis_table
    lo, hi, fr, ins = T(5, 10, 0.5, 0.0, 'nearest')                               # q = 0, .5, 1, ...: ties go up; q = 4.5 is outside
    assert lo.tolist() == [0, 1, 1, 2, 2, 3, 3, 4, 4, 4] and ins.tolist() == [True] * 9 + [False]
    lo, hi, fr, ins = T(5, 10, 0.5, 0.0, 'linear')
    assert lo.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and hi.tolist() == [1, 1, 2, 2, 3, 3, 4, 4, 4, 4] and fr.tolist() == [0.0, 0.5] * 5
    lo, hi, fr, ins = T(7, 5, 1.5, 0.0, 'nearest')                                # q = 0, 1.5, 3, 4.5, 6
    assert lo.tolist() == [0, 2, 3, 5, 6] and ins.all()
    lo, hi, fr, ins = T(7, 5, 1.5, 0.0, 'linear')
    assert lo.tolist() == [0, 1, 3, 4, 6] and hi.tolist() == [1, 2, 4, 5, 6] and fr.tolist() == [0.0, 0.5, 0.0, 0.5, 0.0]
    lo, hi, fr, ins = T(9, 14, 2.0 / 3.0, 0.0, 'linear')
    assert lo.tolist() == [0, 0, 1, 2, 2, 3, 4, 4, 5, 6, 6, 7, 8, 8] and ins.tolist() == [True] * 13 + [False]
    assert fr[1] == np.float32(2.0 / 3.0) and fr[3] == np.float32(3 * (2.0 / 3.0) - 2.0)
    lo, hi, fr, ins = T(3, 14, 0.25, 0.0, 'nearest')                              # q up to 3.25: the last outputs fall outside (q >= 2.5)
    assert ins.tolist() == [True] * 10 + [False] * 4 and lo.tolist() == [0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2]
    lo, hi, fr, ins = T(6, 6, -1.0, 5.0, 'nearest')                               # a flip
    assert lo.tolist() == [5, 4, 3, 2, 1, 0] and ins.all()
    lo, hi, fr, ins = T(6, 6, -1.0, 5.0, 'linear')
    assert lo.tolist() == [5, 4, 3, 2, 1, 0] and not fr.any() and ins.all()
    lo, hi, fr, ins = T(1, 4, 0.5, 0.0, 'linear')                                 # one input voxel: q = 0 only is inside
    assert lo.tolist() == [0] * 4 and hi.tolist() == [0] * 4 and ins.tolist() == [True, False, False, False]
    lo, hi, fr, ins = T(8, 8, 1.0, 0.0, 'linear')                                 # identity
    assert lo.tolist() == list(range(8)) and not fr.any() and ins.all()
    lo, hi, fr, ins = T(5, 3, 1.0, -0.4, 'linear')                                # q = -0.4 is inside, lower tap 0 and fraction 0
    assert ins[0] and lo[0] == 0 and fr[0] == 0.0
    for bad in (dict(n_in=0, n_out=3), dict(n_in=3, n_out=0), dict(n_in=3, n_out=3, scale=float('nan')), dict(n_in=3, n_out=3, interpolator='cubic')):
        kw = dict(dict(scale=1.0, offset=0.0, interpolator='nearest'), **bad)
        with pytest.raises(ValueError):
            T(**kw)


def test_resample_new_size_at_exact_and_inexact_quotients():
    from deepatlas_amd.lib.transforms import Resample
    # the reference's formula, rounding included: 0.36 * 384 / 0.36 is 384.00000000000006 in double, and its ceil is 385
    assert Resample.new_size((384, 384, 160), (0.36, 0.36, 0.7), (0.36, 0.36, 0.7)) == (385, 385, 160)
    assert Resample.new_size((384, 384, 160), (0.5, 0.25, 0.75), (0.5, 0.25, 0.75)) == (384, 384, 160)
    assert Resample.new_size((4, 6, 8), (1.0, 1.0, 2.0), (1.0, 1.0, 1.0)) == (4, 6, 16)
    assert Resample.new_size((10, 10, 10), (0.7, 0.7, 0.7), (1.0, 1.0, 1.0)) == (7, 7, 7)
    assert Resample.new_size((10, 10, 10), (0.7, 0.7, 0.7), (1.0, 1.0, 1.0)) == tuple(int(math.ceil(0.7 * 10 / 1.0)) for _ in range(3))
    assert Resample.new_size((5, 7, 9), (1.0, 1.0, 1.0), (2.0, 3.0, 4.0)) == (3, 3, 3)
    assert Resample.new_size((3, 3, 3), (0.1, 0.1, 0.1), (0.3, 0.3, 0.3)) == tuple(int(math.ceil(0.1 * 3 / 0.3)) for _ in range(3))
    assert Resample(2.0).voxel_size == (2.0, 2.0, 2.0) and Resample([1, 2, 3]).voxel_size == (1.0, 2.0, 3.0)
    for bad in ((1.0, 2.0), (1.0, 0.0, 1.0), -1.0):
        with pytest.raises(ValueError):
            Resample(bad)
    with pytest.raises(ValueError):
        Resample(1.0, interpolator='bspline')


# ---- symbols, arguments, command line --------------------------------------------------------------------------------------------------
def test_symbols_in_header_signatures_and_library():
    import __graft_entry__ as ge
    from deepatlas_amd import _native
    header = open(os.path.join(ROOT, 'include', 'deepatlas_hip.h')).read()
    declared = set(re.findall(r'\b(da_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(ge.build())
    for name in PREPROCESS_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert 'preprocess.hip' in ge.HIP_SOURCES
    L = _native.lib()
    fake = ctypes.c_void_p(0x1000)
    big = 1 << 40
    two = (ctypes.c_double * 2)(0.5, 99.5)
    three = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    # da_resample_axes: null pointers, dtype, interpolator, extents -> -1; 2^31 voxels in or out -> -3
    ok = (1, 3, 4, 5, 3, 4, 5)
    assert L.da_resample_axes(None, 0, fake, 1, *ok, fake, 0.0, None) == -1
    assert L.da_resample_axes(fake, 0, None, 1, *ok, fake, 0.0, None) == -1
    assert L.da_resample_axes(fake, 0, fake, 1, *ok, None, 0.0, None) == -1
    assert L.da_resample_axes(fake, 5, fake, 1, *ok, fake, 0.0, None) == -1
    assert L.da_resample_axes(fake, -1, fake, 1, *ok, fake, 0.0, None) == -1
    assert L.da_resample_axes(fake, 0, fake, 2, *ok, fake, 0.0, None) == -1
    assert L.da_resample_axes(fake, 0, fake, 1, 1, 3, 4, 5, 3, 0, 5, fake, 0.0, None) == -1
    assert L.da_resample_axes(fake, 0, fake, 1, 1, 2048, 1024, 1024, 3, 4, 5, fake, 0.0, None) == -3
    assert L.da_resample_axes(fake, 0, fake, 0, 2, 3, 4, 5, 1024, 1024, 1024, fake, 0.0, None) == -3
    # moments
    assert L.da_volume_moments_ws_bytes(100) > 0 and L.da_volume_moments_ws_bytes(0) == 0 and L.da_volume_moments_ws_bytes(2 ** 31) == 0
    assert L.da_volume_moments(None, 0, 100, fake, fake, big, None) == -1
    assert L.da_volume_moments(fake, 0, 100, None, fake, big, None) == -1
    assert L.da_volume_moments(fake, 0, 100, fake, None, big, None) == -1
    assert L.da_volume_moments(fake, 7, 100, fake, fake, big, None) == -1
    assert L.da_volume_moments(fake, 0, 0, fake, fake, big, None) == -1
    assert L.da_volume_moments(fake, 0, 100, fake, fake, 8, None) == -2
    assert L.da_volume_moments(fake, 0, 2 ** 31, fake, fake, big, None) == -3
    # percentiles
    assert L.da_volume_percentiles_ws_bytes(100) >= 4 * 2048 * 4 and L.da_volume_percentiles_ws_bytes(2 ** 31) == 0
    assert L.da_volume_percentiles(None, 0, 100, two, 2, fake, fake, big, None) == -1
    assert L.da_volume_percentiles(fake, 0, 100, None, 2, fake, fake, big, None) == -1
    assert L.da_volume_percentiles(fake, 0, 100, two, 2, None, fake, big, None) == -1
    assert L.da_volume_percentiles(fake, 0, 100, two, 2, fake, None, big, None) == -1
    assert L.da_volume_percentiles(fake, 9, 100, two, 2, fake, fake, big, None) == -1
    assert L.da_volume_percentiles(fake, 0, 100, three, 3, fake, fake, big, None) == -1               # more than two percentiles
    assert L.da_volume_percentiles(fake, 0, 100, two, 0, fake, fake, big, None) == -1
    assert L.da_volume_percentiles(fake, 0, 100, (ctypes.c_double * 1)(101.0), 1, fake, fake, big, None) == -1
    assert L.da_volume_percentiles(fake, 0, 100, (ctypes.c_double * 1)(float('nan')), 1, fake, fake, big, None) == -1
    assert L.da_volume_percentiles(fake, 0, 100, two, 2, fake, fake, 64, None) == -2
    assert L.da_volume_percentiles(fake, 0, 2 ** 31, two, 2, fake, fake, big, None) == -3
    # affine intensity, look-up table
    assert L.da_affine_intensity_to_f32(None, 0, fake, 100, 0.0, 1.0, 0, None) == -1
    assert L.da_affine_intensity_to_f32(fake, 0, None, 100, 0.0, 1.0, 0, None) == -1
    assert L.da_affine_intensity_to_f32(fake, 5, fake, 100, 0.0, 1.0, 0, None) == -1
    assert L.da_affine_intensity_to_f32(fake, 0, fake, 100, 0.0, 1.0, 2, None) == -1
    assert L.da_affine_intensity_to_f32(fake, 0, fake, 2 ** 31, 0.0, 1.0, 0, None) == -3
    assert L.da_label_lut(None, 3, fake, 100, fake, 256, None) == -1
    assert L.da_label_lut(fake, 3, fake, 100, None, 256, None) == -1
    assert L.da_label_lut(fake, 0, fake, 100, fake, 256, None) == -1                                 # float labels
    assert L.da_label_lut(fake, 2, fake, 100, fake, 256, None) == -1
    assert L.da_label_lut(fake, 4, fake, 100, fake, 65537, None) == -1
    assert L.da_label_lut(fake, 4, fake, 100, fake, 0, None) == -1
    assert L.da_label_lut(fake, 4, fake, 2 ** 31, fake, 256, None) == -3


def test_argument_errors_are_raised_before_the_device():
    from deepatlas_amd import ops, _native
    v = torch.zeros((3, 4, 5))
    with pytest.raises(ValueError):
        ops.resample_volume(v, (3, 4, 5), (1, 1, 1), (0, 0, 0), 'cubic')
    with pytest.raises(ValueError):
        ops.resample_volume(v, (3, 4), (1, 1, 1), (0, 0, 0))
    with pytest.raises(ValueError):
        ops.resample_volume(v, (3, 0, 5), (1, 1, 1), (0, 0, 0))
    with pytest.raises(ValueError):
        ops.resample_volume(v.to(torch.int64), (3, 4, 5), (1, 1, 1), (0, 0, 0))
    with pytest.raises(ValueError):
        ops.resample_volume(v[0], (3, 4, 5), (1, 1, 1), (0, 0, 0))
    huge = torch.zeros(1).expand(2048, 1024, 1024)                                                # zero strides: nothing allocated
    with pytest.raises(ValueError, match='2\\^31'):
        ops.volume_moments(huge)
    with pytest.raises(ValueError, match='2\\^31'):
        ops.resample_volume(v, (2048, 1024, 1024), (1, 1, 1), (0, 0, 0))
    with pytest.raises(ValueError):
        ops.volume_percentiles(v, (1, 2, 3))
    with pytest.raises(ValueError):
        ops.volume_percentiles(v, (50, 101))
    with pytest.raises(ValueError):
        ops.label_lut(v, [0, 1])
    with pytest.raises(ValueError):
        ops.label_lut(v.to(torch.uint8), list(range(65537)))
    # a well-formed call on a host tensor fails loudly: there is no CPU path
    for fn in (lambda: ops.resample_volume(v, (3, 4, 5), (1, 1, 1), (0, 0, 0)), lambda: ops.volume_moments(v), lambda: ops.volume_percentiles(v, (1, 99)),
               lambda: ops.affine_intensity(v, 0.0, 1.0), lambda: ops.label_lut(v.to(torch.uint8), [0, 1])):
        with pytest.raises(_native.NativeError):
            fn()


def test_command_line_flags_and_untouched_synthetic_configs(tmp_path, monkeypatch):
    import train_joint
    import train_reg
    import train_seg
    from deepatlas_amd.lib import transforms as T
    from deepatlas_amd.models import nifti_data
    seen = []

    class Fake(object):
        def __init__(self, config):
            seen.append(config)

        def train(self):
            pass

        def test(self):
            pass
    monkeypatch.setattr(train_seg, 'SegmentationExperiment', Fake)
    monkeypatch.setattr(train_reg, 'RegistrationExperiment', Fake)
    monkeypatch.setattr(train_joint, 'DeepAtlasExperiment', Fake)
    new_keys = set(nifti_data._ARGUMENT_KEYS) | {'training_list_file', 'validation_list_file', 'testing_list_file', 'preprocess'}
    flags = ['--data', 'OAI', '--data-dir', '/d', '--train-list', 'a.txt', 'b.txt', '--valid-list', 'v.txt', '--test-list', 't.txt', '--voxel-size', '1', '1', '1',
             '--rescale-percentiles', '0.5', '99.5', '--normalize', '--ignore-labels', '3', '4', '--crop-size', '1', '2', '3', '--preload']
    for mod in (train_seg, train_reg, train_joint):
        del seen[:]
        mod.main([])
        mod.main(flags)
        plain, cfg = seen
        assert plain['data'] == 'synthetic' and not (new_keys & set(plain)) and plain['log_dir'] == '././logs/synthetic'
        assert plain['data_dir'] == os.path.join('./data', 'synthetic')
        assert cfg['data'] == 'OAI' and cfg['data_dir'] == '/d' and cfg['valid_data_dir'] == '/d' and cfg['log_dir'] == '././logs/OAI'
        assert cfg['training_list_file'] == ['a.txt', 'b.txt'] and cfg['validation_list_file'] == ['v.txt'] and cfg['testing_list_file'] == ['t.txt']
        assert cfg['preload'] is True and cfg['crop_size'] == [1, 2, 3] and not (set(nifti_data._ARGUMENT_KEYS) & set(cfg))
        assert cfg['preprocess'] == [['resample', {'voxel_size': [1.0, 1.0, 1.0]}], ['percentile_rescale', {'lo': 0.5, 'hi': 99.5}], ['normalize', {}],
                                     ['label_filter', {'ignore_labels': [3, 4]}]]
        with pytest.raises(ValueError):
            mod.main(['--data', 'OAI'])
    # build_config tolerates a namespace without the new attributes
    args = argparse.Namespace(debug=False, num_epochs=1, num_samples=2, lr=1e-3, shape=[16, 16, 16], data_root='./data', log_root='./logs', device='0')
    assert train_seg.build_config(args)['data'] == 'synthetic'
    steps = T.make_preprocess(seen[1]['preprocess'] + [['left_to_right', {}], ['identity', None]])
    assert [type(s) for s in steps] == [T.Resample, T.PercentileRescale, T.Normalization, T.SegmentationLabelFilter, T.LeftToRight, T.IdentityTransform]
    with pytest.raises(ValueError):
        T.make_preprocess([['sharpen', {}]])
    chain = nifti_data.pre_transform(dict(seen[1]))
    assert isinstance(chain.transforms[-2], T.SitkToTensor) and isinstance(chain.transforms[-1], T.CropTensor) and len(chain.transforms) == 6
    assert isinstance(nifti_data.pre_transform({'crop_size': None}).transforms[-1], T.SitkToTensor)


def test_synthetic_only_options_and_shape_check():
    from deepatlas_amd.models import nifti_data
    nifti_data.refuse_synthetic_only({'data': 'synthetic', 'misalign': (5.0, 2.0)}, ('misalign', 'report_tre'))
    nifti_data.refuse_synthetic_only({'data': 'OAI', 'misalign': None}, ('misalign', 'report_tre'))
    with pytest.raises(ValueError, match='synthetic-only'):
        nifti_data.refuse_synthetic_only({'data': 'OAI', 'misalign': (5.0, 2.0)}, ('misalign', 'report_tre'))
    with pytest.raises(ValueError, match='synthetic-only'):
        nifti_data.refuse_synthetic_only({'data': 'OAI', 'report_tre': {'amp_vox': 2.0}}, ('misalign', 'report_tre'))

    def vols(shapes):
        return [(torch.zeros((1,) + s), torch.zeros(s, dtype=torch.uint8), 'vol%d' % k) for k, s in enumerate(shapes)]
    assert nifti_data.check_shapes([vols([(8, 16, 24)] * 2), None, vols([(8, 16, 24)])], ['UNet_light', 'voxel_morph_cvpr']) == (8, 16, 24)
    with pytest.raises(ValueError, match=r'vol0 8x16x24, vol1 8x16x16'):
        nifti_data.check_shapes([vols([(8, 16, 24), (8, 16, 16)])], ['UNet_light'])
    with pytest.raises(ValueError, match=r'multiples of 8: vol0 8x16x20'):
        nifti_data.check_shapes([vols([(8, 16, 20)])], ['UNet_light'])
    assert nifti_data.check_shapes([vols([(8, 16, 20)])], ['voxel_morph_cvpr']) == (8, 16, 20)
    with pytest.raises(ValueError):
        nifti_data.check_shapes([None, []], ['UNet_light'])
