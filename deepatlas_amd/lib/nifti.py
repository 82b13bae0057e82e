"""Single-file NIfTI-1 reader and writer on numpy and the standard library (the reference reads its volumes through SimpleITK,
lib/datasets.py:16-328; a NIfTI-1 file is a 348-byte header followed by a raw array, which needs neither).

read_nifti(path) -> Volume with
  array    numpy, C-contiguous, shape (nz, ny, nx): the file stores i (x) fastest, so this is exactly sitk.GetArrayFromImage's array and no
           axis is moved; scl_slope / scl_inter applied when the slope is finite, non-zero and not (1, 0) (float32, float64 for 64-bit data)
  spacing  (x, y, z) = |pixdim[1:4]|, 0 replaced by 1
  affine   4 x 4 float64 voxel (i, j, k) -> world: the sform when sform_code > 0, else the qform (the standard's quaternion formula with
           qfac), else diag(pixdim)
  header   the raw header fields, a dict
Supported: .nii and .nii.gz, magic 'n+1', little and big endian (detected from sizeof_hdr == 348 in either byte order), dim[0] in 3..7 with
every extent beyond the third equal to 1, vox_offset, datatypes u8 i16 i32 f32 f64 i8 u16 u32 i64 u64.  Everything else (NIfTI-2, 'ni1'
header / image pairs, RGB and complex data, truncated data) raises a ValueError that says which.  Not done here: reorientation by the affine.

write_nifti(path, array, like=None, spacing=None, affine=None) writes little endian with sform and qform set and vox_offset 352, so a
prediction can leave the process with its input's geometry (like=the input Volume).

write_nifti_field(path, array (3, nz, ny, nx) float32, like=...) / read_nifti_field(path): a displacement field as a 5-D vector image,
dim = [5, nx, ny, nz, 1, 3], intent code 1007, the layout ITK and ANTs use; read_nifti and write_nifti keep refusing it.
"""
import gzip
import struct

import numpy as np

HEADER_BYTES = 348
# datatype code -> numpy type character (without byte order)
DATATYPES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 256: 'i1', 512: 'u2', 768: 'u4', 1024: 'i8', 1280: 'u8'}
_UNSUPPORTED_NAMES = {0: 'unknown', 1: 'binary', 32: 'complex64', 128: 'RGB24', 1536: 'float128', 1792: 'complex128', 2048: 'complex256',
                      2304: 'RGBA32'}
_CODE_OF = {np.dtype(v).newbyteorder('<').str.lstrip('<|'): k for k, v in DATATYPES.items()}


class Volume(object):
    """What read_nifti returns: array (nz, ny, nx), spacing (x, y, z), affine 4 x 4 float64, header dict."""

    def __init__(self, array, spacing, affine, header):
        self.array = array
        self.spacing = tuple(float(s) for s in spacing)
        self.affine = affine
        self.header = header

    def __repr__(self):
        return 'Volume(shape=%s, dtype=%s, spacing=%s)' % (self.array.shape, self.array.dtype, self.spacing)


def _read_all(path):
    path = str(path)
    if path.endswith('.gz'):
        try:
            with gzip.open(path, 'rb') as f:
                return f.read()
        except EOFError:
            raise ValueError('%s: truncated gzip stream' % path)
    with open(path, 'rb') as f:
        return f.read()


def quaternion_affine(b, c, d, qoffset, pixdim, qfac):
    """The standard's qform: rotation from the unit quaternion (a, b, c, d), a = sqrt(1 - b^2 - c^2 - d^2) >= 0, columns scaled by
    pixdim[1:4], the third also by qfac (-1 or 1), translation qoffset."""
    b, c, d = float(b), float(c), float(d)
    a = 1.0 - (b * b + c * c + d * d)
    if a < 1e-7:                                   # |(b, c, d)| >= 1: a = 0 and the vector is normalised (nifti1_io's quatern_to_mat44)
        s = 1.0 / np.sqrt(b * b + c * c + d * d)
        b, c, d, a = b * s, c * s, d * s, 0.0
    else:
        a = np.sqrt(a)
    R = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                  [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                  [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]], dtype=np.float64)
    scale = np.array([pixdim[0], pixdim[1], pixdim[2] * (-1.0 if qfac < 0 else 1.0)], dtype=np.float64)
    A = np.eye(4)
    A[:3, :3] = R * scale[None, :]
    A[:3, 3] = qoffset
    return A


def affine_quaternion(affine):
    """Inverse of quaternion_affine for an affine with orthogonal columns: (b, c, d), qoffset, pixdim (3), qfac."""
    A = np.asarray(affine, dtype=np.float64)
    M = A[:3, :3].copy()
    pix = np.sqrt((M * M).sum(0))
    pix[pix == 0] = 1.0
    R = M / pix[None, :]
    qfac = 1.0
    if np.linalg.det(R) < 0:
        R[:, 2] = -R[:, 2]
        qfac = -1.0
    r11, r12, r13, r21, r22, r23, r31, r32, r33 = R.reshape(-1)
    a = r11 + r22 + r33 + 1.0
    if a > 0.5:
        a = 0.5 * np.sqrt(a)
        b, c, d = 0.25 * (r32 - r23) / a, 0.25 * (r13 - r31) / a, 0.25 * (r21 - r12) / a
    else:
        xd, yd, zd = 1.0 + r11 - (r22 + r33), 1.0 + r22 - (r11 + r33), 1.0 + r33 - (r11 + r22)
        if xd > 1.0:
            b = 0.5 * np.sqrt(xd)
            c, d, a = 0.25 * (r12 + r21) / b, 0.25 * (r13 + r31) / b, 0.25 * (r32 - r23) / b
        elif yd > 1.0:
            c = 0.5 * np.sqrt(yd)
            b, d, a = 0.25 * (r12 + r21) / c, 0.25 * (r23 + r32) / c, 0.25 * (r13 - r31) / c
        else:
            d = 0.5 * np.sqrt(zd)
            b, c, a = 0.25 * (r13 + r31) / d, 0.25 * (r23 + r32) / d, 0.25 * (r21 - r12) / d
        if a < 0:
            b, c, d = -b, -c, -d
    return (float(b), float(c), float(d)), A[:3, 3].copy(), pix, qfac


def parse_header(raw, name='<bytes>'):
    """The fields of a 348-byte NIfTI-1 header -> (dict, byte-order character)."""
    if len(raw) < 4:
        raise ValueError('%s: truncated header (%d bytes)' % (name, len(raw)))
    order = None
    for o in '<>':
        size = struct.unpack(o + 'i', raw[:4])[0]
        if size == HEADER_BYTES:
            order = o
            break
        if size == 540:
            raise ValueError('%s: NIfTI-2 (sizeof_hdr 540) is not supported' % name)
    if order is None:
        raise ValueError('%s: not a NIfTI-1 file (sizeof_hdr %d)' % (name, struct.unpack('<i', raw[:4])[0]))
    if len(raw) < HEADER_BYTES:
        raise ValueError('%s: truncated header (%d of %d bytes)' % (name, len(raw), HEADER_BYTES))
    magic = raw[344:348]
    if magic == b'ni1\0':
        raise ValueError("%s: 'ni1' header / image pairs are not supported (single-file 'n+1' only)" % name)
    if magic != b'n+1\0':
        raise ValueError('%s: bad magic %r (single-file NIfTI-1 has n+1)' % (name, magic))
    u = lambda fmt, off: struct.unpack_from(order + fmt, raw, off)
    h = {'sizeof_hdr': HEADER_BYTES, 'dim': u('8h', 40), 'intent_p': u('3f', 56), 'intent_code': u('h', 68)[0], 'datatype': u('h', 70)[0],
         'bitpix': u('h', 72)[0], 'slice_start': u('h', 74)[0], 'pixdim': u('8f', 76), 'vox_offset': u('f', 108)[0],
         'scl_slope': u('f', 112)[0], 'scl_inter': u('f', 116)[0], 'xyzt_units': raw[123], 'cal_max': u('f', 124)[0], 'cal_min': u('f', 128)[0],
         'descrip': raw[148:228].split(b'\0')[0], 'qform_code': u('h', 252)[0], 'sform_code': u('h', 254)[0], 'quatern': u('3f', 256),
         'qoffset': u('3f', 268), 'srow_x': u('4f', 280), 'srow_y': u('4f', 296), 'srow_z': u('4f', 312), 'magic': magic}
    return h, order


def header_affine(h):
    """sform when sform_code > 0, else qform when qform_code > 0, else diag(pixdim); 4 x 4 float64."""
    if h['sform_code'] > 0:
        A = np.eye(4)
        A[0], A[1], A[2] = h['srow_x'], h['srow_y'], h['srow_z']
        return A
    pix = [float(p) for p in h['pixdim'][1:4]]
    if h['qform_code'] > 0:
        return quaternion_affine(*h['quatern'], qoffset=h['qoffset'], pixdim=pix, qfac=h['pixdim'][0])
    return np.diag(pix + [1.0]).astype(np.float64)


def read_nifti(path):
    name = str(path)
    raw = _read_all(path)
    h, order = parse_header(raw, name)
    ndim = h['dim'][0]
    if not 3 <= ndim <= 7:
        raise ValueError('%s: dim[0] = %d, a volume needs 3..7' % (name, ndim))
    extents = h['dim'][1:1 + ndim]
    if min(extents[:3]) < 1:
        raise ValueError('%s: bad extents %s' % (name, (extents,)))
    if any(e != 1 for e in extents[3:]):
        raise ValueError('%s: extents %s: every extent beyond the third must be 1 (one 3-D volume per file)' % (name, tuple(extents)))
    code = h['datatype']
    if code not in DATATYPES:
        raise ValueError('%s: datatype %d (%s) is not supported' % (name, code, _UNSUPPORTED_NAMES.get(code, 'not a NIfTI-1 code')))
    dt = np.dtype(DATATYPES[code]).newbyteorder(order)
    nx, ny, nz = (int(e) for e in extents[:3])
    offset = int(h['vox_offset'])
    if offset < HEADER_BYTES + 4:
        offset = HEADER_BYTES + 4
    need = nx * ny * nz * dt.itemsize
    if len(raw) < offset + need:
        raise ValueError('%s: truncated data: %d bytes after offset %d, %d needed' % (name, max(len(raw) - offset, 0), offset, need))
    arr = np.frombuffer(raw, dtype=dt, count=nx * ny * nz, offset=offset).reshape(nz, ny, nx)
    arr = np.ascontiguousarray(arr.astype(dt.newbyteorder('='), copy=True))
    slope, inter = float(h['scl_slope']), float(h['scl_inter'])
    if np.isfinite(slope) and slope != 0.0 and np.isfinite(inter) and not (slope == 1.0 and inter == 0.0):
        wide = np.float64 if dt.itemsize == 8 else np.float32
        arr = arr.astype(wide) * wide(slope) + wide(inter)
    spacing = tuple(abs(float(p)) or 1.0 for p in h['pixdim'][1:4])
    return Volume(arr, spacing, header_affine(h), h)


def _resolve_geometry(like, spacing, affine):
    """write_nifti's geometry rule: (spacing or None, affine 4 x 4 float64)."""
    if affine is None and like is not None:
        affine = like.affine
    if spacing is None and like is not None:
        spacing = like.spacing
    if affine is None:
        affine = np.diag([float(s) for s in (spacing or (1.0, 1.0, 1.0))] + [1.0])
    affine = np.asarray(affine, dtype=np.float64)
    if affine.shape != (4, 4):
        raise ValueError('affine must be 4 x 4')
    return spacing, affine


def _header_bytes(dim8, dtype, spacing, affine, intent_code=0):
    """The 352 bytes in front of the data: little endian, sform and qform both set (codes 1), vox_offset 352, no scaling."""
    (qb, qc, qd), qoff, qpix, qfac = affine_quaternion(affine)
    if spacing is None:
        spacing = qpix
    if max(dim8[1:4]) > 32767:
        raise ValueError('NIfTI-1 extents are 16-bit: shape %s' % (tuple(reversed(dim8[1:4])),))
    key = np.dtype(dtype).newbyteorder('<').str.lstrip('<|')
    buf = bytearray(HEADER_BYTES + 4)
    struct.pack_into('<i', buf, 0, HEADER_BYTES)
    struct.pack_into('<8h', buf, 40, *dim8)
    struct.pack_into('<h', buf, 68, intent_code)
    struct.pack_into('<hh', buf, 70, _CODE_OF[key], np.dtype(dtype).itemsize * 8)
    struct.pack_into('<8f', buf, 76, qfac, float(spacing[0]), float(spacing[1]), float(spacing[2]), 1.0, 1.0, 1.0, 1.0)
    struct.pack_into('<f', buf, 108, 352.0)
    struct.pack_into('<ff', buf, 112, 1.0, 0.0)
    buf[123] = 2                                                 # NIFTI_UNITS_MM
    struct.pack_into('<hh', buf, 252, 1, 1)
    struct.pack_into('<3f', buf, 256, qb, qc, qd)
    struct.pack_into('<3f', buf, 268, *[float(v) for v in qoff])
    for row, off in enumerate((280, 296, 312)):
        struct.pack_into('<4f', buf, off, *[float(v) for v in affine[row]])
    buf[344:348] = b'n+1\0'
    return buf


def _write_all(path, buf, data):
    path = str(path)
    if path.endswith('.gz'):
        with gzip.open(path, 'wb', compresslevel=1) as f:
            f.write(bytes(buf))
            f.write(data)
    else:
        with open(path, 'wb') as f:
            f.write(bytes(buf))
            f.write(data)
    return path


def write_nifti(path, array, like=None, spacing=None, affine=None):
    """array (nz, ny, nx) in one of the supported dtypes (bool -> uint8, float16 -> float32).  Geometry: `affine` (4 x 4), else `like`'s (a
    Volume), else diag(spacing); `spacing` (x, y, z) defaults to like's, else the affine's column norms, else 1.  Little endian, sform and
    qform both set (codes 1, 'scanner'), vox_offset 352, no scaling."""
    arr = np.asarray(array)
    if arr.ndim != 3:
        raise ValueError('write_nifti takes one 3-D volume (nz, ny, nx), got shape %s' % (arr.shape,))
    if arr.dtype == np.bool_:
        arr = arr.astype(np.uint8)
    elif arr.dtype == np.float16:
        arr = arr.astype(np.float32)
    key = arr.dtype.newbyteorder('<').str.lstrip('<|')
    if key not in _CODE_OF:
        raise ValueError('write_nifti: dtype %s is not a supported NIfTI-1 datatype' % arr.dtype)
    spacing, affine = _resolve_geometry(like, spacing, affine)
    nz, ny, nx = arr.shape
    buf = _header_bytes((3, nx, ny, nz, 1, 1, 1, 1), arr.dtype, spacing, affine)
    data = np.ascontiguousarray(arr.astype(arr.dtype.newbyteorder('<'), copy=False)).tobytes()
    return _write_all(path, buf, data)


# ---- displacement fields: a 5-D vector image (dim = [5, nx, ny, nz, 1, 3], intent NIFTI_INTENT_VECTOR), the layout ITK and ANTs write --------
INTENT_VECTOR = 1007


def write_nifti_field(path, array, like=None, spacing=None, affine=None):
    """array (3, nz, ny, nx) float32: a displacement in millimetres per voxel, component (world x, y, z) first.  Written as dim = [5, nx, ny,
    nz, 1, 3] with intent code 1007 (vector); the component is the slowest file axis, so the array goes out as it lies.  Geometry as in
    write_nifti.  read_nifti refuses such a file (more than one volume); read_nifti_field reads it."""
    arr = np.asarray(array)
    if arr.ndim != 4 or arr.shape[0] != 3:
        raise ValueError('write_nifti_field takes a (3, nz, ny, nx) array, got shape %s' % (arr.shape,))
    if arr.dtype != np.float32:
        raise ValueError('write_nifti_field takes float32, got %s' % arr.dtype)
    spacing, affine = _resolve_geometry(like, spacing, affine)
    _, nz, ny, nx = arr.shape
    buf = _header_bytes((5, nx, ny, nz, 1, 3, 1, 1), arr.dtype, spacing, affine, intent_code=INTENT_VECTOR)
    return _write_all(path, buf, np.ascontiguousarray(arr.astype('<f4', copy=False)).tobytes())


def read_nifti_field(path):
    """A file write_nifti_field wrote (or any NIfTI-1 with dim = [5, nx, ny, nz, 1, 3], float32, intent 1007) -> Volume whose array is
    (3, nz, ny, nx) float32; spacing, affine and header as read_nifti gives them."""
    name = str(path)
    raw = _read_all(path)
    h, order = parse_header(raw, name)
    dim = h['dim']
    if dim[0] != 5 or dim[4] != 1 or dim[5] != 3 or min(dim[1:4]) < 1:
        raise ValueError('%s: dim %s is not a displacement field [5, nx, ny, nz, 1, 3]' % (name, tuple(dim[:6])))
    if h['intent_code'] != INTENT_VECTOR:
        raise ValueError('%s: intent code %d, a displacement field has %d (vector)' % (name, h['intent_code'], INTENT_VECTOR))
    if h['datatype'] != 16:
        raise ValueError('%s: datatype %d, a displacement field is float32 (16)' % (name, h['datatype']))
    nx, ny, nz = (int(e) for e in dim[1:4])
    offset = max(int(h['vox_offset']), HEADER_BYTES + 4)
    need = 3 * nx * ny * nz * 4
    if len(raw) < offset + need:
        raise ValueError('%s: truncated data: %d bytes after offset %d, %d needed' % (name, max(len(raw) - offset, 0), offset, need))
    arr = np.frombuffer(raw, dtype=np.dtype('f4').newbyteorder(order), count=3 * nx * ny * nz, offset=offset).reshape(3, nz, ny, nx)
    arr = np.ascontiguousarray(arr.astype(np.float32, copy=True))
    spacing = tuple(abs(float(p)) or 1.0 for p in h['pixdim'][1:4])
    return Volume(arr, spacing, header_affine(h), h)
