"""From a BraTS download to a filled volume store, on the device: the step in front of every phase of this package.

The reference trains from an h5 file of already normalised volumes.  The only record of how they were made is a commented-out block of its
preprocessing script (`src/data_preprocessing_BraTS.py:70-98`; the same rule is live in `data_preprocessing_ZeroDose.py:124-134`); the fold lists
come from lines 100-146 of the same script.  This module restates both:
  * `read_nifti`            a single-file NIfTI-1 reader on gzip, struct and numpy.frombuffer alone: the voxel array as the file holds it
  * `prep_stats` / `prep_write` / `prep_volume`
                            the rule of :79-96 as two HIP entry points (csrc/mrdis_prep.hip): the raw voxels go to the device in their own
                            dtype (int16 for BraTS: 18 MB instead of 71 MB of float64) and the fp32 store volume is written there
  * `build_store_from_raw`  a directory of subjects -> VolumeStore / VolumeStore3D, with the rejection rule of :80
  * `write_fold_lists`      :100-146: the five folds, as 2-D (`subject slice`) and 3-D (one id per line) list files
  * `write_nifti` / `save_nifti` / `export_store_volume`
                            the way back: label and synthesized volumes, in the store's cropped geometry on the device, as NIfTI files on the
                            scan's own canvas, in its geometry and (units 'scan') its units -- hip.export_volume (csrc/mrdis_export.hip), one
                            device-to-host copy and a stdlib NIfTI-1 writer; needs what build_store_from_raw keeps in `store.raw_meta`
Conventions of this package, where the reference leaves a choice or depends on its file system:
  * subjects are taken in SORTED order (the reference: `glob` order);
  * a subject with one rejected volume is dropped WHOLE, with one log line (the reference `break`s and leaves half a group in the file);
  * `norm_type: mean` is `v / norm` with nothing filled in: this package's reading of the commented alternative at :91, which made the
    `BraTS_All.h5` whose background is 0;
  * the ZeroDose rule's template brain mask and its padding are not built.
"""
import gzip
import math
import os
import struct
import sys
import warnings

import numpy as np
import torch

from . import hip
from .data import VolumeStore

NIFTI_DTYPES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 512: 'u2'}      # NIfTI-1 datatype code -> numpy kind
BRATS_FILES = (('T1', 't1'), ('T1c', 't1ce'), ('T2', 't2'), ('T2_FLAIR', 'flair'), ('seg', 'seg'))      # store key, file suffix (:45-59)
BRATS_CROP = ((40, 40), (24, 24))                 # (240, 240, 155) -> (160, 192, 155)   (:85)
BRATS_INNER = (50, 50)                            # the planes whose NaNs the rejection rule counts (:80)
MAX_INNER_NAN = 100000                            # :80
HEADER_BYTES = 348
GEOMETRY_FLOATS = ('quatern_b', 'quatern_c', 'quatern_d', 'qoffset_x', 'qoffset_y', 'qoffset_z')      # header bytes 256 .. 279, in this order
DEFAULT_GEOMETRY = {'dim_info': 0, 'xyzt_units': 0, 'pixdim': (1.0,) * 8, 'qform_code': 0, 'sform_code': 0, 'quatern_b': 0.0, 'quatern_c': 0.0,
                    'quatern_d': 0.0, 'qoffset_x': 0.0, 'qoffset_y': 0.0, 'qoffset_z': 0.0, 'srow_x': (0.0,) * 4, 'srow_y': (0.0,) * 4,
                    'srow_z': (0.0,) * 4}                 # what write_nifti writes without a geometry: unit voxels, qfac 1, no orientation
GZIP_LEVEL = 1                                    # write_nifti's deflate level (profiles/export_bench.txt, DESIGN.md: the host deflate bounds a file's write)
EXPORT_DTYPES = {2: torch.uint8, 4: torch.int16, 16: torch.float32}      # the NIfTI datatypes units='scan' writes in; any other file: float32


def read_nifti(path):
    """-> (raw, info) of a single-file NIfTI-1 (.nii or .nii.gz).  raw: the voxel array in FILE order, unscaled and in the file's dtype, shape
    (D, W, H) C-contiguous (the first NIfTI axis is the fastest): a view of the bytes read, copied only to swap the bytes of a file of the other
    byte order; `raw.transpose(2, 1, 0)` is the (H, W, D) array of nibabel.  info: shape (H, W, D), datatype, slope, inter (a scl_slope of 0 or
    NaN means 1 and 0), pixdim (3 floats), byteswapped, geometry: the header fields that place the voxels in space, parsed in the file's byte order --
    dim_info, xyzt_units, pixdim (all 8, qfac first), qform_code, sform_code, quatern_b/c/d, qoffset_x/y/z, srow_x/y/z (4 floats each) --, the dict
    write_nifti takes.  Anything else than a 3-D volume of a supported datatype raises ValueError naming the
    header field and its value."""
    with (gzip.open(path, 'rb') if str(path).endswith('.gz') else open(path, 'rb')) as f:
        buf = f.read()
    if len(buf) < HEADER_BYTES:
        raise ValueError(f'{path}: sizeof_hdr: the file holds {len(buf)} bytes, a NIfTI-1 header takes {HEADER_BYTES}')
    size_le, size_be = struct.unpack_from('<i', buf, 0)[0], struct.unpack_from('>i', buf, 0)[0]
    if size_le == HEADER_BYTES:
        e = '<'
    elif size_be == HEADER_BYTES:
        e = '>'
    else:
        raise ValueError(f'{path}: sizeof_hdr {size_le}: {HEADER_BYTES} wanted (in either byte order)')
    dim = struct.unpack_from(e + '8h', buf, 40)
    datatype, bitpix = struct.unpack_from(e + '2h', buf, 70)
    pixdim = struct.unpack_from(e + '8f', buf, 76)
    vox_offset, slope, inter = struct.unpack_from(e + '3f', buf, 108)
    magic = bytes(buf[344:348])
    if magic != b'n+1\0':
        raise ValueError(f'{path}: magic {magic!r}: only the single-file form n+1 is read')
    if dim[0] not in (3, 4) or any(d != 1 for d in dim[4:dim[0] + 1]):
        raise ValueError(f'{path}: dim {dim}: three axes wanted (a fourth of extent 1 is accepted)')
    if min(dim[1:4]) < 1:
        raise ValueError(f'{path}: dim {dim}: every extent must be at least 1')
    if datatype not in NIFTI_DTYPES:
        raise ValueError(f'{path}: datatype {datatype}: one of {sorted(NIFTI_DTYPES)} (uint8, int16, int32, float32, float64, uint16)')
    if not vox_offset >= 352 or vox_offset != int(vox_offset):
        raise ValueError(f'{path}: vox_offset {vox_offset}: a whole number >= 352 wanted')
    dt = np.dtype(e + NIFTI_DTYPES[datatype])
    H, W, D = (int(d) for d in dim[1:4])
    if len(buf) < int(vox_offset) + H * W * D * dt.itemsize:
        raise ValueError(f'{path}: dim {dim}: {H * W * D} voxels of {dt.itemsize} bytes from vox_offset {int(vox_offset)} need '
                         f'{int(vox_offset) + H * W * D * dt.itemsize} bytes, the file holds {len(buf)}')
    raw = np.frombuffer(buf, dtype=dt, count=H * W * D, offset=int(vox_offset)).reshape(D, W, H)
    swapped = e != ('<' if sys.byteorder == 'little' else '>')
    if not dt.isnative:
        raw = raw.astype(dt.newbyteorder('='))
    if slope == 0 or math.isnan(slope):
        slope, inter = 1.0, 0.0
    qs = struct.unpack_from(e + '2h18f', buf, 252)                     # qform_code, sform_code, quatern_b/c/d, qoffset_x/y/z, srow_x/y/z
    geometry = {'dim_info': buf[39], 'xyzt_units': buf[123], 'pixdim': tuple(float(p) for p in pixdim),
                'qform_code': int(qs[0]), 'sform_code': int(qs[1])}
    geometry.update(zip(GEOMETRY_FLOATS, (float(v) for v in qs[2:8])))
    geometry.update(srow_x=tuple(float(v) for v in qs[8:12]), srow_y=tuple(float(v) for v in qs[12:16]), srow_z=tuple(float(v) for v in qs[16:20]))
    return raw, {'shape': (H, W, D), 'datatype': int(datatype), 'slope': float(slope), 'inter': float(inter),
                 'pixdim': tuple(float(p) for p in pixdim[1:4]), 'byteswapped': swapped, 'geometry': geometry}


def write_nifti(path, voxels, geometry=None, descrip=b'mrdis', compresslevel=GZIP_LEVEL):
    """a single-file NIfTI-1 (.nii, or .nii.gz for a path that ends in .gz) on struct and gzip alone: the inverse of read_nifti.  voxels: a C-contiguous
    (D, W, H) numpy array -- FILE order, the first NIfTI axis the fastest, what read_nifti returns and hip.export_volume makes -- of a datatype in
    NIFTI_DTYPES.  Always little-endian; sizeof_hdr 348, vox_offset 352 (four zero extension bytes), dim [3, H, W, D, 1, 1, 1, 1], datatype / bitpix of
    the array, scl_slope 1, scl_inter 0, magic n+1.  geometry: the dict of read_nifti's info['geometry'] (dim_info, xyzt_units, pixdim with qfac first,
    qform_code, sform_code, quatern_b/c/d, qoffset_x/y/z, srow_x/y/z); None: pixdim 1 (qfac 1), both codes 0.  A .gz goes through
    gzip.GzipFile(mtime=0) with an empty name: two writes of one volume give the same bytes.  compresslevel: GZIP_LEVEL, see DESIGN.md on how it was
    chosen.  ValueError names the argument that is wrong."""
    if not isinstance(voxels, np.ndarray) or voxels.ndim != 3:
        raise ValueError(f'voxels: a 3-D (D, W, H) numpy array wanted, got {type(voxels).__name__} of shape {getattr(voxels, "shape", None)}')
    code = {np.dtype(k): c for c, k in NIFTI_DTYPES.items()}.get(voxels.dtype.newbyteorder('='))
    if code is None:
        raise ValueError(f'voxels: dtype {voxels.dtype}: one of {sorted(NIFTI_DTYPES.values())} wanted')
    if not voxels.flags['C_CONTIGUOUS']:
        raise ValueError(f'voxels: a C-contiguous array wanted, got strides {voxels.strides} for shape {voxels.shape}')
    if max(voxels.shape) > 32767:
        raise ValueError(f'voxels: shape {voxels.shape}: an extent does not fit the int16 dim field')
    descrip = bytes(descrip)
    if len(descrip) > 79:
        raise ValueError(f'descrip: {len(descrip)} bytes, at most 79 fit')
    g = dict(DEFAULT_GEOMETRY)
    if geometry is not None:
        unknown = set(geometry) - set(g)
        if unknown or len(geometry.get('pixdim', g['pixdim'])) != 8 or any(len(geometry.get(k, g[k])) != 4 for k in ('srow_x', 'srow_y', 'srow_z')):
            raise ValueError(f'geometry: the keys of read_nifti\'s info["geometry"] wanted (pixdim of 8, srow_x/y/z of 4), got {geometry!r}')
        g.update(geometry)
    D, W, H = voxels.shape
    hdr = bytearray(HEADER_BYTES + 4)
    struct.pack_into('<i', hdr, 0, HEADER_BYTES)
    hdr[39] = int(g['dim_info']) & 255
    struct.pack_into('<8h', hdr, 40, 3, H, W, D, 1, 1, 1, 1)
    struct.pack_into('<2h', hdr, 70, code, voxels.dtype.itemsize * 8)
    struct.pack_into('<8f', hdr, 76, *g['pixdim'])
    struct.pack_into('<3f', hdr, 108, float(HEADER_BYTES + 4), 1.0, 0.0)
    hdr[123] = int(g['xyzt_units']) & 255
    hdr[148:148 + len(descrip)] = descrip
    struct.pack_into('<2h18f', hdr, 252, int(g['qform_code']), int(g['sform_code']), *(g[k] for k in GEOMETRY_FLOATS), *g['srow_x'], *g['srow_y'], *g['srow_z'])
    hdr[344:348] = b'n+1\0'
    data = voxels.astype(voxels.dtype.newbyteorder('<'), copy=False)
    if str(path).endswith('.gz'):
        with open(path, 'wb') as raw_file, gzip.GzipFile(filename='', mode='wb', compresslevel=compresslevel, fileobj=raw_file, mtime=0) as f:
            f.write(hdr)
            f.write(memoryview(data).cast('B'))
    else:
        with open(path, 'wb') as f:
            f.write(hdr)
            f.write(memoryview(data).cast('B'))
    return path


def to_device(raw, device):
    """a numpy volume goes to the device as it is, in its own dtype; a device tensor is returned unchanged"""
    if isinstance(raw, torch.Tensor):
        return raw
    raw = np.asarray(raw)
    if not raw.dtype.isnative:
        raw = raw.astype(raw.dtype.newbyteorder('='))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)          # a view of a file's bytes is read-only; it is only ever read
        return torch.from_numpy(raw).to(device)


def prep_stats(raw, crop, slope=1.0, inter=0.0, order='file', inner=BRATS_INNER, device='cuda:0'):
    """hip.prep_stats; a numpy `raw` is uploaded to `device` first"""
    return hip.prep_stats(to_device(raw, device), crop, slope, inter, order, inner)


def prep_write(raw, stats, kind, crop, layout, slope=1.0, inter=0.0, order='file', out=None):
    """hip.prep_write; a numpy `raw` is uploaded to the device of `stats` first"""
    return hip.prep_write(to_device(raw, stats.device), stats, kind, crop, layout, slope, inter, order, out)


def prep_volume(raw, kind, crop, layout, slope=1.0, inter=0.0, order='file', inner=BRATS_INNER, out=None, device='cuda:0'):
    """-> (fp32 store volume, stats): prep_stats then prep_write on one upload, with no host read in between or after"""
    raw = to_device(raw, device)
    stats = hip.prep_stats(raw, crop, slope, inter, order, inner)
    return hip.prep_write(raw, stats, kind, crop, layout, slope, inter, order, out), stats


def subject_files(raw_path, subj, contrasts=None):
    """{store key: path} of the files `raw_path/<subj>/<subj>_{t1,t1ce,t2,flair,seg}.nii[.gz]` that exist (.nii.gz first), `seg` always among
    the names looked for"""
    found = {}
    for key, suffix in BRATS_FILES:
        if contrasts is not None and key != 'seg' and key not in contrasts:
            continue
        for ext in ('.nii.gz', '.nii'):
            p = os.path.join(raw_path, subj, f'{subj}_{suffix}{ext}')
            if os.path.exists(p):
                found[key] = p
                break
    return found


def build_store_from_raw(raw_path, device, store_cls=VolumeStore, norm_type='zscore', crop=BRATS_CROP, contrasts=None, subjects=None, log=print):
    """-> (store, subjects kept).  Walks the sub-directories of `raw_path` (or `subjects`) in sorted order; per subject the raw volumes are uploaded,
    the statistics of all of them queued and read with ONE synchronisation, the rule of :80 applied -- a shape different from the first accepted
    volume's, vmax == 0 or more than 100000 NaNs inside the inner planes drops the subject whole, with one log line -- and the accepted volumes
    written straight into the store: `norm_type` 'mean' -> v / norm, anything else -> the z-score with -10 outside the brain; `seg` -> the labels.
    The store's layout follows `store_cls` ((D, H', W') for VolumeStore, (H', W', D) for a VolumeStore3D).  What the way back needs stays on the
    store as `store.raw_meta` = {'crop', 'shape' (the full H, W, D), 'norm_type' ('zscore' | 'mean'), 'subjects': {subj: {key: {'stats' (the device
    tensor of prep_stats), 'stats_host' (the row the synchronisation read), 'geometry', 'datatype', 'slope', 'inter'}}}}: no further synchronisation."""
    from .data3d import VolumeStore3D
    device = torch.device(device)
    store = store_cls(device)
    layout = 'hwd' if isinstance(store, VolumeStore3D) else 'dhw'
    kind = 'mean' if norm_type == 'mean' else 'zscore'
    if subjects is None:
        subjects = [s for s in os.listdir(raw_path) if os.path.isdir(os.path.join(raw_path, s))]
    shape, kept = None, []
    meta = store.raw_meta = {'crop': tuple(tuple(int(v) for v in c) for c in crop), 'shape': None, 'norm_type': kind, 'subjects': {}}
    for subj in sorted(subjects):
        files = subject_files(raw_path, subj, contrasts)
        if not files:
            continue                                                   # an empty directory (:37-38)
        vols = []
        for key, path in files.items():
            raw, info = read_nifti(path)
            vols.append((key, to_device(raw, device), info))
        want = shape or vols[0][2]['shape']
        why = [f'{key} shape {info["shape"]} != {want}' for key, _, info in vols if info['shape'] != want]
        if not why:
            stats = [hip.prep_stats(t, crop, info['slope'], info['inter'], 'file', BRATS_INNER) for _, t, info in vols]
            host = torch.stack(stats).cpu().numpy()                   # the subject's one synchronisation
            why = [f'{key} max {row[3]:g}, {int(row[4])} NaNs inside' for (key, _, _), row in zip(vols, host)
                   if row[3] == 0 or row[4] > MAX_INNER_NAN]
        if why:
            log(f'{subj}: dropped ({"; ".join(why)})')
            continue
        for (key, t, info), st in zip(vols, stats):
            store.add_device(f'{subj}/{key}', hip.prep_write(t, st, 'label' if key == 'seg' else kind, crop, layout, info['slope'], info['inter'], 'file'))
        # what the way back needs (save_nifti): the statistics where they are and as the synchronisation above already read them, and each header
        meta['subjects'][subj] = {key: {'stats': st, 'stats_host': row, 'geometry': info['geometry'], 'datatype': info['datatype'],
                                        'slope': info['slope'], 'inter': info['inter']} for (key, _, info), st, row in zip(vols, stats, host)}
        shape = meta['shape'] = want
        kept.append(subj)
    return store, kept


def save_nifti(path, vol, store, subj, key=None, units='store', layout='hwd', log=print):
    """writes a volume of subject `subj`, in the store's cropped geometry and on the device, as a NIfTI file that overlays on the subject's scans:
    hip.export_volume (one launch), one device-to-host copy, write_nifti.  vol: (H', W', D) for layout 'hwd' (label volumes, synthesized volumes, a
    VolumeStore3D) or (D, H', W') for 'dhw' (a VolumeStore); or a (P, ...) stack with a list of P paths, still one launch.  key None (or 'seg'): a
    label volume; else the contrast the volume shows.  store: one that build_store_from_raw made (it keeps the crop, the headers and the statistics
    in store.raw_meta); any other raises ValueError.
    THIS PACKAGE'S CONVENTIONS (the reference writes no files):
      1. geometry: labels take the geometry of the subject's `seg` file if it has one, a contrast that of its own file; otherwise both take that of
         the subject's first file in BRATS_FILES order;
      2. labels are written uint8, copied, 0 outside the crop;
      3. units 'store': float32, copied, the store's background outside the crop: -10 for z-score, 0 for mean;
      4. units 'scan': the inverse of the rule that made the store, with that file's own statistics, in that file's datatype (float32 if it is
         neither int16, uint8 nor float32), 0 outside the crop.  Values are v = raw slope + inter and the file written says slope 1.  What the
         forward rule destroyed stays destroyed: v <= 0 comes back as 0.  A contrast the subject has no file of has no statistics: it is written as
         units 'store', with one log line;
      5. a store without raw_meta raises ValueError: the export needs data_source raw."""
    meta = getattr(store, 'raw_meta', None)
    if meta is None:
        raise ValueError('save_nifti: store keeps no raw_meta: NIfTI export needs a store built with data_source raw (build_store_from_raw)')
    files = meta['subjects'].get(subj)
    if not files:
        raise ValueError(f'save_nifti: subj {subj!r} is not among the subjects the store was built from')
    if units not in ('store', 'scan'):
        raise ValueError(f"save_nifti: units {units!r}: 'store' or 'scan'")
    label = key is None or key == 'seg'
    own = files.get('seg' if label else key)
    geometry = (own or next(files[k] for k, _ in BRATS_FILES if k in files))['geometry']
    zscore = meta['norm_type'] != 'mean'
    if label:
        kind, stats, fill, dtype = 'copy', None, 0.0, torch.uint8
        if vol.dtype not in hip.EXPORT_SRC_DTYPES:
            vol = vol.to(torch.uint8)
    elif units == 'scan' and own is not None:
        kind, stats, fill, dtype = 'unzscore' if zscore else 'unmean', own['stats'], 0.0, EXPORT_DTYPES.get(own['datatype'], torch.float32)
    else:
        if units == 'scan':
            log(f'{subj}: no {key} file, so no statistics: written in store units')
        kind, stats, fill, dtype = 'copy', None, -10.0 if zscore else 0.0, torch.float32
    paths = [path] if isinstance(path, (str, os.PathLike)) else list(path)
    if (vol.dim() == 4) != (not isinstance(path, (str, os.PathLike))) or (vol.dim() == 4 and len(paths) != vol.shape[0]):
        raise ValueError(f'save_nifti: path: one path for a volume, a list of P for a (P, ...) stack; got {len(paths)} for shape {tuple(vol.shape)}')
    (h0, h1), (w0, w1) = meta['crop']
    Hc, Wc, D = tuple(vol.shape[-3:]) if layout == 'hwd' else tuple(vol.shape[i] for i in (-2, -1, -3))
    if (Hc + h0 + h1, Wc + w0 + w1, D) != tuple(meta['shape']):
        raise ValueError(f'save_nifti: vol {tuple(vol.shape)} in layout {layout!r} with crop {meta["crop"]} is not the scans\' {meta["shape"]}')
    out = hip.export_volume(vol, meta['crop'], layout, kind, stats, fill, dtype).cpu().numpy()
    for p, v in zip(paths, out if vol.dim() == 4 else out[None]):
        write_nifti(p, v, geometry)
    return paths


def export_store_volume(store, key, path, units='scan', log=print):
    """writes the stored volume `key` = 'subject/contrast' (or 'subject/seg') itself, of a VolumeStore or a VolumeStore3D, with save_nifti: with
    units 'scan' the file holds the scan the volume was made from, v = raw slope + inter -- max(v, 0) under the z-score, which put every v <= 0 at
    -10; every v under the mean rule -- inside the crop: the round trip that checks a store."""
    from .data3d import VolumeStore3D
    if key not in store:
        raise ValueError(f'export_store_volume: key {key!r} is not in the store')
    subj, _, contrast = key.rpartition('/')
    return save_nifti(path, store.vols[key], store, subj, contrast, units, 'hwd' if isinstance(store, VolumeStore3D) else 'dhw', log)[0]


def fold_split(subjects, seed=10):
    """:100-139 -> five (train, val, test) triples of id lists: the ids shuffled by np.random.RandomState(seed) -- the permutation of the
    reference's np.random.seed(10); np.random.shuffle, without touching the global stream --, fold f tests ids [f k, (f + 1) k) with
    k = int(0.2 n), validates on the first int(0.1 len) of the rest, and ids containing 'Validation' leave all three."""
    ids = [str(s) for s in subjects]
    np.random.RandomState(seed).shuffle(ids)
    k = int(0.2 * len(ids))
    keep = lambda part: [s for s in part if 'Validation' not in s]
    folds = []
    for f in range(5):
        test = ids[f * k:(f + 1) * k]
        rest = ids[:f * k] + ids[(f + 1) * k:]
        nv = int(0.1 * len(rest))
        folds.append((keep(rest[nv:]), keep(rest[:nv]), keep(test)))
    return folds


def write_fold_lists(subjects, out_dir, dataset='BraTS', seed=10, slices=(50, 105)):
    """:100-146: writes fold_<dataset>_{f}_{train,val,test}_noval.txt (`subject slice` lines for slices[0] <= slice < slices[1]) and
    fold_<dataset>_3d_{f}_{train,val,test}_noval.txt (one id per line) for the five folds of fold_split -> the list of paths written"""
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for f, parts in enumerate(fold_split(subjects, seed)):
        for name, part in zip(('train', 'val', 'test'), parts):
            p2 = os.path.join(out_dir, f'fold_{dataset}_{f}_{name}_noval.txt')
            with open(p2, 'w') as ft:
                for s in part:
                    for i in range(int(slices[0]), int(slices[1])):
                        ft.write(f'{s} {i}\n')
            p3 = os.path.join(out_dir, f'fold_{dataset}_3d_{f}_{name}_noval.txt')
            with open(p3, 'w') as ft:
                for s in part:
                    ft.write(s + '\n')
            paths += [p2, p3]
    return paths


def ensure_fold_lists(subjects, data_path, names, dataset='BraTS', slices=(50, 105)):
    """writes the fold lists under `data_path` unless every file of `names` is already there"""
    if not all(os.path.exists(os.path.join(data_path, n)) for n in names):
        write_fold_lists(subjects, data_path, dataset=dataset, slices=slices)
