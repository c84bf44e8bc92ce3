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


def read_nifti(path):
    """-> (raw, info) of a single-file NIfTI-1 (.nii or .nii.gz).  raw: the voxel array in FILE order, unscaled and in the file's dtype, shape
    (D, W, H) C-contiguous (the first NIfTI axis is the fastest): a view of the bytes read, copied only to swap the bytes of a file of the other
    byte order; `raw.transpose(2, 1, 0)` is the (H, W, D) array of nibabel.  info: shape (H, W, D), datatype, slope, inter (a scl_slope of 0 or
    NaN means 1 and 0), pixdim (3 floats), byteswapped.  Anything else than a 3-D volume of a supported datatype raises ValueError naming the
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
    return raw, {'shape': (H, W, D), 'datatype': int(datatype), 'slope': float(slope), 'inter': float(inter),
                 'pixdim': tuple(float(p) for p in pixdim[1:4]), 'byteswapped': swapped}


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
    The store's layout follows `store_cls` ((D, H', W') for VolumeStore, (H', W', D) for a VolumeStore3D)."""
    from .data3d import VolumeStore3D
    device = torch.device(device)
    store = store_cls(device)
    layout = 'hwd' if isinstance(store, VolumeStore3D) else 'dhw'
    kind = 'mean' if norm_type == 'mean' else 'zscore'
    if subjects is None:
        subjects = [s for s in os.listdir(raw_path) if os.path.isdir(os.path.join(raw_path, s))]
    shape, kept = None, []
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
        shape = want
        kept.append(subj)
    return store, kept


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
