"""Patch sampling for the 3-D nets on the device (csrc/mrdis_patch.hip): random sub-volumes of the whole stored scan, a share of them centred
on a tumour voxel.  THIS PACKAGE'S CONVENTIONS -- the reference trains on one fixed depth crop and has no patch sampling:

  * pick(u, n) = (u n) >> 32 maps a uint32 draw onto 0 .. n - 1
  * uniform patch: h0 = pick(u_h, H - PH + 1), w0 and d0 likewise
  * foreground patch: the class is present[pick(u_class, len(present))] over the classes the subject has, in list order; the centre is the
    r-th voxel (r = pick(u_voxel, n_class), 0-based, increasing flat index (h W + w) D + d) of that class; h0 = clamp(hc - PH // 2, 0, H - PH),
    w0 and d0 likewise: the patch is clamped into the volume, never padded.  No label volume, no prefix table or no present class: uniform
  * evaluation: the centre patch ((H - PH) // 2, (W - PW) // 2, (D - PD) // 2)
  * the augmentation's `== min()` rule compares with the minimum of the WHOLE stored volume, not of the patch

    prefix = fg_prefix(seg, (1, 2, 4))                              # once per subject: (nblk + 1, K) int32
    origins = patch_origins(table, M, (H, W, D), (PH, PW, PD), (1, 2, 4))
    inputs, mask = patch_gather(table, origins, M, (H, W, D), (PH, PW, PD))
    targets = patch_gather(table, origins, M, (H, W, D), (PH, PW, PD), targets=True, K=3, relabel=True)

The table is data3d.VolumeLoader3D.patch_table's: one row of 2 M + TABLE_EXTRA 64-bit words per sample (include/mrdis.h).  Every draw comes
from it, so the three launches of a batch replay from a captured graph with the next batch's table.

Rotation and zoom of the patches (`patch_warp`, `warp_matrix`, `pack_warp`; rows WARP_EXTRA words longer, flag WARP): warp3d.py, whose
docstring has the conventions.  warp3d imports this module for its checks; the package binds its three functions here under their names.
"""
import torch

from . import hip

BLOCK = 1024                          # flat indices per counted block
MAX_CLASSES = hip.PATCH_MAX_CLASSES
TABLE_EXTRA = 7                       # words of a table row beyond the 2 M pointers
WARP_EXTRA = 5                        # further words of a row that `patch_warp` reads: the nine Q16 matrix entries, two per word
# the flag word [2M+1]
FLIP_H, AUG, FLIP_W, FLIP_D, FG, CENTRE, WARP = 1, 2, 4, 8, 16, 32, 64
FLIP_BITS = {'h': FLIP_H, 'w': FLIP_W, 'd': FLIP_D}


# ---------------------------------------------------------------- the binding (the ctypes table is hip._SIGS)
# Every tensor a kernel gets is checked here first, as hip.py checks its own (hip._want / hip._refuse: MrdisError before any launch).
def _class_list(classes, what, lo):
    try:
        vals = [int(c) for c in classes]
    except (TypeError, ValueError):
        raise hip.MrdisError(f'{what}: classes {classes!r}: a list of integers') from None
    if not lo <= len(vals) <= MAX_CLASSES or any(not 1 <= v <= 255 for v in vals) or len(set(vals)) != len(vals):
        raise hip.MrdisError(f'{what}: {lo} .. {MAX_CLASSES} distinct classes in 1 .. 255, got {vals}')
    return vals


def _geometry(what, M, shape, patch):
    try:
        M = int(M)
        H, W, D = (int(v) for v in shape)
        PH, PW, PD = (int(v) for v in patch)
    except (TypeError, ValueError):
        raise hip.MrdisError(f'{what}: M {M!r}, shape {shape!r}, patch {patch!r}: an integer and two triples of integers') from None
    if not 1 <= M <= 64 or min(H, W, D) < 1 or H * W * D >= 1 << 31:
        raise hip.MrdisError(f'{what}: unsupported geometry M {M}, volume {(H, W, D)}: M in 1 .. 64, H W D in 1 .. 2^31 - 1')
    if min(PH, PW, PD) < 1 or PH > H or PW > W or PD > D:
        raise hip.MrdisError(f'{what}: patch {(PH, PW, PD)} does not fit the volume {(H, W, D)}: no padding past the border')
    return M, H, W, D, PH, PW, PD


def _table(table, what, M, extra=TABLE_EXTRA):
    B, ld = hip._want(table, f'{what}: table', torch.int64, ('B', 'ld'))
    if ld < 2 * M + extra: hip._refuse(f'{what}: table rows of at least 2 M + {extra} = {2 * M + extra} words', 'vec', table)
    if not 1 <= B <= 65535: hip._refuse(f'{what}: 1 .. 65535 samples', 'arg', table)
    return B, ld


def _gather(entry, what, extra, table, origins, M, shape, patch, targets, K, relabel):
    """`patch_gather` and warp3d.patch_warp: every check of a gather over rows of 2 M + `extra` words, then the call (hip._gather3d)"""
    M, H, W, D, PH, PW, PD = _geometry(what, M, shape, patch)
    B, ld = _table(table, what, M, extra)
    hip._want(origins, f'{what}: origins', torch.int32, (B, 4), table.device)
    if not targets:
        if K: hip._refuse(f'{what}: K = 0 for the inputs', 'arg', K)
    elif isinstance(K, bool) or not isinstance(K, int) or not 0 <= K <= 64: hip._refuse(f'{what}: K region channels in 0 .. 64', 'arg', K)
    return hip._gather3d(entry, what, table, origins, M, (H, W, D), (PH, PW, PD), (PH, PW, PD), targets, K, relabel)


def fg_block_counts(seg, classes):
    """-> counts (nblk, K) int32 on seg's device (include/mrdis.h mrdis_fg_block_counts): counts[j][c] = the voxels equal to classes[c] among
    the flat indices [1024 j, 1024 j + 1024) of the label volume seg (H, W, D) fp32 contiguous.  1 .. 8 distinct classes.  One launch."""
    lib = hip.load()
    H, W, D = hip._want(seg, 'fg_block_counts: seg', torch.float32, ('H', 'W', 'D'))
    vals = _class_list(classes, 'fg_block_counts', 1)
    if min(H, W, D) < 1 or H * W * D >= 1 << 31: hip._refuse('fg_block_counts: H W D in 1 .. 2^31 - 1', 'arg', seg)
    counts = torch.empty(((H * W * D + BLOCK - 1) // BLOCK, len(vals)), dtype=torch.int32, device=seg.device)
    hip._chk(lib.mrdis_fg_block_counts(hip._ptr(seg), (hip._I * len(vals))(*vals), len(vals), hip._ptr(counts), H, W, D, hip._stream()), 'fg_block_counts')
    return counts


def fg_prefix(seg, classes):
    """-> the subject's prefix table (nblk + 1, K) int32: row j = the voxels of every class in the blocks before j, the last row the totals.
    One `fg_block_counts` launch and a running sum (torch, on the device): build time, once per subject."""
    counts = fg_block_counts(seg, classes)
    prefix = torch.zeros((counts.shape[0] + 1, counts.shape[1]), dtype=torch.int32, device=counts.device)
    prefix[1:] = torch.cumsum(counts, 0, dtype=torch.int32)
    return prefix


def patch_origins(table, M, shape, patch, classes=()):
    """-> origins (B, 4) int32 on the device = h0, w0, d0, index of the chosen class (-1 = uniform or centre) (include/mrdis.h
    mrdis_patch_origins).  table (B, >= 2 M + 7) int64 on the device; shape = (H, W, D) of the stored volumes, patch = (PH, PW, PD) <= shape;
    classes: the class values of the prefix tables the rows point to (none: every sample takes the uniform rule).  One launch."""
    lib = hip.load()
    M, H, W, D, PH, PW, PD = _geometry('patch_origins', M, shape, patch)
    B, ld = _table(table, 'patch_origins', M)
    vals = _class_list(classes, 'patch_origins', 0)
    origins = torch.empty((B, 4), dtype=torch.int32, device=table.device)
    hip._chk(lib.mrdis_patch_origins(hip._ptr(table), ld, hip._ptr(origins), (hip._I * len(vals))(*vals) if vals else None, len(vals), B, M, H, W, D, PH, PW, PD,
                                     hip._stream()), 'patch_origins')
    return origins


def patch_gather(table, origins, M, shape, patch, targets=False, K=0, relabel=False):
    """table and origins of `patch_origins` -> inputs (B, M, PH, PW, PD) channels-last-3d and mask (B, M), or with `targets` the label patch
    (B, PH, PW, PD) / its K region channels (B, K, PH, PW, PD) channels-last-3d (include/mrdis.h mrdis_patch_gather).  One launch."""
    return _gather(hip.load().mrdis_patch_gather, 'patch_gather', TABLE_EXTRA, table, origins, M, shape, patch, targets, K, relabel)
