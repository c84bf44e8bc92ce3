"""Rotated and zoomed training patches for the 3-D nets on the device (csrc/mrdis_warp.hip); reached as patch3d.patch_warp and
patch3d.warp_matrix.  THIS PACKAGE'S CONVENTIONS -- the reference has no spatial augmentation:

  * A = (R_h R_w R_d) / zoom in float64 on the host, R_x the right-handed rotation about axis x of (h, w, d) coordinates, rounded ONCE to
    Q16: a[r][c] = floor(A[r][c] 65536 + 0.5).  A zoom above 1 magnifies: the patch samples a smaller region.
  * the source coordinate of output voxel o, all integers in units of 2^-17 voxel, 64-bit; o' is o after the flip rule of patch_gather,
    origin the (h0, w0, d0) of patch_origins, P = (PH, PW, PD):
        s[r] = ((2 origin[r] + P[r] - 1) << 16) + sum_c a[r][c] (2 o'[c] - (P[c] - 1))
        floor index i0 = s >> 17,  fraction f = s & (2^17 - 1),  nearest index = (s + 2^16) >> 17
    -- a rotation about the centre of the unwarped patch, so a foreground-centred patch keeps its tumour voxel at the centre
  * i0, i0 + 1 and the nearest index are clamped per axis into the volume (edge replication); nothing is padded
  * targets: the raw label at the nearest index, then the relabel and region-channel rules of patch_gather.  Exact.
  * inputs, per contrast (an absent one reads 0 everywhere), m0 the whole-volume minimum of patch_gather's `== min()` rule: with the augment
    bit, exactly -10 where the voxel at the nearest index equals m0; elsewhere every one of the eight corners that equals m0 takes the nearest
    voxel's value (the background marker never bleeds into tissue), the corners are interpolated trilinearly along d, then w, then h with
    the weights f / 2^17 (exact in fp32), and x * scale + shift follows.  Without the augment bit: the interpolated raw corners.
  * a row with the WARP flag clear comes out as patch_gather gives it, bit for bit

    a = warp_matrix((10.0, -20.0, 30.0), 1.2)                       # (3, 3) int32
    table[b, 2 * M + 1] |= patch3d.WARP; table[b, 2 * M + 7:2 * M + 12] = pack_warp(a)
    inputs, mask = patch_warp(table, origins, M, (H, W, D), (PH, PW, PD))
    targets = patch_warp(table, origins, M, (H, W, D), (PH, PW, PD), targets=True, K=3, relabel=True)
"""
import numpy as np

from . import hip, patch3d


def warp_matrix(angles_deg, zoom):
    """-> (3, 3) int32 numpy array: a[r][c] = floor(A[r][c] 65536 + 0.5), A = (R_h R_w R_d) / zoom.  angles_deg: the rotations about the H, W
    and D axes in degrees; zoom > 0."""
    try:
        ah, aw, ad = (float(v) for v in angles_deg)
        zoom = float(zoom)
    except (TypeError, ValueError):
        raise ValueError(f'warp_matrix: angles {angles_deg!r}, zoom {zoom!r}: three angles in degrees and a number') from None
    if not all(np.isfinite([ah, aw, ad, zoom])) or not zoom > 0:
        raise ValueError(f'warp_matrix: finite angles and a zoom above 0, got {angles_deg!r}, {zoom!r}')

    def rot(axis, deg):
        c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))      # (cos of a quarter turn is 6e-17, which the Q16 rounding takes to 0)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]                 # the plane the axis turns, right-handed: i -> j
        R = np.eye(3, dtype=np.float64)
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        return R

    q = np.floor(rot(0, ah) @ rot(1, aw) @ rot(2, ad) / zoom * 65536.0 + 0.5)
    if np.abs(q).max() >= 2 ** 31:
        raise ValueError(f'warp_matrix: zoom {zoom!r} leaves the Q16 range')
    return q.astype(np.int32)


def pack_warp(a):
    """the five table words [2M+7 .. 2M+11] of a (3, 3) int32 matrix: row-major, two entries per 64-bit word, the low half first, the last high
    half zero -> (5,) int64 numpy array"""
    a = np.asarray(a)
    if a.shape != (3, 3) or a.dtype != np.int32:
        raise ValueError(f'pack_warp: a (3, 3) int32 matrix, got {a.dtype} {a.shape}')
    e = np.zeros(10, dtype=np.uint64)
    e[:9] = np.ascontiguousarray(a).reshape(-1).view(np.uint32)      # two's complement: a negative entry fills its own 32 bits only
    return (e[0::2] | (e[1::2] << np.uint64(32))).view(np.int64)


def patch_warp(table, origins, M, shape, patch, targets=False, K=0, relabel=False):
    """`patch3d.patch_gather` with the rotation and zoom of the rows whose WARP flag is set (include/mrdis.h mrdis_patch_warp).  table
    (B, >= 2 M + TABLE_EXTRA + WARP_EXTRA) int64 on the device: the rows of `patch_gather` followed by `pack_warp(warp_matrix(...))`.  Results
    and layouts are patch_gather's: inputs (B, M, PH, PW, PD) channels-last-3d and mask (B, M), or with `targets` the label patch
    (B, PH, PW, PD) / its K region channels (B, K, PH, PW, PD).  Every tensor is checked first: MrdisError before any launch.  One launch."""
    return patch3d._gather(hip.load().mrdis_patch_warp, 'patch_warp', patch3d.TABLE_EXTRA + patch3d.WARP_EXTRA, table, origins, M, shape, patch, targets, K, relabel)
