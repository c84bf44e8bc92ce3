"""Intensity augmentation of the 3-D training patches on the device (csrc/mrdis_tone.hip): Gaussian blur, contrast, gamma and additive noise
on the gathered or warped inputs; reached as patch3d.patch_blur / patch_stats / patch_tone / patch_intensify / blur_taps / pack_tone.  THIS
PACKAGE'S CONVENTIONS -- the reference has no such augmentation (include/mrdis.h has the full rule):

  * a voxel is background iff it equals -10.0 exactly; background voxels stay -10 and enter no sum.  Targets and `mask` are not touched
  * blur: a 9-tap (radius 4) separable normalised convolution over the tissue voxels, passes along d, w, h, fp32 fmaf chains; the patch border
    renormalises as the background does.  taps g[t] = exp(-t^2 / (2 sigma^2)) / sum, float64 on the host, rounded once (`blur_taps`)
  * statistics of the blurred patch per (item, contrast) over tissue: min, max, mean (float64 sum), count
  * contrast: v = clamp(mean + (v - mean) f, lo, hi); gamma (only if hi > lo): t = (v - lo) / (hi - lo), t = t ** gamma, or 1 - (1 - t) ** gamma
    for the inverted curve, v = lo + t (hi - lo); noise: v += std z, z from Philox4x32-10 on (flat voxel index, contrast) under the row's seed:
    the sum of the 16 output bytes, centred and scaled to variance 1
  * an item or contrast without a flag comes out of all three calls bit for bit as it went in

    table[b, col:col + TONE_EXTRA(M)] = pack_tone(seed, flags, sigma, f, gamma, std)        # per item; flags (M,) of BLUR | CONTRAST | ...
    y = patch_intensify(x, table, col, M)                                                   # = patch_blur, patch_stats, patch_tone

Every per-batch value comes from the table, so the calls replay from a captured graph with the next batch's table.
"""
import numpy as np
import torch

from . import hip

BLUR, CONTRAST, GAMMA, INVERT, NOISE = 1, 2, 4, 8, 16         # include/mrdis.h MRDIS_TONE_*
RADIUS = 4                                                    # taps on either side of the centre
SIGMA_MAX = 1.0                                               # the radius is at least four sigmas


def TONE_EXTRA(M):
    """words of a table row that the three calls read at `col`: the seed, then five per contrast"""
    return 1 + 5 * int(M)


def blur_taps(sigma):
    """-> (5,) float32: g[t] = exp(-t^2 / (2 sigma^2)) / (g0 + 2 sum_{t = 1 .. 4} g[t]), in float64, rounded once"""
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f'blur_taps: sigma {sigma!r}: a number') from None
    if not np.isfinite(sigma) or not 0 < sigma <= SIGMA_MAX:
        raise ValueError(f'blur_taps: sigma {sigma!r}: above 0 and at most {SIGMA_MAX} (the tap radius is {RADIUS})')
    t = np.arange(RADIUS + 1, dtype=np.float64)
    g = np.exp(-t * t / (2.0 * sigma * sigma))
    return (g / (g[0] + 2.0 * g[1:].sum())).astype(np.float32)


def pack_tone(seed, flags, sigma, f, gamma, std):
    """the TONE_EXTRA(M) table words of one item -> (1 + 5 M,) int64 numpy array.  seed: two uint32 (lo, hi); flags: M integers of BLUR |
    CONTRAST | GAMMA | INVERT | NOISE; sigma, f, gamma, std: M numbers each, rounded once to fp32 (sigma is read only where BLUR is set and
    goes in as its five taps; a contrast without BLUR gets zero taps)."""
    flags = [int(v) for v in flags]
    M = len(flags)
    vals = [np.asarray(v, dtype=np.float64).reshape(-1) for v in (sigma, f, gamma, std)]
    if M < 1 or any(len(v) != M for v in vals) or any(not 0 <= v < 32 for v in flags) or len(seed) != 2:
        raise ValueError(f'pack_tone: a seed of two uint32, M flags in 0 .. 31 and four lists of M numbers, got {seed!r}, {flags!r}, {[v.tolist() for v in vals]}')
    half = np.zeros(2 + 10 * M, dtype=np.uint32)
    half[0], half[1] = np.uint32(seed[0]), np.uint32(seed[1])
    for m in range(M):
        h = half[2 + 10 * m:12 + 10 * m]
        h[0] = flags[m]
        if flags[m] & BLUR:
            h[1:6] = blur_taps(vals[0][m]).view(np.uint32)
        h[6:9] = np.array([vals[1][m], vals[2][m], vals[3][m]], dtype=np.float64).astype(np.float32).view(np.uint32)
    half = half.astype(np.uint64)
    return (half[0::2] | (half[1::2] << np.uint64(32))).view(np.int64)


# ---------------------------------------------------------------- the binding (the ctypes table is hip._SIGS)
# Every tensor a kernel gets is checked here first (hip._want / hip._refuse: MrdisError before any launch).
def _patches(x, what, M):
    """x: (B, M, PH, PW, PD) fp32 dense channels-last-3d -> (B, PH, PW, PD)"""
    if isinstance(M, bool) or not isinstance(M, int) or not 1 <= M <= 64: hip._refuse(f'{what}: M contrasts in 1 .. 64', 'arg', M)
    B, _, PH, PW, PD = hip._want(x, f'{what}: x', torch.float32, ('B', M, 'PH', 'PW', 'PD'), cl=True)
    if not 1 <= B <= 65535 or min(PH, PW, PD) < 1 or PH * PW * PD >= 1 << 31: hip._refuse(f'{what}: 1 .. 65535 patches of 1 .. 2^31 - 1 voxels', 'arg', x)
    return B, PH, PW, PD


def _block(table, what, col, B, M, device):
    if isinstance(col, bool) or not isinstance(col, int) or col < 0: hip._refuse(f'{what}: col, the word offset of the block in a row, >= 0', 'arg', col)
    _, ld = hip._want(table, f'{what}: table', torch.int64, (B, 'ld'), device)
    if ld < col + TONE_EXTRA(M): hip._refuse(f'{what}: table rows of at least col + 1 + 5 M = {col + TONE_EXTRA(M)} words', 'vec', table)
    return ld


def patch_blur(x, table, col, M):
    """x (B, M, PH, PW, PD) fp32 channels-last-3d (what patch_gather / patch_warp return), table (B, >= col + TONE_EXTRA(M)) int64 on the
    device -> y, a new tensor of x's layout: the contrasts whose BLUR flag is set blurred over their tissue voxels, every other one x bit for
    bit (include/mrdis.h mrdis_patch_blur).  Two launches at M == 4, three otherwise."""
    lib = hip.load()
    B, PH, PW, PD = _patches(x, 'patch_blur', M)
    ld = _block(table, 'patch_blur', col, B, M, x.device)
    y = torch.empty_like(x)                                          # (preserve_format keeps the dense channels-last-3d strides)
    if y.stride() != x.stride(): hip._refuse('patch_blur: an output of the strides of x', 'dense', x, y)
    nbytes = hip._ws_bytes(lib.mrdis_patch_blur_workspace, B, M, PH, PW, PD)
    ws = hip._ws(nbytes, x.device)
    hip._chk(lib.mrdis_patch_blur(hip._ptr(x), hip._ptr(y), hip._ptr(table), ld, col, B, M, PH, PW, PD, hip._ptr(ws), nbytes, hip._stream()), 'patch_blur')
    return y


def patch_stats(x, M):
    """x (B, M, PH, PW, PD) fp32 channels-last-3d -> stats (B, M, 4) int32 on the device: the fp32 bits of the minimum, the maximum and the
    mean over the tissue voxels (those not equal to -10) of every (item, contrast) and their count; zeros where there is none
    (include/mrdis.h mrdis_patch_stats).  Two launches; the same bits on every run."""
    lib = hip.load()
    B, PH, PW, PD = _patches(x, 'patch_stats', M)
    stats = torch.empty((B, M, 4), dtype=torch.int32, device=x.device)
    nbytes = hip._ws_bytes(lib.mrdis_patch_stats_workspace, B, M, PH, PW, PD)
    ws = hip._ws(nbytes, x.device)
    hip._chk(lib.mrdis_patch_stats(hip._ptr(x), hip._ptr(stats), B, M, PH, PW, PD, hip._ptr(ws), nbytes, hip._stream()), 'patch_stats')
    return stats


def patch_tone(x, stats, table, col, M):
    """contrast, gamma and noise IN PLACE on the tissue voxels of x (B, M, PH, PW, PD) fp32 channels-last-3d, per contrast and only where the
    flag of the step is set, with the `stats` (B, M, 4) int32 of `patch_stats` (include/mrdis.h mrdis_patch_tone).  -> x.  One launch."""
    lib = hip.load()
    B, PH, PW, PD = _patches(x, 'patch_tone', M)
    hip._want(stats, 'patch_tone: stats', torch.int32, (B, M, 4), x.device)
    ld = _block(table, 'patch_tone', col, B, M, x.device)
    hip._chk(lib.mrdis_patch_tone(hip._ptr(x), hip._ptr(stats), hip._ptr(table), ld, col, B, M, PH, PW, PD, hip._stream()), 'patch_tone')
    return x


def patch_intensify(x, table, col, M):
    """blur, statistics, then contrast, gamma and noise of the gathered inputs x under the table block at `col` -> a new tensor (x is left
    as it was).  The three calls `patch_blur`, `patch_stats`, `patch_tone`: counted as 'patchblur', 'patchstats', 'patchtone', one each."""
    y = patch_blur(x, table, col, M)
    return patch_tone(y, patch_stats(y, M), table, col, M)
