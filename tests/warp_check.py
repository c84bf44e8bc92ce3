"""Plain-numpy oracle of the rotated and zoomed training patches (csrc/mrdis_warp.hip, patch3d.warp_matrix / patch_warp, data3d.py's
`patch_warp` keys): the rules restated independently, the coordinates in int64 (Python-integer semantics: floor shifts), the intensities in
float64 or -- the same statements, the same order -- in float32.  Labels, the -10 positions and the rows without a warp are compared exactly;
the interpolated intensities against the float64 evaluation within the bound the tests derive.  Used by tests/test_warp_cpu.py and
tests/test_gpu_warp.py; extends tests/patch3d_check.py."""
import numpy as np

import patch3d_check as chk

ONE = 1 << 17                # units per voxel of a source coordinate


def matrix(angles_deg, zoom):
    """(3, 3) int32: floor(A 65536 + 0.5), A = (R_h R_w R_d) / zoom, right-handed rotations about the H, W, D axes of (h, w, d) coordinates"""
    th, tw, td = (np.deg2rad(np.float64(v)) for v in angles_deg)
    ch, sh, cw, sw, cd, sd = np.cos(th), np.sin(th), np.cos(tw), np.sin(tw), np.cos(td), np.sin(td)
    Rh = np.array([[1, 0, 0], [0, ch, -sh], [0, sh, ch]], dtype=np.float64)
    Rw = np.array([[cw, 0, sw], [0, 1, 0], [-sw, 0, cw]], dtype=np.float64)
    Rd = np.array([[cd, -sd, 0], [sd, cd, 0], [0, 0, 1]], dtype=np.float64)
    A = (Rh @ Rw @ Rd) / np.float64(zoom)
    return np.floor(A * 65536.0 + 0.5).astype(np.int64).astype(np.int32)


IDENTITY = np.array([[65536, 0, 0], [0, 65536, 0], [0, 0, 65536]], dtype=np.int32)


def pack(a):
    """the five table words of a (3, 3) int32 matrix, by Python integers: entry e in bits 32 (e % 2) .. of word e // 2, two's complement in 32 bits"""
    words = [0] * 5
    for e, v in enumerate(int(x) for x in np.asarray(a).reshape(-1)):
        words[e // 2] |= (v & 0xffffffff) << (32 * (e % 2))
    return np.array([w - (1 << 64) if w >= 1 << 63 else w for w in words], dtype=np.int64)


def coords(a, o, patch, shape, flips=(False, False, False)):
    """-> (lo, hi, near, frac): four (3, PH, PW, PD) int64 arrays -- the clamped floor index, the clamped floor index + 1, the clamped nearest
    index and the fraction in 0 .. 2^17 - 1 of every output voxel, per axis"""
    a = np.asarray(a, dtype=np.int64)
    P = [int(v) for v in patch]
    grid = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in P], indexing='ij')
    op = [P[c] - 1 - grid[c] if flips[c] else grid[c] for c in range(3)]           # the output index after the flip rule
    t = [2 * op[c] - (P[c] - 1) for c in range(3)]
    lo, hi, near, frac = [], [], [], []
    for r in range(3):
        s = ((2 * int(o[r]) + P[r] - 1) << 16) + a[r, 0] * t[0] + a[r, 1] * t[1] + a[r, 2] * t[2]
        i0 = s >> 17                                                               # (numpy's >> on int64 floors, as Python's)
        top = int(shape[r]) - 1
        lo.append(np.clip(i0, 0, top)); hi.append(np.clip(i0 + 1, 0, top)); near.append(np.clip((s + (1 << 16)) >> 17, 0, top))
        frac.append(s & (ONE - 1))
    return np.stack(lo), np.stack(hi), np.stack(near), np.stack(frac)


def warp_targets(seg, a, o, patch, flips=(False, False, False), K=0, relabel=True):
    """the raw label at the nearest index, then label 4 -> 3 with `relabel` and the K region channels; zeros without a label volume"""
    if seg is None:
        t = np.zeros(patch, np.float32)
    else:
        seg = np.asarray(seg, np.float32)
        _, _, near, _ = coords(a, o, patch, seg.shape, flips)
        t = seg[near[0], near[1], near[2]].copy()
    if relabel:
        t[t == 4] = 3
    if K == 0:
        return t
    return np.stack([(t == np.float32(c + 1)).astype(np.float32) for c in range(K)])


def _lerp(x, y, w):
    d = y - x                 # each statement rounds once in the arrays' dtype
    p = w * d
    return x + p


def warp_inputs(vols, a, o, patch, flips=(False, False, False), aug=False, scale=1.0, shift=0.0, dtype=np.float64):
    """vols: the M stored volumes of the item, None = absent (reads 0 everywhere).  -> (inputs (M, PH, PW, PD) of `dtype`, mask (M,), marker
    (M, PH, PW, PD) bool: where the rule puts exactly -10).  m0 as patch3d_check.gather_inputs; scale and shift are fp32-rounded parameters."""
    shape = next(v.shape for v in vols if v is not None) if any(v is not None for v in vols) else tuple(patch)
    lo, hi, near, frac = coords(a, o, patch, shape, flips)
    w = [(frac[r].astype(dtype) / dtype(ONE)) for r in range(3)]                   # exact in fp32: 17-bit integers over a power of two
    mask = np.array([0.0 if v is None else 1.0 for v in vols], dtype=np.float32)
    m0 = None
    if aug:
        mins = [np.float32(v.min()) for v in vols if v is not None] + ([np.float32(0)] if any(v is None for v in vols) else [])
        m0 = np.float32(min(mins))
    out, marker = [], []
    for v in vols:
        v = np.zeros(shape, np.float32) if v is None else np.asarray(v, np.float32)
        vn = v[near[0], near[1], near[2]]
        c = {}
        for bh, ih in ((0, lo[0]), (1, hi[0])):
            for bw, iw in ((0, lo[1]), (1, hi[1])):
                for bd, id_ in ((0, lo[2]), (1, hi[2])):
                    x = v[ih, iw, id_]
                    if aug:
                        x = np.where(x == m0, vn, x)                               # the background marker never bleeds into tissue
                    c[bh, bw, bd] = x.astype(dtype)
        xd = {(bh, bw): _lerp(c[bh, bw, 0], c[bh, bw, 1], w[2]) for bh in (0, 1) for bw in (0, 1)}          # along d,
        xw = {bh: _lerp(xd[bh, 0], xd[bh, 1], w[1]) for bh in (0, 1)}                                      # then w,
        x = _lerp(xw[0], xw[1], w[0])                                                                      # then h
        mk = np.zeros(x.shape, bool)
        if aug:
            xs = x * dtype(np.float32(scale))
            x = xs + dtype(np.float32(shift))
            mk = vn == m0
            x[mk] = dtype(-10)
        out.append(x); marker.append(mk)
    return np.stack(out), mask, np.stack(marker)


def amax(vols):
    """the largest absolute stored value among the volumes of a row (the scale of the interpolation bound)"""
    return max([float(np.abs(np.asarray(v, np.float64)).max()) for v in vols if v is not None] + [0.0])


def bound(vols, scale, shift, units=18):
    """units * 2^-24 * (amax |scale| + |shift|), per element, u = 2^-24 the relative error of one fp32 rounding.  One interpolation
    a + t (b - a) with |a|, |b| <= amax and 0 <= t < 1 rounds three times: the difference (<= 2 amax: error <= 2 u amax, then scaled by t),
    the product (<= 2 u amax) and the sum (a convex combination, <= amax: error <= u amax) -- at most 5 u amax.  The seven interpolations
    sit three deep (d, then w, then h), and a level passes the errors of the one below through a convex combination, so they add per level
    and do not grow: 15 u amax.  x * scale rounds once (u amax |scale|) and + shift once (u (amax |scale| + |shift|)): 17 units to first
    order, 18 with the second-order terms."""
    return units * 2.0 ** -24 * (amax(vols) * abs(float(np.float32(scale))) + abs(float(np.float32(shift))))


def draw_item(rng, n_present, dropoff, aug, patch_fg, patch_flips, patch_warp=0.0, patch_rot=(30, 30, 30), patch_zoom=(0.7, 1.4)):
    """patch3d_check.draw_item with the warp draws: directly after the flips and before scale and shift, only with aug and patch_warp > 0, one
    rand(5) whatever its first value says.  -> (drop, fg, u, flips, scale, shift, warp): warp = None (no draw) or (warped, angles, zoom)"""
    drop = -1
    if dropoff and n_present > 1:
        if rng.rand() > 0.8:
            drop = int(rng.choice(np.arange(n_present), 1)[0])
    fg = bool(rng.rand() < patch_fg) if patch_fg > 0 else False
    u = rng.randint(0, 2 ** 32, size=5, dtype=np.uint32)
    flips, scale, shift, warp = [False, False, False], 1.0, 0.0, None
    if aug:
        for i, axis in enumerate('hwd'):
            if axis in patch_flips:
                flips[i] = bool(rng.rand() > 0.5)
        if patch_warp > 0:
            r = rng.rand(5)
            warp = (bool(r[0] < patch_warp), tuple((2 * r[1 + ax] - 1) * patch_rot[ax] for ax in range(3)), patch_zoom[0] + r[4] * (patch_zoom[1] - patch_zoom[0]))
        scale = 1 + 0.2 * (rng.rand() - 0.5)
        shift = 0.2 * (rng.rand() - 0.5)
    return drop, fg, u, tuple(flips), scale, shift, warp


def loader_batches(data, subjects, contrasts, batch_size, patch, rng, aug=True, dropoff=False, patch_fg=0.0, patch_flips='h', K=0, classes=(1, 2, 4),
                   patch_warp=0.0, patch_rot=(30, 30, 30), patch_zoom=(0.7, 1.4)):
    """the batches of an unshuffled warping patch-mode VolumeLoader3D, as patch3d_check.loader_batches: a list of dicts with 'inputs' (float64
    evaluation), 'inputs32' (float32 evaluation), 'marker', 'targets', 'mask', 'origins', and per item 'warped' and 'bound' (the per-element
    bound of the row; 0 for a row without a warp: exact)"""
    shape = next(iter(data.values())).shape
    out = []
    for k in range(0, len(subjects), batch_size):
        items = []
        for sid in subjects[k:k + batch_size]:
            vols = [data.get(sid + '/' + c) for c in contrasts]
            seg = data.get(sid + '/seg')
            present = [m for m, v in enumerate(vols) if v is not None]
            drop, fg, u, flips, scale, shift, warp = draw_item(rng, len(present), dropoff, aug, patch_fg, patch_flips, patch_warp, patch_rot, patch_zoom)
            if drop >= 0:
                vols[present[drop]] = None
            o = chk.origin(shape, patch, u, fg=fg, seg=seg, classes=classes if patch_fg > 0 else ())
            if warp is not None and warp[0]:
                a = matrix(warp[1], warp[2])
                x, mask, marker = warp_inputs(vols, a, o, patch, flips, aug, scale, shift, np.float64)
                x32 = warp_inputs(vols, a, o, patch, flips, aug, scale, shift, np.float32)[0]
                t = warp_targets(seg, a, o, patch, flips, K)
                bnd = bound(vols, scale, shift)
            else:
                x32, mask = chk.gather_inputs(vols, o, patch, flips, aug, scale, shift)
                x, marker, bnd = x32.astype(np.float64), x32 == np.float32(-10), 0.0
                if not aug:
                    marker = np.zeros_like(marker)
                t = chk.gather_targets(seg, o, patch, flips, K)
            items.append(dict(inputs=x, inputs32=x32, marker=marker, targets=t, mask=mask, origins=np.array(o[:4], np.int32),
                              warped=bool(warp is not None and warp[0]), bound=bnd))
        out.append({key: np.stack([i[key] for i in items]) for key in ('inputs', 'inputs32', 'marker', 'targets', 'mask', 'origins')}
                   | {'warped': [i['warped'] for i in items], 'bound': [i['bound'] for i in items]})
    return out
