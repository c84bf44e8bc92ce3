"""Plain-numpy oracle of the intensity augmentation of the 3-D training patches (csrc/mrdis_tone.hip, tone3d.py, data3d.py's `patch_blur` ..
`patch_noise_std` keys): the three rules of include/mrdis.h restated independently, taking a dtype -- float64, or float32 with every statement
rounded once and the fused multiply-add emulated exactly (`fma`: one rounding of the exact product and sum) -- Philox4x32-10, the table
packing, the loader's draws (extending tests/warp_check.py) and the bounds the tests hold the kernels to.  Nothing here imports the package.
Items are (M, PH, PW, PD) arrays, one contrast after the other; a voxel is background iff it equals -10.0 exactly.

Used by tests/test_tone_cpu.py and tests/test_gpu_tone.py."""
import numpy as np

BLUR, CONTRAST, GAMMA, INVERT, NOISE = 1, 2, 4, 8, 16
R = 4
BG = np.float32(-10.0)
Z_SCALE = np.array([0x3addb446], dtype=np.uint32).view(np.float32)[0]          # the fp32 nearest to 349520^-1/2
U = 2.0 ** -24                                                                   # the relative error of one fp32 rounding


def TONE_EXTRA(M):
    return 1 + 5 * M


def taps(sigma):
    """(5,) float32: exp(-t^2 / (2 sigma^2)) over the sum of all nine, float64, rounded once"""
    t = np.arange(R + 1, dtype=np.float64)
    g = np.exp(-(t * t) / (2.0 * np.float64(sigma) ** 2))
    return (g / (g[0] + 2.0 * (g[1] + g[2] + g[3] + g[4]))).astype(np.float32)


def fma(a, b, c, dtype):
    """a b + c with ONE rounding in `dtype`.  float32: the product of two fp32 is exact in float64; the float64 sum is rounded to odd (TwoSum
    gives its error exactly), and 53 bits rounded to odd, then to the nearest 24, is the correctly rounded fp32 of the exact value."""
    if dtype is np.float64:
        return np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                                # exact: s + e == p + c
    s, e = np.broadcast_arrays(s, e)
    s = s.copy()
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s[fix] = np.nextafter(s[fix], np.where(e[fix] > 0, np.inf, -np.inf))
    return s.astype(np.float32)


# ---------------------------------------------------------------- blur
def blur(x, flags, g, dtype=np.float64, radius=R, border=True, marker_in_sum=False, order=(2, 1, 0), extent_of=None):
    """x (M, PH, PW, PD) float32, flags (M,) integers, g (M, 5) float32 taps -> y (M, PH, PW, PD) of `dtype`.  A contrast without BLUR: x.
    The planted faults of the tests: `radius` 3, `border` False (a tap outside the patch still adds its weight to D: no renormalisation at
    the patch border), `marker_in_sum` (the -10 voxels enter N and D), `order` (the axes of the passes; the rule is d, w, h = 2, 1, 0 -- the
    passes are linear with the same taps, so another order is the same sum in exact arithmetic and only moves roundings) and `extent_of`
    ({axis: axis}: the pass along an axis tests "inside the patch" against another axis's extent -- the d and h passes swapped in a kernel
    whose passes are (stride, extent) pairs: each steps along its own axis with the other's extent; a tap at or beyond the smaller extent
    is dropped)."""
    x = np.asarray(x, np.float32)
    out = x.astype(dtype).copy()
    for m in range(x.shape[0]):
        if not int(flags[m]) & BLUR:
            continue
        tissue = x[m] != BG
        keep = np.ones_like(tissue) if marker_in_sum else tissue
        N = np.where(keep, x[m], np.float32(0)).astype(dtype)
        D = keep.astype(dtype)
        for axis in order:
            n = x.shape[1 + axis]
            accN, accD = np.zeros_like(N), np.zeros_like(D)
            for t in range(-radius, radius + 1):                                 # t increasing: the order of the chain
                gt = dtype(g[m][abs(t)])
                lo, hi = max(0, -t), min(n, n - t)                               # the p with p + t inside
                if extent_of is not None:                                        # the fault: inside means inside the other axis's extent
                    lim = min(n, x.shape[1 + extent_of.get(axis, axis)])
                    hi = max(lo, min(hi, lim - t))
                if hi > lo:
                    dst = [slice(None)] * 3
                    src = [slice(None)] * 3
                    dst[axis], src[axis] = slice(lo, hi), slice(lo + t, hi + t)
                    dst, src = tuple(dst), tuple(src)
                    accN[dst] = fma(gt, N[src], accN[dst], dtype)
                    accD[dst] = fma(gt, D[src], accD[dst], dtype)
                if not border:                                                   # the fault: the taps outside count as tissue of value 0
                    outside = np.ones(n, bool)
                    outside[lo:hi] = False
                    sl = [None] * 3
                    sl[axis] = slice(None)
                    accD = np.where(outside[tuple(sl)], fma(gt, dtype(1), accD, dtype), accD)
            N, D = accN, accD
        with np.errstate(invalid='ignore', divide='ignore'):
            q = (N / D).astype(dtype)
        out[m] = np.where(tissue, q, dtype(BG))
    return out


def blur_bound(x, units=56):
    """per contrast, units * 2^-24 * amax, amax the largest absolute tissue value of the contrast.  A pass is a chain of at most nine fmaf with
    non-negative taps; every fmaf rounds once, by at most u |partial sum|, and the partial sums of N are at most amax times those of D, which
    grow to the pass's own D'[p]: a pass adds at most 9 u amax D'[p] to N and 9 u D'[p] to D.  The next pass carries the errors of its inputs
    through the same non-negative combination, so they stay proportional to the new D': after three passes |dN| <= 27 u amax D and
    |dD| <= 27 u D (to first order; a tap outside the patch or on background adds an exact zero).  The quotient: |dy| <= (|dN| + |y| |dD|) / D
    + u |y| <= 27 u amax + 27 u amax + u amax = 55 u amax; 56 with the second-order terms."""
    x = np.asarray(x, np.float32)
    out = []
    for m in range(x.shape[0]):
        t = x[m][x[m] != BG]
        out.append(units * U * (float(np.abs(t.astype(np.float64)).max()) if t.size else 0.0))
    return np.array(out)


# ---------------------------------------------------------------- statistics
def stats(y):
    """y (M, ...) float32 -> (lo, hi, mean) float32 (M,) and n int (M,): over the tissue voxels; zeros where there is none.  The mean is the
    float64 sum over the float64 count, rounded once (any order of a float64 sum of fp32 values stays within 2^-53 n of it: far below the
    fp32 rounding, but it can move a mean that sits on a rounding boundary: the tests allow one fp32 ulp)."""
    y = np.asarray(y, np.float32)
    M = y.shape[0]
    lo, hi, mean, n = np.zeros(M, np.float32), np.zeros(M, np.float32), np.zeros(M, np.float32), np.zeros(M, np.int64)
    for m in range(M):
        t = y[m][y[m] != BG]
        n[m] = t.size
        if t.size:
            lo[m], hi[m] = t.min(), t.max()
            mean[m] = np.float32(t.astype(np.float64).sum() / np.float64(t.size))
    return lo, hi, mean, n


# ---------------------------------------------------------------- noise
def philox(counter, key):
    """Philox4x32-10: counter four uint32 (arrays broadcast), key two uint32 -> four uint32 arrays"""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xffffffff) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    mask, sh = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                                            # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [v.astype(np.uint32) for v in c]


def noise_z(n, m, seed):
    """(n,) float32: z of the voxels p = 0 .. n - 1 of contrast m: (float)(2 S - 4080) * C, S the sum of the 16 bytes of
    philox((p, m, 0, 0), seed)"""
    words = philox((np.arange(n, dtype=np.uint64), m, 0, 0), seed)
    S = np.zeros(n, dtype=np.int64)
    for w in words:
        w = w.astype(np.int64)
        S += (w & 255) + ((w >> 8) & 255) + ((w >> 16) & 255) + ((w >> 24) & 255)
    return ((2 * S - 4080).astype(np.float32) * Z_SCALE).astype(np.float32)


# ---------------------------------------------------------------- tone
def tone(y, st, flags, f, gamma, std, seed, dtype=np.float64):
    """y (M, PH, PW, PD) float32, st = (lo, hi, mean, n) of `stats` -> the toned item in `dtype`: contrast, gamma, noise on the tissue voxels of
    every contrast, each only where its flag is set.  The parameters are fp32 values; z is the fp32 value of `noise_z` in both dtypes."""
    y = np.asarray(y, np.float32)
    out = y.astype(dtype).copy()
    lo_, hi_, mean_, _ = st
    shape = y.shape[1:]
    for m in range(y.shape[0]):
        fl = int(flags[m])
        if not fl & (CONTRAST | GAMMA | NOISE):
            continue
        tissue = y[m] != BG
        v = y[m].astype(dtype)
        lo, hi, mean = dtype(np.float32(lo_[m])), dtype(np.float32(hi_[m])), dtype(np.float32(mean_[m]))
        if fl & CONTRAST:
            d = (v - mean).astype(dtype)
            v = np.minimum(np.maximum(fma(d, dtype(np.float32(f[m])), mean, dtype), lo), hi).astype(dtype)
        if fl & GAMMA and hi > lo:
            rg = dtype(hi - lo)
            t = np.minimum(np.maximum(((v - lo).astype(dtype) / rg).astype(dtype), dtype(0)), dtype(1))
            if fl & INVERT:
                t = (dtype(1) - t).astype(dtype)
            t = np.power(t, dtype(np.float32(gamma[m]))).astype(dtype)
            if fl & INVERT:
                t = (dtype(1) - t).astype(dtype)
            v = fma(t, rg, lo, dtype).astype(dtype)
        if fl & NOISE:
            z = noise_z(int(np.prod(shape)), m, seed).reshape(shape)
            v = fma(dtype(np.float32(std[m])), z.astype(dtype), v, dtype).astype(dtype)
        out[m] = np.where(tissue, v, dtype(BG))
    return out


def contrast_bound(lo, hi, f, units=None):
    """units * 2^-24 * A, A = max(|lo|, |hi|) (every tissue voxel and the mean lie in [lo, hi]).  v - mean rounds once: at most 2 u A, and the
    factor carries it as 2 |f| u A; the fmaf rounds once, a result of at most |mean| + 2 |f| A: (1 + 2 |f|) u A; the clamp onto [lo, hi] moves
    no value further from the float64 one.  4 |f| + 1 units, one more for the second-order terms."""
    units = 4.0 * abs(float(f)) + 2.0 if units is None else units
    return units * U * max(abs(float(lo)), abs(float(hi)))


def gamma_unit(lo, hi):
    """2^-24 max(|lo|, |hi|): the unit of the gamma step's kappa (4 times the worst ratio of the plain fp32 numpy evaluation of the same rows
    -- `tone(dtype=np.float32)`, numpy.power in fp32 -- to float64: powf is a library function, tests/aux_check.py's practice)"""
    return U * max(abs(float(lo)), abs(float(hi)))


# ---------------------------------------------------------------- table and draws
def pack(seed, flags, sigma, f, gamma, std):
    """the 1 + 5 M table words of an item, by Python integers: word 0 = seed_lo | seed_hi << 32, then per contrast the ten halves flags, g0 ..
    g4, f, gamma, std, 0, the low half first; the taps only where BLUR is set"""
    bits = lambda v: int(np.array([v], dtype=np.float64).astype(np.float32).view(np.uint32)[0])
    halves = [int(seed[0]) & 0xffffffff, int(seed[1]) & 0xffffffff]
    for m, fl in enumerate(flags):
        g = [int(b) for b in taps(sigma[m]).view(np.uint32)] if int(fl) & BLUR else [0] * 5
        halves += [int(fl)] + g + [bits(f[m]), bits(gamma[m]), bits(std[m]), 0]
    words = [halves[i] | (halves[i + 1] << 32) for i in range(0, len(halves), 2)]
    return np.array([w - (1 << 64) if w >= 1 << 63 else w for w in words], dtype=np.int64)


def unpack(words, M):
    """-> (seed (2,), flags (M,), taps (M, 5) float32, f, gamma, std (M,) float32) of a packed block"""
    w = np.asarray(words, dtype=np.int64).view(np.uint64)
    halves = np.stack([w & np.uint64(0xffffffff), w >> np.uint64(32)], axis=1).reshape(-1).astype(np.uint32)
    per = halves[2:2 + 10 * M].reshape(M, 10)
    as_f = lambda a: np.ascontiguousarray(a).view(np.float32)
    return halves[:2].copy(), per[:, 0].astype(np.int64), as_f(per[:, 1:6]), as_f(per[:, 6]), as_f(per[:, 7]), as_f(per[:, 8])


DEFAULTS = dict(patch_blur=0.0, patch_blur_sigma=(0.5, 1.0), patch_contrast=0.0, patch_contrast_range=(0.75, 1.25), patch_gamma=0.0,
                patch_gamma_range=(0.7, 1.5), patch_gamma_invert=0.25, patch_noise=0.0, patch_noise_std=(0.0, 0.3))


def intensifies(aug, keys):
    return bool(aug) and any(keys[k] > 0 for k in ('patch_blur', 'patch_contrast', 'patch_gamma', 'patch_noise'))


def draw_tone(rng, present, keys):
    """step 4c: rand(4 + 6 M), then two uint32 -> (seed, flags, sigma, f, gamma, std), the values fp32.  present: per contrast, whether the item
    has it after the drop-off"""
    M = len(present)
    r = rng.rand(4 + 6 * M)
    seed = rng.randint(0, 2 ** 32, size=2, dtype=np.uint32)
    flags, vals = [], [[], [], [], []]
    for m in range(M):
        q = r[4 + 6 * m:10 + 6 * m]
        fl = 0
        if present[m]:
            if r[0] < keys['patch_blur'] and q[0] < 0.5:
                fl |= BLUR
            if r[1] < keys['patch_contrast']:
                fl |= CONTRAST
            if r[2] < keys['patch_gamma']:
                fl |= GAMMA | (INVERT if q[4] < keys['patch_gamma_invert'] else 0)
            if r[3] < keys['patch_noise']:
                fl |= NOISE
        flags.append(fl)
        for k, (key, col) in enumerate((('patch_blur_sigma', 1), ('patch_contrast_range', 2), ('patch_gamma_range', 3), ('patch_noise_std', 5))):
            lo, hi = keys[key]
            vals[k].append(np.float32(lo + q[col] * (hi - lo)))
    return (seed, tuple(flags)) + tuple(np.array(v, np.float32) for v in vals)


def draw_item(rng, present, dropoff, aug, patch_fg, patch_flips, patch_warp=0.0, patch_rot=(30, 30, 30), patch_zoom=(0.7, 1.4), **keys):
    """warp_check.draw_item (restated) with the intensity draws: after the warp draw (or the flips), before scale and shift, only with aug and a share
    above 0.  present: per contrast, whether the subject has it.  -> (drop, fg, u, flips, scale, shift, warp, tone): tone = None (no draw) or
    `draw_tone`'s tuple"""
    keys = dict(DEFAULTS, **keys)
    have = [m for m, p in enumerate(present) if p]
    drop = -1
    if dropoff and len(have) > 1:
        if rng.rand() > 0.8:
            drop = int(rng.choice(np.arange(len(have)), 1)[0])
    live = [bool(p) and (drop < 0 or m != have[drop]) for m, p in enumerate(present)]
    fg = bool(rng.rand() < patch_fg) if patch_fg > 0 else False
    u = rng.randint(0, 2 ** 32, size=5, dtype=np.uint32)
    flips, scale, shift, warp, tn = [False, False, False], 1.0, 0.0, None, None
    if aug:
        for i, axis in enumerate('hwd'):
            if axis in patch_flips:
                flips[i] = bool(rng.rand() > 0.5)
        if patch_warp > 0:
            r = rng.rand(5)
            warp = (bool(r[0] < patch_warp), tuple((2 * r[1 + ax] - 1) * patch_rot[ax] for ax in range(3)), patch_zoom[0] + r[4] * (patch_zoom[1] - patch_zoom[0]))
        if intensifies(aug, keys):
            tn = draw_tone(rng, live, keys)
        scale = 1 + 0.2 * (rng.rand() - 0.5)
        shift = 0.2 * (rng.rand() - 0.5)
    return drop, fg, u, tuple(flips), scale, shift, warp, tn



def loader_batches(data, subjects, contrasts, batch_size, patch, rng, dropoff=False, patch_fg=0.0, patch_flips='h', K=0, classes=(1, 2, 4), **keys):
    """the batches of an unshuffled, augmenting, intensifying (and not warping) patch-mode VolumeLoader3D, as patch3d_check.loader_batches: a list
    of dicts with 'gathered' (B, M, PH, PW, PD) float32 -- the exact result of the gather, what the three calls start from -- 'tone' (per item,
    `draw_tone`'s tuple), 'targets', 'mask', 'origins'"""
    import patch3d_check as chk
    shape = next(iter(data.values())).shape
    out = []
    for k in range(0, len(subjects), batch_size):
        items = []
        for sid in subjects[k:k + batch_size]:
            vols = [data.get(sid + '/' + c) for c in contrasts]
            seg = data.get(sid + '/seg')
            present = [v is not None for v in vols]
            drop, fg, u, flips, scale, shift, _, tn = draw_item(rng, present, dropoff, True, patch_fg, patch_flips, **keys)
            if drop >= 0:
                vols[[m for m, p in enumerate(present) if p][drop]] = None
            o = chk.origin(shape, patch, u, fg=fg, seg=seg, classes=classes if patch_fg > 0 else ())
            x, mask = chk.gather_inputs(vols, o, patch, flips, True, scale, shift)
            items.append(dict(gathered=x, tone=tn, targets=chk.gather_targets(seg, o, patch, flips, K), mask=mask, origins=np.array(o[:4], np.int32)))
        out.append({key: np.stack([i[key] for i in items]) for key in ('gathered', 'targets', 'mask', 'origins')} | {'tone': [i['tone'] for i in items]})
    return out
