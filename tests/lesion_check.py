"""numpy oracles of the lesion-wise scores (tests/test_lesion_cpu.py checks them against scipy.ndimage, tests/test_gpu_lesion.py checks the
kernels of csrc/mrdis_lesion.hip and mrdis.lesion_scores against them).  numpy only, independent of the package.

The oracle follows the two-step procedure literally: label T with 26-connectivity, dilate every component by iterated 18-neighbourhood
shifts, merge the components whose dilations are 26-connected, then loop over the lesions, select the predicted components by overlap with
the dilated lesion, and score each pair by Dice and by an HD95 from brute-force distances under the package's integer percentile rule."""
import itertools

import numpy as np

OFFSETS = {6: [o for o in itertools.product((-1, 0, 1), repeat=3) if sum(map(abs, o)) == 1],
           18: [o for o in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(map(abs, o)) <= 2],
           26: [o for o in itertools.product((-1, 0, 1), repeat=3) if any(o)]}
BRATS_REGIONS = (('wt', (1, 2, 4)), ('tc', (1, 4)), ('et', (4,)))


def shift(a, off, fill=0):
    """b[x] = a[x - off], `fill` where x - off lies outside the volume: nothing wraps"""
    out = np.full_like(a, fill)
    src, dst = [], []
    for n, o in zip(a.shape, off):
        src.append(slice(max(0, -o), n - max(0, o)))
        dst.append(slice(max(0, o), n - max(0, -o)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def dilate(mask, iterations=1, connectivity=18):
    """binary dilation of one (H, W, D) volume by the 6 / 18 / 26 neighbourhood, iterated; a uint8 volume dilates bit by bit"""
    out = np.array(mask, dtype=np.uint8 if mask.dtype != bool else bool)
    for _ in range(iterations):
        acc = out.copy()
        for off in OFFSETS[connectivity]:
            acc |= shift(out, off)
        out = acc
    return out


def components(mask, connectivity=26):
    """comp (H, W, D) int64: -1 on background, else the smallest flat index of the voxel's component (min-propagation to a fixed point)"""
    mask = np.asarray(mask).astype(bool)
    big = mask.size
    lab = np.where(mask, np.arange(mask.size, dtype=np.int64).reshape(mask.shape), big)
    fg = np.flatnonzero(mask.reshape(-1))
    while True:
        new = lab.copy()
        for off in OFFSETS[connectivity]:
            new = np.minimum(new, shift(lab, off, big))
        new = np.where(mask, new, big)
        flat = new.reshape(-1)                                       # a label is the index of a voxel of the same component: follow it
        for _ in range(4):
            flat[fg] = flat[flat[fg]]
        if (new == lab).all():
            break
        lab = new
    return np.where(mask, lab, -1)


def surface(mask):
    """voxels of the mask with a face neighbour outside it; the volume border counts as outside"""
    mask = np.asarray(mask).astype(bool)
    inner = mask.copy()
    for off in OFFSETS[6]:
        inner &= shift(mask, off, False)
    return mask & ~inner


def directed_k(a_surf, b_surf):
    """the squared nearest-rank 95 % distance measured at the voxels of a_surf to b_surf: the smallest k with 20 * #(d2 <= k) >= 19 * n"""
    a = np.argwhere(a_surf).astype(np.int64)
    b = np.argwhere(b_surf).astype(np.int64)
    if len(a) == 0 or len(b) == 0:
        return 0
    d2 = np.empty(len(a), dtype=np.int64)
    for i0 in range(0, len(a), 256):
        diff = a[i0:i0 + 256, None, :] - b[None, :, :]
        d2[i0:i0 + 256] = (diff * diff).sum(-1).min(1)
    d2.sort()
    n = len(d2)
    for i, k in enumerate(d2):                                       # cum[k] = number of values <= k
        if i + 1 < n and d2[i + 1] == k:
            continue
        if 20 * (i + 1) >= 19 * n:
            return int(k)
    raise AssertionError('unreachable')


def pair_scores(s, t, spacing=1.0):
    """(dice, hd95, [|t|, |s|, |s and t|, k at t's surface, k at s's surface]) of two masks under the package's region rules"""
    s, t = np.asarray(s).astype(bool), np.asarray(t).astype(bool)
    ns, nt, ni = int(s.sum()), int(t.sum()), int((s & t).sum())
    pen = np.float64(spacing) * np.sqrt(np.float64(sum(n * n for n in s.shape)))
    if ns == 0 and nt == 0:
        return 1.0, 0.0, [0, 0, 0, 0, 0]
    dice = 2.0 * np.float64(ni) / np.float64(ns + nt)
    if ns == 0 or nt == 0:
        return float(dice), float(pen), [nt, ns, ni, 0, 0]
    ss, ts = surface(s), surface(t)
    kt, ks = directed_k(ts, ss), directed_k(ss, ts)
    return float(dice), float(np.float64(spacing) * np.sqrt(np.float64(max(kt, ks)))), [nt, ns, ni, kt, ks]


def region_mask(vol, labels):
    """membership of a region: integral values among `labels`; a non-integral value or one outside 0 .. 7 belongs to no region"""
    v = np.asarray(vol)
    out = np.zeros(v.shape, dtype=bool)
    for l in labels:
        out |= v == l
    return out


def lesions_two_step(t, dilation):
    """[(id, dilated lesion mask, T_L mask)] in id order: label T, dilate each component, merge components whose dilations are 26-connected
    (their union has them in one 26-component), id = the smallest flat index of the merged dilated set"""
    comp = components(t, 26)
    ids = [int(i) for i in np.unique(comp) if i >= 0]
    dil = {i: dilate(comp == i, dilation, 18).astype(bool) for i in ids}
    near = {i: dilate(dil[i], 1, 26).astype(bool) for i in ids}      # 26-connected: a voxel of one within the 3 x 3 x 3 cube of the other
    group = {i: i for i in ids}                                      # every component -> the smallest component id of its merged group
    for a, b in itertools.combinations(ids, 2):
        if group[a] != group[b] and (near[a] & dil[b]).any():
            lo, hi = sorted((group[a], group[b]))
            group = {i: (lo if g == hi else g) for i, g in group.items()}
    groups = [[i for i in ids if group[i] == g] for g in sorted(set(group.values()))]
    out = []
    for g in groups:
        m = np.logical_or.reduce([dil[i] for i in g])
        tl = np.logical_or.reduce([comp == i for i in g])
        out.append((int(np.flatnonzero(m.reshape(-1))[0]), m, tl))
    return sorted(out, key=lambda x: x[0])


def lesion_scores(labels, targets, regions=BRATS_REGIONS, dilation=3, min_voxels=50, spacing=1.0, has_target=None):
    """the dict of mrdis.lesion_scores as numpy arrays, for labels (B, H, W, D) integers and targets (B, H, W, D) numbers"""
    labels, targets = np.asarray(labels), np.asarray(targets)
    B, R = labels.shape[0], len(regions)
    shape = labels.shape[1:]
    pen = np.float64(spacing) * np.sqrt(np.float64(sum(n * n for n in shape)))
    has_target = np.ones(B, dtype=bool) if has_target is None else np.asarray(has_target).astype(bool)
    dice_out, hd_out = np.zeros((B, R)), np.zeros((B, R))
    counts = np.zeros((B, R, 5), dtype=np.int64)
    rows, dice_each, hd_each = [], [], []
    for b in range(B):
        for r, (_, labs) in enumerate(regions):
            p = region_mask(labels[b], labs)
            t = region_mask(targets[b], labs) if has_target[b] else np.zeros(shape, dtype=bool)
            pc = components(p, 26)
            pids = [int(i) for i in np.unique(pc) if i >= 0]
            matched = set()
            sd, sh, kept_n, missed = np.float64(0), np.float64(0), 0, 0
            les = lesions_two_step(t, dilation)
            for lid, m, tl in les:
                hit = [i for i in pids if (m & (pc == i)).any()]
                matched.update(hit)
                s = np.isin(pc, hit) if hit else np.zeros(shape, dtype=bool)
                d, h, ints = pair_scores(s, tl, spacing)
                kept = int(ints[0] >= min_voxels)
                rows.append([b, r, lid] + ints + [kept])
                dice_each.append(d)
                hd_each.append(h)
                if kept:
                    sd += d
                    sh += h
                    kept_n += 1
                    missed += int(ints[1] == 0)
            fp = len(pids) - len(matched)
            counts[b, r] = [len(les), kept_n, missed, len(pids), fp]
            den = kept_n + fp
            dice_out[b, r] = sd / den if den else 1.0
            hd_out[b, r] = (sh + np.float64(fp) * pen) / den if den else 0.0
        if not has_target[b]:
            dice_out[b], hd_out[b] = np.nan, np.nan
    return {'lesion_dice': dice_out, 'lesion_hd95': hd_out, 'counts': counts, 'lesions': np.asarray(rows, dtype=np.int64).reshape(-1, 9),
            'lesion_dice_each': np.asarray(dice_each, dtype=np.float64), 'lesion_hd95_each': np.asarray(hd_each, dtype=np.float64)}
