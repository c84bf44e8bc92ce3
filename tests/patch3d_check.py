"""Plain-numpy oracle of patch sampling for the 3-D nets (csrc/mrdis_patch.hip, patch3d.py, data3d.py's patch mode): the rules restated
independently, in Python integers / uint64 for `pick` and float32 with two roundings for the augmentation.  Every comparison against it is
exact.  Used by tests/test_patch3d_cpu.py (hand-worked cases, no GPU) and tests/test_gpu_patch3d.py."""
import numpy as np

BLOCK = 1024


def pick(u, n):
    """(u n) >> 32 in uint64: a uint32 draw onto 0 .. n - 1"""
    assert 0 <= int(u) < 2 ** 32 and 1 <= int(n) < 2 ** 32
    return int((np.uint64(u) * np.uint64(n)) >> np.uint64(32))


def u_reaching(r, n):
    """the smallest uint32 u with pick(u, n) == r: ceil(r 2^32 / n)"""
    return -((-int(r) << 32) // int(n))


def block_counts(seg, classes):
    """(nblk, K) int32: voxels of each class per block of 1024 consecutive flat indices"""
    flat = np.asarray(seg, dtype=np.float32).reshape(-1)
    nblk = (flat.size + BLOCK - 1) // BLOCK
    out = np.zeros((nblk, len(classes)), dtype=np.int32)
    for j in range(nblk):
        blk = flat[j * BLOCK:(j + 1) * BLOCK]
        for c, v in enumerate(classes):
            out[j, c] = int((blk == np.float32(v)).sum())
    return out


def prefix_table(seg, classes):
    """(nblk + 1, K) int32: exclusive prefix of `block_counts`, the last row the totals"""
    counts = block_counts(seg, classes)
    return np.concatenate([np.zeros((1, len(classes)), np.int32), np.cumsum(counts, axis=0, dtype=np.int64).astype(np.int32)])


def clamp(v, lo, hi):
    return max(lo, min(hi, v))


def origin(shape, patch, u, fg=False, seg=None, classes=(), has_prefix=True, centre=False):
    """-> (h0, w0, d0, chosen class index or -1, centre voxel (hc, wc, dc) or None).  u = (u_class, u_voxel, u_h, u_w, u_d)."""
    H, W, D = shape
    PH, PW, PD = patch
    assert PH <= H and PW <= W and PD <= D
    if centre:
        return (H - PH) // 2, (W - PW) // 2, (D - PD) // 2, -1, None
    u_class, u_voxel, u_h, u_w, u_d = (int(v) for v in u)
    uniform = (pick(u_h, H - PH + 1), pick(u_w, W - PW + 1), pick(u_d, D - PD + 1), -1, None)
    if not fg or seg is None or not has_prefix or not classes:
        return uniform
    flat = np.asarray(seg, dtype=np.float32).reshape(-1)
    where = [np.flatnonzero(flat == np.float32(v)) for v in classes]          # increasing flat index
    present = [c for c in range(len(classes)) if where[c].size]
    if not present:
        return uniform
    c = present[pick(u_class, len(present))]
    f = int(where[c][pick(u_voxel, where[c].size)])
    hc, wc, dc = f // (W * D), (f // D) % W, f % D
    return clamp(hc - PH // 2, 0, H - PH), clamp(wc - PW // 2, 0, W - PW), clamp(dc - PD // 2, 0, D - PD), c, (hc, wc, dc)


def cut(vol, o, patch, flips):
    """the (PH, PW, PD) patch of `vol` at origin o, mirrored inside the patch on the flipped axes"""
    h0, w0, d0 = o[:3]
    PH, PW, PD = patch
    p = vol[h0:h0 + PH, w0:w0 + PW, d0:d0 + PD]
    fh, fw, fd = flips
    return p[::-1 if fh else 1, ::-1 if fw else 1, ::-1 if fd else 1]


def gather_inputs(vols, o, patch, flips=(False, False, False), aug=False, scale=1.0, shift=0.0):
    """vols: the M stored volumes of the item, None = absent or dropped.  -> (inputs (M, PH, PW, PD) fp32, mask (M,)).  With aug:
    x * scale + shift in fp32 with fp32-rounded parameters and two roundings, -10 where the RAW value equals m0 = the minimum over the
    present contrasts of the WHOLE stored volume's minimum, and 0 if a contrast is absent."""
    raw = np.stack([cut(v, o, patch, flips) if v is not None else np.zeros(patch, np.float32) for v in vols]).astype(np.float32)
    mask = np.array([0.0 if v is None else 1.0 for v in vols], dtype=np.float32)
    if not aug:
        return raw, mask
    mins = [np.float32(v.min()) for v in vols if v is not None] + ([np.float32(0)] if any(v is None for v in vols) else [])
    m0 = np.float32(min(mins))
    xs = (raw * np.float32(scale)).astype(np.float32)                          # first rounding
    x = (xs + np.float32(shift)).astype(np.float32)                           # second rounding
    x[raw == m0] = np.float32(-10)
    return x, mask


def gather_targets(seg, o, patch, flips=(False, False, False), K=0, relabel=True):
    """-> the label patch (PH, PW, PD), label 4 -> 3 with `relabel`, or its K region channels (K, PH, PW, PD), channel c = (label == c + 1);
    zeros without a label volume"""
    t = np.zeros(patch, np.float32) if seg is None else cut(np.asarray(seg, np.float32), o, patch, flips).copy()
    if relabel:
        t[t == 4] = 3
    if K == 0:
        return t
    return np.stack([(t == np.float32(c + 1)).astype(np.float32) for c in range(K)])


def draw_item(rng, n_present, dropoff, aug, patch_fg, patch_flips):
    """the host draws of one patch-mode item, in the documented order, from `rng` (a np.random.RandomState or the np.random module):
    -> (drop index among the PRESENT contrasts or -1, fg, u (5,) uint32, (flip h, w, d), scale, shift)"""
    drop = -1
    if dropoff and n_present > 1:
        if rng.rand() > 0.8:
            drop = int(rng.choice(np.arange(n_present), 1)[0])
    fg = bool(rng.rand() < patch_fg) if patch_fg > 0 else False
    u = rng.randint(0, 2 ** 32, size=5, dtype=np.uint32)
    flips, scale, shift = [False, False, False], 1.0, 0.0
    if aug:
        for i, axis in enumerate('hwd'):
            if axis in patch_flips:
                flips[i] = bool(rng.rand() > 0.5)
        scale = 1 + 0.2 * (rng.rand() - 0.5)
        shift = 0.2 * (rng.rand() - 0.5)
    return drop, fg, u, tuple(flips), scale, shift


def loader_batches(data, subjects, contrasts, batch_size, patch, rng, aug=False, dropoff=False, patch_fg=0.0, patch_flips='h', K=0,
                   classes=(1, 2, 4), centre=False):
    """the batches of an unshuffled patch-mode VolumeLoader3D over `data` ({'subject/contrast' | 'subject/seg': (H, W, D) array}), drawn from
    `rng`: a list of {'inputs' (B, M, PH, PW, PD), 'targets', 'mask' (B, M), 'origins' (B, 4) int32, 'centres'}"""
    shape = next(iter(data.values())).shape
    out = []
    for k in range(0, len(subjects), batch_size):
        items = []
        for sid in subjects[k:k + batch_size]:
            vols = [data.get(sid + '/' + c) for c in contrasts]
            seg = data.get(sid + '/seg')
            present = [m for m, v in enumerate(vols) if v is not None]
            if centre:
                drop = -1
                if dropoff and len(present) > 1 and rng.rand() > 0.8:
                    drop = int(rng.choice(np.arange(len(present)), 1)[0])
                fg, u, flips, scale, shift = False, np.zeros(5, np.uint32), (False, False, False), 1.0, 0.0
            else:
                drop, fg, u, flips, scale, shift = draw_item(rng, len(present), dropoff, aug, patch_fg, patch_flips)
            if drop >= 0:
                vols[present[drop]] = None
            o = origin(shape, patch, u, fg=fg, seg=seg, classes=classes if patch_fg > 0 else (), centre=centre)
            x, mask = gather_inputs(vols, o, patch, flips, aug and not centre, scale, shift)
            items.append((x, gather_targets(seg, o, patch, flips, K), mask, np.array(o[:4], np.int32), o[4]))
        out.append({'inputs': np.stack([i[0] for i in items]), 'targets': np.stack([i[1] for i in items]), 'mask': np.stack([i[2] for i in items]),
                    'origins': np.stack([i[3] for i in items]), 'centres': [i[4] for i in items]})
    return out
