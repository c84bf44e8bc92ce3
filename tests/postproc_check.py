"""CPU oracles of the connected-component tests (tests/test_postproc_cpu.py checks them against a flood fill and scipy;
tests/test_gpu_postproc.py checks the kernels of csrc/mrdis_cc.hip against them).  numpy only, independent of the package."""
import itertools

import numpy as np

BIG = np.iinfo(np.int64).max


def offsets(c):
    """the c-neighbourhood: every offset in {-1, 0, 1}^3 with 1 .. k non-zero entries, k = 1 / 2 / 3 for c = 6 / 18 / 26"""
    k = {6: 1, 18: 2, 26: 3}[c]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(x != 0 for x in o) <= k]


def foreground(labels, fg):
    labels = np.asarray(labels)
    return np.isin(labels, [l for l in fg if 0 < l <= 7])


def np_components(mask, c):
    """mask (H, W, D) bool -> (comp, size) int32 (H, W, D): comp = the smallest flat index of the voxel's component (-1 on background), size =
    the component's voxel count at its root voxel, 0 elsewhere.  The minimum label is propagated over the c-neighbourhood (the volume padded with
    "no label", so nothing wraps) and pointers are jumped (label <- label of the voxel the label names), until nothing changes."""
    mask = np.asarray(mask, dtype=bool)
    H, W, D = mask.shape
    idx = np.arange(H * W * D, dtype=np.int64).reshape(H, W, D)
    lab = np.where(mask, idx, BIG)
    offs = offsets(c)
    while True:
        pad = np.full((H + 2, W + 2, D + 2), BIG, dtype=np.int64)
        pad[1:-1, 1:-1, 1:-1] = lab
        new = lab.copy()
        for dh, dw, dd in offs:
            np.minimum(new, pad[1 + dh:1 + dh + H, 1 + dw:1 + dw + W, 1 + dd:1 + dd + D], out=new)
        new = np.where(mask, new, BIG)
        flat = new.reshape(-1)
        for _ in range(64):                                          # pointer jumping to a fixed point of this round
            nxt = flat.copy()
            fgi = flat != BIG
            nxt[fgi] = flat[flat[fgi]]
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        new = flat.reshape(H, W, D)
        if np.array_equal(new, lab):
            break
        lab = new
    comp = np.where(mask, lab, -1).astype(np.int32)
    size = np.zeros(H * W * D, dtype=np.int32)
    roots, counts = np.unique(comp[mask], return_counts=True)
    size[roots] = counts
    return comp, size.reshape(H, W, D)


def np_components_batch(labels, fg, c):
    labels = np.asarray(labels)
    res = [np_components(foreground(v, fg), c) for v in labels]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def flood_components(mask, c):
    """the same by a hand-written flood fill in scan order (small volumes): the first voxel of a component in scan order is its smallest index"""
    mask = np.asarray(mask, dtype=bool)
    H, W, D = mask.shape
    comp = np.full((H, W, D), -1, dtype=np.int32)
    size = np.zeros((H, W, D), dtype=np.int32)
    offs = offsets(c)
    for h in range(H):
        for w in range(W):
            for d in range(D):
                if not mask[h, w, d] or comp[h, w, d] >= 0:
                    continue
                root = (h * W + w) * D + d
                comp[h, w, d] = root
                stack, n = [(h, w, d)], 0
                while stack:
                    a, b, e = stack.pop()
                    n += 1
                    for dh, dw, dd in offs:
                        x, y, z = a + dh, b + dw, e + dd
                        if 0 <= x < H and 0 <= y < W and 0 <= z < D and mask[x, y, z] and comp[x, y, z] < 0:
                            comp[x, y, z] = root
                            stack.append((x, y, z))
                size[h, w, d] = n
    return comp, size


def np_clean(labels, fg=(1, 2, 4), c=26, min_voxels=0, keep='all', et_label=4, et_min_voxels=0, et_replace=1):
    """the three rules of clean_labels written out per sample.  labels (B, H, W, D) uint8 -> (cleaned (B, H, W, D) uint8, stats (B, 6) int32)"""
    labels = np.asarray(labels, dtype=np.uint8)
    out = labels.copy()
    stats = np.zeros((labels.shape[0], 6), dtype=np.int32)
    for b, vol in enumerate(labels):
        mask = foreground(vol, fg)
        comp, size = np_components(mask, c)
        flat_size = size.reshape(-1)
        roots = [int(r) for r in np.flatnonzero(flat_size > 0)]            # ascending root index
        if keep == 'largest':
            cand = []
            for r in roots:                                                # the first of the largest: a tie goes to the smaller root
                if not cand or flat_size[r] > flat_size[cand[0]]:
                    cand = [r]
        else:
            cand = roots
        kept = [r for r in cand if flat_size[r] >= min_voxels]
        removed = mask & ~np.isin(comp, kept)
        o = out[b]
        o[removed] = 0
        n = int((o == et_label).sum())
        replaced = int(et_min_voxels > 0 and 0 < n < et_min_voxels)
        if replaced:
            o[o == et_label] = et_replace
        stats[b] = [len(roots), len(kept), int(mask.sum()), int(removed.sum()), n, replaced]
    return out, stats


def same_partition(comp, other):
    """comp (-1 on background) and `other` (0 on background, any positive ids: scipy.ndimage.label) describe the same partition"""
    comp, other = np.asarray(comp).reshape(-1), np.asarray(other).reshape(-1)
    if not np.array_equal(comp >= 0, other > 0):
        return False
    pairs = set(zip(comp[comp >= 0].tolist(), other[comp >= 0].tolist()))
    return len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
