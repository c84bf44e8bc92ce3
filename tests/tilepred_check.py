"""Float64 oracle of the tile-wise prediction rule (include/mrdis.h: mrdis_tile_accum, mrdis_tile_label_volume; model3d.predict_tiles), shared by
tests/test_tilepred_cpu.py and tests/test_gpu_tilepred.py.  Nothing here imports the package: offsets, views, weights and sums are written out
again from the rule, so a slip in model3d shows as a difference.

The rule's fp32 quantities are INPUTS of the oracle, formed with the rule's own roundings: the axis weights (float64 formula, rounded once) and
the weight of a tile position, (wh[i] * ww[j]) * wd[k] in fp32.  Everything summed -- probabilities and weights -- is summed in float64, and
the denominator is the brute-force sum of the position weights over every (tile, view) that reaches a voxel, not the product of axis sums:
the factorisation the kernels rely on is tested against it.
"""
import itertools

import numpy as np
import torch

FLIP_H, FLIP_W, FLIP_D = 1, 4, 8
FLIP_BITS = {'h': FLIP_H, 'w': FLIP_W, 'd': FLIP_D}
FLOOR = 2.0 ** -20
EXCUSED_SHARE = 1e-3
SEED = 12

# case -> B, C, volume, tile, stride, the mirror strings it runs with (the issue's table)
CASES = {
    'main': dict(B=2, C=3, shape=(9, 10, 37), tile=(6, 8, 16), stride=(3, 4, 8), mirrors=('', 'h', 'wd', 'hwd')),
    'c1': dict(B=3, C=1, shape=(9, 10, 37), tile=(6, 8, 16), stride=(3, 4, 8), mirrors=('', 'h', 'wd', 'hwd')),
    'elements': dict(B=1, C=1, shape=(3, 5, 7), tile=(2, 3, 3), stride=(1, 2, 2), mirrors=('', 'd')),
    'vectors': dict(B=2, C=4, shape=(4, 6, 16), tile=(4, 4, 8), stride=(4, 2, 8), mirrors=('', 'w')),
    'allviews': dict(B=1, C=3, shape=(6, 6, 10), tile=(4, 4, 8), stride=(2, 2, 2), mirrors=('hwd',)),
}
CASE_VIEWS = [(name, m) for name, c in CASES.items() for m in c['mirrors']]


def offsets(n, T, S):
    """0, S, 2 S, ... below n - T, then n - T"""
    out = []
    o = 0
    while o < n - T:
        out.append(o)
        o += S
    return out + [n - T]


def views(mirror):
    """flag masks in launch order: binary count over the named axes in h, w, d order, the first named axis the lowest bit"""
    axes = [a for a in 'hwd' if a in mirror]
    out = []
    for v in range(2 ** len(axes)):
        out.append(sum(FLIP_BITS[a] for i, a in enumerate(axes) if (v // 2 ** i) % 2))
    return out


def weights(T, kind, sigma=0.125, rng=None):
    """(T,) float32.  'random': positive and asymmetric (a weight indexed on the mirrored side shows)"""
    if kind == 'uniform':
        return np.ones(T, dtype=np.float32)
    if kind == 'random':
        return (0.25 + rng.random(T)).astype(np.float32)
    x = np.arange(T, dtype=np.float64)
    g = np.exp(-0.5 * ((x - (T - 1) / 2) / (sigma * T)) ** 2)
    return np.maximum(g, FLOOR).astype(np.float32)


def position_weights(w):
    """(TH, TW, TD) float32: (wh[i] * ww[j]) * wd[k] with both roundings in fp32"""
    hw = (w[0][:, None] * w[1][None, :]).astype(np.float32)
    return (hw[:, :, None] * w[2][None, None, :]).astype(np.float32)


def axis_norm(n, T, offs, w, scale=1):
    """float64 sum of the fp32 axis weights over the offsets, times scale, rounded once"""
    s = np.zeros(n, dtype=np.float64)
    for o in offs:
        s[o:o + T] += w.astype(np.float64)
    return (s * scale).astype(np.float32)


def make_case(name, mirror, kind='gaussian', sigma=0.125, seed=SEED, labels_max=3):
    """seeded CPU inputs: one fresh (B, TH, TW, TD, C) logits tensor, 3 * randn, per (tile, view) in launch order (h0 outermost, d0 innermost,
    views innermost of all), raw (B, H, W, D) label volumes, the axis weights"""
    c = dict(CASES[name])
    c['name'], c['mirror'], c['kind'] = name, mirror, kind
    g = torch.Generator().manual_seed(seed)
    c['offsets'] = [offsets(n, t, s) for n, t, s in zip(c['shape'], c['tile'], c['stride'])]
    c['views'] = views(mirror)
    c['geom'] = [(o, v) for o in itertools.product(*c['offsets']) for v in c['views']]
    c['logits'] = [3 * torch.randn(c['B'], *c['tile'], c['C'], generator=g) for _ in c['geom']]
    c['tvol'] = torch.randint(0, labels_max + 1, (c['B'], *c['shape']), generator=g).float()
    rng = np.random.default_rng(seed)
    c['w'] = [weights(t, kind, sigma, rng) for t in c['tile']]
    c['norms'] = [axis_norm(n, t, o, w, len(c['views']) if a == 2 else 1) for a, (n, t, o, w) in enumerate(zip(c['shape'], c['tile'], c['offsets'], c['w']))]
    return c


def unmirror(p, flips):
    """a (B, TH, TW, TD, C) array of a mirrored view put back"""
    axes = [a for a, bit in ((1, FLIP_H), (2, FLIP_W), (3, FLIP_D)) if flips & bit]
    return np.flip(p, axes) if axes else p


def oracle_acc(c, geom=None, logits=None):
    """-> acc64 (B, H, W, D, C): float64 sum of weight * float64 sigmoid; den64 (H, W, D): float64 sum of the position weights (brute force);
    n_acc (H, W, D): accumulations per voxel"""
    geom = c['geom'] if geom is None else geom
    logits = c['logits'] if logits is None else logits
    H, W, D = c['shape']
    TH, TW, TD = c['tile']
    w3 = position_weights(c['w']).astype(np.float64)
    acc = np.zeros((c['B'], H, W, D, c['C']), dtype=np.float64)
    den = np.zeros((H, W, D), dtype=np.float64)
    n_acc = np.zeros((H, W, D), dtype=np.int64)
    for ((h0, w0, d0), v), l in zip(geom, logits):
        p = 1.0 / (1.0 + np.exp(-l.numpy().astype(np.float64)))
        acc[:, h0:h0 + TH, w0:w0 + TW, d0:d0 + TD] += w3[None, ..., None] * unmirror(p, v)
        den[h0:h0 + TH, w0:w0 + TW, d0:d0 + TD] += w3
        n_acc[h0:h0 + TH, w0:w0 + TW, d0:d0 + TD] += 1
    return acc, den, n_acc


def excuse_bound(n_acc):
    """8 (n_acc + 1) 2^-24: per accumulation about 3.5 units of 2^-24 (sigmoid and fma), 3 more for the denominator and the division, doubled"""
    return 8.0 * (int(n_acc) + 1) * 2.0 ** -24


def oracle_labels(acc64, den64, tvol, relabel, bound):
    """float64 rule -> labels (B, H, W, D) int64, predicted / labelled masks (B, H, W, D, C), excused voxels (B, H, W, D); all numpy"""
    d = den64[None, ..., None]
    pbar = np.where(d > 0, acc64 / np.where(d > 0, d, 1.0), 0.0)
    C = acc64.shape[-1]
    t = tvol.numpy().copy()
    if relabel:
        t[t == 4] = 3
    pred = pbar > 0.5
    lab = np.stack([t == k + 1 for k in range(C)], axis=-1)
    arg = np.argmax(pbar, axis=-1)                                                 # the first maximum
    labels = np.where(pbar.max(-1) > 0.5, arg + 1, 0)
    if relabel:
        labels[labels == 3] = 4
    excused = (np.abs(pbar - 0.5) < bound).any(-1)
    if C > 1:
        top = np.sort(pbar, axis=-1)
        excused |= (top[..., -1] - top[..., -2]) < bound
    excused &= (den64 > 0)[None]
    return labels, pred, lab, excused


def counts_of(pred, lab, keep):
    """(B, C, 3) [I, P, T] over the voxels `keep` (B, H, W, D)"""
    k = keep[..., None]
    f = lambda m: (m & k).reshape(m.shape[0], -1, m.shape[-1]).sum(1)
    return np.stack([f(pred & lab), f(pred), f(lab)], axis=-1)


def assert_labels_counts(labels, counts, want, pred, lab, excused, what):
    """labels (B, H, W, D) and counts (B, C, 3) as CPU tensors against the oracle, outside the excused voxels"""
    labels, counts = labels.numpy().astype(np.int64), counts.numpy().astype(np.int64)
    n_exc = int(excused.sum())
    assert n_exc <= EXCUSED_SHARE * excused.size, f'{what}: {n_exc} of {excused.size} voxels excused'
    bad = (labels != want) & ~excused
    assert int(bad.sum()) == 0, f'{what}: {int(bad.sum())} labels differ outside the excused voxels'
    lo = counts_of(pred, lab, ~excused)
    hi = lo + excused.reshape(excused.shape[0], -1).sum(1)[:, None, None]
    assert bool(((counts >= lo) & (counts <= hi)).all()), f'{what}: counts {counts.tolist()} outside [{lo.tolist()}, {hi.tolist()}]'
    assert np.array_equal(counts[..., 2], counts_of(pred, lab, np.ones_like(excused))[..., 2]), what      # T never depends on a probability
