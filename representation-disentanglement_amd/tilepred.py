"""Tile-wise prediction of the 3-D nets on the device (csrc/mrdis_segvol.hip: mrdis_tile_accum, mrdis_tile_label_volume): the binding.  The rule
-- tile origins, mirrored views, separable weights, the fp32 order of the accumulation and the normalisation by three axis sums -- is stated in
include/mrdis.h and is THIS PACKAGE'S CONVENTION: the reference ships no 3-D inference.  The host side is model3d.predict_tiles.

    acc = torch.zeros(B, H, W, D, C)
    tile_accum(net(tile)[0], acc, (wh, ww, wd), (h0, w0, d0), flips)          # per tile and view, in launch order
    labels, counts = tile_label_volume(acc, (nh, nw, nd), target_ptrs, relabel=True)

The ctypes table is hip._SIGS; the package also binds both functions as hip.tile_accum / hip.tile_label_volume.  Every tensor a kernel gets is
checked here first, as hip.py checks its own (hip._want / hip._refuse: MrdisError before any launch); nothing is copied.
"""
import torch

from . import hip


def _int_triple(v, what):
    """three integers, else MrdisError"""
    try:
        a, b, c = (int(x) for x in v)
    except (TypeError, ValueError):
        raise hip.MrdisError(f'{what}: {v!r}: three integers') from None
    return a, b, c


def tile_accum(logits, acc, weights, origin, flips=0):
    """acc[:, h0 + i, w0 + j, d0 + k, :] = fma((wh[i] * ww[j]) * wd[k], sigmoid(logits), acc), the logits un-mirrored along the axes of `flips`
    (bits 1 = h | 4 = w | 8 = d) (include/mrdis.h mrdis_tile_accum), in place; returns acc.  logits (B, C, TH, TW, TD) fp32 dense
    channels-last-3d (the net's output for one tile), acc (B, H, W, D, C) fp32 contiguous, weights = (wh (TH,), ww (TW,), wd (TD,)) fp32 on the
    device, origin = (h0, w0, d0).  Any other layout, a tile that does not fit, an origin outside the volume or other flip bits raise
    MrdisError: nothing is copied.  One launch."""
    lib = hip.load()
    B, C, TH, TW, TD = hip._want(logits, 'tile_accum: logits', torch.float32, ('B', 'C', 'TH', 'TW', 'TD'), cl=True)
    _, H, W, D, _ = hip._want(acc, 'tile_accum: acc', torch.float32, (B, 'H', 'W', 'D', C), logits.device)
    try:
        wh, ww, wd = weights
    except (TypeError, ValueError):
        raise hip.MrdisError(f'tile_accum: weights {type(weights).__name__}: the three vectors (wh, ww, wd)') from None
    for w, n, name in ((wh, TH, 'wh'), (ww, TW, 'ww'), (wd, TD, 'wd')):
        hip._want(w, f'tile_accum: weights {name}', torch.float32, (n,), logits.device)
    h0, w0, d0 = _int_triple(origin, 'tile_accum: origin')
    if isinstance(flips, bool) or not isinstance(flips, int) or flips & ~hip.TILE_FLIPS: hip._refuse('tile_accum: flips of the bits 1 | 4 | 8', 'arg', flips)
    if TH > H or TW > W or TD > D or not (0 <= h0 <= H - TH and 0 <= w0 <= W - TW and 0 <= d0 <= D - TD):
        hip._refuse(f'tile_accum: a tile inside the volume, origin {(h0, w0, d0)}', 'arg', logits, acc)
    hip._chk(lib.mrdis_tile_accum(hip._ptr(logits), hip._ptr(acc), hip._ptr(wh), hip._ptr(ww), hip._ptr(wd), B, H, W, D, TH, TW, TD, C, h0, w0, d0, flips, hip._stream()), 'tile_accum')
    return acc


def tile_label_volume(acc, norms, target_ptrs=None, relabel=False):
    """-> (labels (B, H, W, D) uint8, counts (B, C, 3) int32), both on the device (include/mrdis.h mrdis_tile_label_volume): `seg_label_volume`
    with the denominator (nh[h] * nw[w]) * nd[d].  acc (B, H, W, D, C) fp32 contiguous as `tile_accum` leaves it, norms = (nh (H,), nw (W,),
    nd (D,)) fp32 on the device, target_ptrs as there.  A tensor that is not dense in that layout raises MrdisError; nothing is copied."""
    lib = hip.load()
    B, H, W, D, C = hip._want(acc, 'tile_label_volume: acc', torch.float32, ('B', 'H', 'W', 'D', 'C'))
    try:
        nh, nw, nd = norms
    except (TypeError, ValueError):
        raise hip.MrdisError(f'tile_label_volume: norms {type(norms).__name__}: the three vectors (nh, nw, nd)') from None
    for v, n, name in ((nh, H, 'nh'), (nw, W, 'nw'), (nd, D, 'nd')):
        hip._want(v, f'tile_label_volume: norms {name}', torch.float32, (n,), acc.device)
    target_ptrs is None or hip._want(target_ptrs, 'tile_label_volume: target_ptrs', torch.int64, (B,), acc.device)
    labels = torch.empty((B, H, W, D), dtype=torch.uint8, device=acc.device)
    counts = torch.zeros((B, C, 3), dtype=torch.int32, device=acc.device)
    hip._chk(lib.mrdis_tile_label_volume(hip._ptr(acc), hip._ptr(nh), hip._ptr(nw), hip._ptr(nd), hip._ptr(target_ptrs), hip._ptr(labels), hip._ptr(counts), B, H, W, D, C,
                                     int(bool(relabel)), hip._stream()), 'tile_label_volume')
    return labels, counts
