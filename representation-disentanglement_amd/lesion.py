"""Lesion-wise scoring of predicted label volumes -- the way BraTS ranks since 2023 -- and the binary dilation it needs, on the device where
`predict_volumes` leaves its labels (csrc/mrdis_lesion.hip).

    scores = mrdis.lesion_scores(labels, loader.target_ptrs(batch))           # lesion-wise Dice and HD95 of WT / TC / ET
    grown = mrdis.dilate3d(mask, iterations=3, connectivity=18)               # binary dilation

A region of a subject is split into lesions; every ground-truth lesion is scored against the predicted components that touch it, and every
predicted component that touches no lesion is a false positive.  Three per-voxel steps are kernels of their own -- the region membership
planes with their dilation (`region_planes`, `dilate`), the matching of predicted components to dilated lesions (`lesion_match`)
and the expansion of the matched sets into per-lesion masks (`lesion_expand`); the components come from `hip.cc_label`, the per-lesion
Dice and HD95 from `hip.region_surfaces` / `hip.surface_hist` under `region_scores`' rules.  Integer arithmetic throughout: exact, the same
bits from run to run.  What is left for the host is `lesion_scores_from_rows`: a handful of integers per lesion.
"""
import numpy as np
import torch

from . import hip
from .postproc import _volume
from .surfdist import BRATS_REGIONS, percentile_ranks, region_masks, scores_from_counts, _target_table

CONNECTIVITIES = hip.CC_CONNECTIVITIES
MAX_DILATION = hip.DILATE_MAX_ITERATIONS
COUNT_COLUMNS = ('lesions', 'kept', 'missed', 'components', 'fp')      # counts[b, r]: lesions, kept lesions, kept lesions with empty S_L, predicted components, FP
ROW_COLUMNS = ('b', 'r', 'id', 't', 's', 'i', 'k_t', 'k_s', 'kept')    # one row of `lesions`
# csv column prefix, key of the `lesion_scores` dict / column of its counts: the columns of predict_lesions.csv and seg_lesions.csv
LESION_CSV_KEYS = (('ldice', 'lesion_dice'), ('lhd95', 'lesion_hd95'), ('lesions', 0), ('kept', 1), ('missed', 2), ('comps', 3), ('fp', 4))


# ---------------------------------------------------------------- the binding of csrc/mrdis_lesion.hip (the ctypes table is hip._SIGS)
# Every tensor a kernel gets is checked here first, as hip.py checks its own (hip._want / hip._refuse: MrdisError before any launch).
def _region_mask_list(region_masks, what):
    masks = [int(m) for m in region_masks]
    if not 1 <= len(masks) <= hip.SURF_MAX_REGIONS or any(not 0 <= m <= 255 for m in masks):
        raise hip.MrdisError(f'{what}: 1 .. {hip.SURF_MAX_REGIONS} region masks in 0 .. 255, got {masks}')
    return masks


def region_planes(labels, target_ptrs, region_masks):
    """-> planes (B, H, W, D) uint8 on the device (include/mrdis.h mrdis_region_planes): bit r = the voxel lies in predicted region r, bit 4 + r
    = in ground-truth region r.  labels, target_ptrs, region_masks as `region_surfaces` takes them; the membership is the one it counts.  One launch."""
    lib = hip.load()
    B, H, W, D = hip._volume_u8(labels, 'region_planes: labels')
    hip._cc_geometry(B, H, W, D, 'region_planes')
    masks = _region_mask_list(region_masks, 'region_planes')
    target_ptrs is None or hip._want(target_ptrs, 'region_planes: target_ptrs', torch.int64, (B,), labels.device)
    planes = torch.empty((B, H, W, D), dtype=torch.uint8, device=labels.device)
    hip._chk(lib.mrdis_region_planes(hip._ptr(labels), hip._ptr(target_ptrs), (hip._I * len(masks))(*masks), len(masks), hip._ptr(planes), B, H, W, D, hip._stream()),
         'region_planes')
    return planes


def dilate(src, iterations=1, connectivity=18):
    """-> (B, H, W, D) uint8 on the device: src dilated `iterations` (1 .. 8) times by the 6 / 18 / 26 neighbourhood, every bit of a byte as a
    plane of its own (include/mrdis.h mrdis_dilate).  src (B, H, W, D) uint8 contiguous.  One launch per iteration."""
    lib = hip.load()
    B, H, W, D = hip._volume_u8(src, 'dilate: src')
    hip._cc_geometry(B, H, W, D, 'dilate')
    iterations, connectivity = int(iterations), int(connectivity)
    if not 1 <= iterations <= hip.DILATE_MAX_ITERATIONS or connectivity not in hip.CC_CONNECTIVITIES:
        raise hip.MrdisError(f'dilate: iterations in 1 .. {hip.DILATE_MAX_ITERATIONS} and connectivity in {hip.CC_CONNECTIVITIES}, got {iterations} and {connectivity}')
    dst = torch.empty((B, H, W, D), dtype=torch.uint8, device=src.device)
    nws = hip._ws_bytes(lib.mrdis_dilate_workspace, iterations, B, H, W, D)
    ws = torch.empty(nws, dtype=torch.uint8, device=src.device) if nws else None       # one byte per voxel: its own allocation, returned after the call
    hip._chk(lib.mrdis_dilate(hip._ptr(src), hip._ptr(dst), connectivity, iterations, hip._ptr(ws), nws, B, H, W, D, hip._stream()), 'dilate')
    return dst


def _lesion_operands(what, planes, comp_l, rank_l, comp_p, rank_p, first_p, R):
    B, H, W, D = hip._volume_u8(planes, f'{what}: planes')
    hip._cc_geometry(B, H, W, D, what)
    R = int(R)
    if not 1 <= R <= hip.SURF_MAX_REGIONS or B * R > 65535:
        raise hip.MrdisError(f'{what}: 1 .. {hip.SURF_MAX_REGIONS} regions and B R <= 65535, got R={R} B={B}')
    for name, t in (('comp_l', comp_l), ('rank_l', rank_l), ('comp_p', comp_p), ('rank_p', rank_p)):
        hip._want(t, f'{what}: {name}', torch.int32, (B * R, H, W, D), planes.device)
    hip._want(first_p, f'{what}: first_p', torch.int32, (B * R,), planes.device)
    return B, R, H, W, D


def lesion_match(planes, comp_l, rank_l, comp_p, rank_p, first_p, R, n_lesions, words):
    """-> (bits (n_lesions, words), tcount, root, item (n_lesions,)), int32 on the device (include/mrdis.h mrdis_lesion_match).  planes (B, H, W, D)
    as `region_planes` wrote them; comp_* / rank_* (B R, H, W, D) int32: the component ids `cc_label` made of the dilated ground-truth and of the
    predicted plane of every (sample, region) item, and at every root voxel its dense number; first_p (B R,) int32.  One launch."""
    lib = hip.load()
    B, R, H, W, D = _lesion_operands('lesion_match', planes, comp_l, rank_l, comp_p, rank_p, first_p, R)
    n_lesions, words = int(n_lesions), int(words)
    if n_lesions < 1 or not 1 <= words <= 1 << 20: hip._refuse(f'lesion_match: n_lesions {n_lesions}, words {words}', 'arg', planes)
    dev = planes.device
    bits = torch.zeros((n_lesions, words), dtype=torch.int32, device=dev)
    tcount = torch.zeros(n_lesions, dtype=torch.int32, device=dev)
    root = torch.full((n_lesions,), -1, dtype=torch.int32, device=dev)
    item = torch.full((n_lesions,), -1, dtype=torch.int32, device=dev)
    hip._chk(lib.mrdis_lesion_match(hip._ptr(planes), hip._ptr(comp_l), hip._ptr(rank_l), hip._ptr(comp_p), hip._ptr(rank_p), hip._ptr(first_p), words, n_lesions, hip._ptr(bits),
                                hip._ptr(tcount), hip._ptr(root), hip._ptr(item), B, R, H, W, D, hip._stream()), 'lesion_match')
    return bits, tcount, root, item


def lesion_expand(planes, comp_l, rank_l, comp_p, rank_p, first_p, R, bits, item, j0, n):
    """-> (stack_s, stack_t), both (n, H, W, D) uint8 0 / 1 on the device (include/mrdis.h mrdis_lesion_expand): the matched predicted
    components and the ground-truth voxels of lesions j0 .. j0 + n - 1; the other operands as `lesion_match` took and returned them.  One launch."""
    lib = hip.load()
    B, R, H, W, D = _lesion_operands('lesion_expand', planes, comp_l, rank_l, comp_p, rank_p, first_p, R)
    n_lesions, words = hip._want(bits, 'lesion_expand: bits', torch.int32, ('n_lesions', 'words'), planes.device)
    hip._want(item, 'lesion_expand: item', torch.int32, (n_lesions,), planes.device)
    j0, n = int(j0), int(n)
    if j0 < 0 or not 1 <= n <= 65535 or j0 + n > n_lesions or words < 1: hip._refuse(f'lesion_expand: lesions {j0} .. {j0 + n - 1} of {n_lesions}', 'arg', bits)
    stack_s = torch.empty((n, H, W, D), dtype=torch.uint8, device=planes.device)
    stack_t = torch.empty((n, H, W, D), dtype=torch.uint8, device=planes.device)
    hip._chk(lib.mrdis_lesion_expand(hip._ptr(planes), hip._ptr(comp_l), hip._ptr(rank_l), hip._ptr(comp_p), hip._ptr(rank_p), hip._ptr(first_p), hip._ptr(bits), words, hip._ptr(item),
                                 n_lesions, j0, n, hip._ptr(stack_s), hip._ptr(stack_t), B, R, H, W, D, hip._stream()), 'lesion_expand')
    return stack_s, stack_t


# ---------------------------------------------------------------- the public functions
def _int_arg(name, val, lo, hi=None):
    if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or val < lo or (hi is not None and val > hi):
        raise ValueError(f'{name} {val!r}: an integer ' + (f'in {lo} .. {hi}' if hi is not None else f'>= {lo}'))
    return int(val)


def dilate3d(mask, iterations=1, connectivity=18):
    """Binary dilation: uint8, the shape of `mask`.  mask: a (B, H, W, D) or (H, W, D) bool / uint8 device tensor (as `edt3d_sq` takes it); B in
    1 .. 65535, each of H, W, D in 1 .. 1024 (else MrdisError('... unsupported geometry ...'), before any launch).  The structuring element is
    the voxel with its 6 face neighbours (connectivity 6), plus its 12 edge neighbours (18: scipy's generate_binary_structure(3, 2)) or the full
    3 x 3 x 3 cube (26), applied `iterations` (1 .. 8) times -- iterated, not a ball.  Outside the volume is background; nothing wraps around a
    border or crosses into another sample.  Every bit of a byte dilates as a plane of its own: a bool or 0 / 1 mask gives a 0 / 1 mask, a uint8
    volume of flags the OR of each flag over the neighbourhood.  One kernel launch per iteration (`dilate`; counter 'dilate'), no host sync.
    ValueError for iterations outside 1 .. 8 or a connectivity not in {6, 18, 26}."""
    iterations = _int_arg('iterations', iterations, 1, MAX_DILATION)
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f'connectivity {connectivity!r}: one of {CONNECTIVITIES}')
    v, squeeze = _volume(mask, 'dilate3d')
    out = dilate(v, iterations, int(connectivity))
    return out[0] if squeeze else out


def lesion_scores_from_rows(rows, dice_each, hd95_each, counts, shape, spacing=1.0, has_target=None):
    """The host half of `lesion_scores`: per-lesion scores -> (lesion_dice, lesion_hd95), float64 CPU tensors (B, R).  rows (n, 9) integers
    `[b, r, lesion id, |T_L|, |S_L|, |S_L and T_L|, k at T's surface, k at S's surface, kept]` in (b, r, id) order, dice_each / hd95_each (n,)
    the scores of every lesion, counts (B, R, 5) = [lesions, kept lesions, kept lesions with empty S_L, predicted components, FP components],
    shape = (H, W, D) of the WHOLE volume (the penalty), has_target (B,) bools (None: all).  With K the kept lesions and F the FP components:
      lesion_dice = sum_K dice_L / (|K| + F),  lesion_hd95 = (sum_K hd95_L + F * penalty) / (|K| + F),  penalty = spacing * sqrt(H^2 + W^2 + D^2);
      |K| + F = 0: dice 1, hd95 0;  no ground truth for the sample: NaN in both.  Sums in float64, in row (= lesion id) order."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, len(ROW_COLUMNS))
    counts = np.asarray(counts, dtype=np.int64)
    B, R = counts.shape[:2]
    H, W, D = (int(x) for x in shape)
    f = np.float64
    penalty = f(spacing) * np.sqrt(f(H * H + W * W + D * D))
    sd, sh = np.zeros((B, R), dtype=f), np.zeros((B, R), dtype=f)
    for i in range(rows.shape[0]):                                   # (row order: float sums depend on it)
        if rows[i, 8]:
            sd[rows[i, 0], rows[i, 1]] += f(dice_each[i])
            sh[rows[i, 0], rows[i, 1]] += f(hd95_each[i])
    den = counts[..., 1] + counts[..., 4]
    fp = counts[..., 4].astype(f)
    with np.errstate(divide='ignore', invalid='ignore'):
        dice = np.where(den > 0, sd / den.astype(f), 1.0)
        hd = np.where(den > 0, (sh + fp * penalty) / den.astype(f), 0.0)
    if has_target is not None:
        none = ~np.asarray(has_target).astype(bool)
        dice = np.where(none[:, None], np.nan, dice)
        hd = np.where(none[:, None], np.nan, hd)
    return torch.from_numpy(np.ascontiguousarray(dice, dtype=f)), torch.from_numpy(np.ascontiguousarray(hd, dtype=f))


def _pair_counts(stack_s, stack_t):
    """(counts (n, 5), ranks (n, 2)) int64 on the device of n mask pairs under `region_scores`' rules: its entry points on (S_L, T_L) as one region"""
    ptrs, keep = _target_table(stack_t, stack_s)
    flags, counts = hip.region_surfaces(stack_s, ptrs, (2,))
    hist = hip.surface_hist(flags, 1)
    n = torch.stack([counts[..., 4], counts[..., 3]], dim=-1)
    ranks = percentile_ranks(hist, n)
    del keep
    return counts.to(torch.int64)[:, 0], ranks[:, 0]


def _crop_pair(stack_s, stack_t):
    """both (n, H, W, D) stacks cut to the joint bounding box of their non-zero voxels, padded by one voxel where the volume goes on: surfaces
    (a voxel beyond the volume and a voxel of the padding are both outside every mask), counts and distances are what they were.  One small
    D2H copy (the occupied planes along each axis); the stacks as they are if the box is the volume or nothing is set."""
    both = stack_s | stack_t
    n, H, W, D = both.shape
    vol = both.max(dim=0).values
    hw = vol.max(dim=2).values
    occ = torch.cat([hw.max(dim=1).values, hw.max(dim=0).values, vol.max(dim=0).values.max(dim=0).values]).cpu().numpy()
    box = []
    for lo, ext in ((0, H), (H, W), (H + W, D)):
        idx = np.flatnonzero(occ[lo:lo + ext])
        if idx.size == 0:
            return stack_s, stack_t
        box.append((max(int(idx[0]) - 1, 0), min(int(idx[-1]) + 2, ext)))
    (h0, h1), (w0, w1), (d0, d1) = box
    if (h1 - h0, w1 - w0, d1 - d0) == (H, W, D):
        return stack_s, stack_t
    return stack_s[:, h0:h1, w0:w1, d0:d1].contiguous(), stack_t[:, h0:h1, w0:w1, d0:d1].contiguous()


def lesion_scores(labels, targets, regions=BRATS_REGIONS, dilation=3, min_voxels=50, spacing=1.0, max_items=8, crop=True):
    """Lesion-wise Dice and HD95 of predicted label volumes by region.  labels, targets, regions, spacing: as `region_scores` takes them (region
    membership is exactly its: label values 0 .. 7, a non-integral or larger ground-truth value belongs to no region, a pointer of 0 means no
    ground truth).  dilation in 0 .. 8, min_voxels >= 0, max_items >= 1 (ValueError before any launch otherwise).  crop: score every chunk of
    lesions inside the joint bounding box of its masks, padded by one voxel -- the same bits as on the whole volume, less distance-transform work.

    -> {'lesion_dice', 'lesion_hd95': float64 CPU (B, R); 'counts': int64 CPU (B, R, 5) = [lesions, kept lesions, kept lesions with empty S_L,
    predicted components, FP components]; 'lesions': int64 CPU (n, 9) rows [b, r, lesion id, |T_L|, |S_L|, |S_L and T_L|, k at T's surface, k at
    S's surface, kept] in (b, r, id) order, k the squared nearest-rank 95 % distances of `region_scores`; 'lesion_dice_each', 'lesion_hd95_each':
    float64 (n,); 'names'}

    The rules are THIS PACKAGE'S CONVENTION, modelled on the BraTS 2023 lesion-wise ranking (which uses a constant 374 where this package uses
    its own penalty).  Per sample and region, with P the predicted and T the ground-truth voxels of the region:
      1. Tdil is T dilated `dilation` times by the 18-neighbourhood (`dilate3d`).
      2. The lesions are the 26-connected components of Tdil; lesion L owns T_L = T and L; its id is the component's root index as
         `components3d` defines it, and lesions are ordered by it.  (Equal to labelling T, dilating every component and merging the components
         whose dilations connect.)  dilation = 0: the components of T itself.
      3. The predicted components are the 26-connected components of P.  Component C matches lesion L iff C meets the dilated L; S_L is the
         union of the components that match L.  A component may match several lesions and then belongs to each S_L; one that matches none is a
         false positive (FP), whatever its size.
      4. dice_L and hd95_L are `region_scores`' rules on (S_L, T_L); S_L empty: dice 0, hd95 = spacing * sqrt(H^2 + W^2 + D^2) (the penalty).
      5. L is kept iff |T_L| >= min_voxels; a lesion that is not kept leaves the sums and the denominator, the components it matched are still not FP.
      6. lesion_dice = sum_K dice_L / (|K| + F), lesion_hd95 = (sum_K hd95_L + F * penalty) / (|K| + F) over the kept lesions K and the F false
         positives; |K| + F = 0: dice 1, hd95 0; no ground truth for the sample: NaN in both (`lesion_scores_from_rows`).

    Launches: one for the planes and `dilation` for the dilation ('dilate'), two `hip.cc_label` calls, one `lesion_match` (none if the batch holds no lesion); then per chunk of
    at most `max_items` lesions one `lesion_expand`, one `hip.region_surfaces` and one `hip.surface_hist` (about 107 MB of workspace per
    lesion of the chunk at BraTS size on the whole volume; the crop cuts it to the chunk's bounding box).  The dense lesion and component numbers are a running sum over the root voxels (torch, on the device);
    one small D2H copy brings the lesion and component counts that size the matching, one the matching's integers, and per chunk one the
    bounding box (with `crop`) and one the lesions' integers."""
    names, masks = region_masks(regions)
    dilation = _int_arg('dilation', dilation, 0, MAX_DILATION)
    min_voxels = _int_arg('min_voxels', min_voxels, 0)
    max_items = _int_arg('max_items', max_items, 1)
    B, H, W, D = hip._volume_u8(labels, 'lesion_scores: labels')
    hip._cc_geometry(B, H, W, D, 'lesion_scores')
    hip._edt_geometry(min(max_items, 65535), H, W, D, 'lesion_scores')
    R, P, dev = len(masks), H * W * D, labels.device
    if B * R > 65535:
        raise hip.MrdisError(f'lesion_scores: unsupported geometry {(B, H, W, D)}: B R <= 65535 with R = {R} regions')
    ptrs, keep = _target_table(targets, labels)
    planes = region_planes(labels, ptrs, masks)
    del keep
    grown = dilate(planes, dilation, 18) if dilation else planes
    shifts = torch.arange(R, dtype=torch.uint8, device=dev).view(1, R, 1, 1, 1)
    # the (B R, H, W, D) stacks of 0 / 1 planes `cc_label` reads with fg = (1,): item = b R + r
    comp_p, size_p = hip.cc_label(((planes.unsqueeze(1) >> shifts) & 1).view(B * R, H, W, D), 2, 26)
    comp_l, size_l = hip.cc_label(((grown.unsqueeze(1) >> (shifts + 4)) & 1).view(B * R, H, W, D), 2, 26)
    del grown
    # dense numbers: the rank of a root voxel among the roots, in (item, root index) order -- a running sum, written over `size` (read at roots only)
    ends = torch.arange(1, B * R + 1, device=dev) * P - 1
    rank_p = torch.cumsum((size_p > 0).view(-1), 0, dtype=torch.int32)
    rank_l = torch.cumsum((size_l > 0).view(-1), 0, dtype=torch.int32)
    del size_p, size_l
    cum = torch.stack([rank_l[ends], rank_p[ends], (ptrs != 0).to(torch.int32).repeat_interleave(R)]).cpu().numpy().astype(np.int64)
    rank_p, rank_l = (rank_p - 1).view(B * R, H, W, D), (rank_l - 1).view(B * R, H, W, D)
    n_l = np.diff(cum[0], prepend=0)                                 # lesions / predicted components of every item
    n_p = np.diff(cum[1], prepend=0)
    has_target = cum[2].reshape(B, R)[:, 0] != 0
    total = int(cum[0, -1])
    counts = np.zeros((B, R, 5), dtype=np.int64)
    counts[..., 0] = n_l.reshape(B, R)
    counts[..., 3] = n_p.reshape(B, R)
    counts[..., 4] = counts[..., 3]                                  # (no lesion: every component is a false positive)
    rows = np.zeros((total, len(ROW_COLUMNS)), dtype=np.int64)
    dice_each, hd_each = np.zeros(total), np.zeros(total)
    if total:
        first_p = torch.from_numpy(np.concatenate([[0], cum[1, :-1]]).astype(np.int32)).to(dev)
        words = max(1, (int(n_p.max()) + 31) // 32)
        bits, tcount, root, item = lesion_match(planes, comp_l, rank_l, comp_p, rank_p, first_p, R, total, words)
        host = torch.cat([tcount, root, item, bits.view(-1)]).cpu().numpy()
        t_n, root_h, item_h = host[:total].astype(np.int64), host[total:2 * total].astype(np.int64), host[2 * total:3 * total].astype(np.int64)
        bits_h = host[3 * total:].reshape(total, words).view(np.uint32)
        if (item_h != np.repeat(np.arange(B * R), n_l)).any():
            raise hip.MrdisError('lesion_scores: the matching did not see every lesion root it was sized for')
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = item_h // R, item_h % R, root_h, t_n
        rows[:, 8] = t_n >= min_voxels
        for it in range(B * R):                                      # false positives: the components no row of the item names
            sel = bits_h[item_h == it]
            hit = int(sum(bin(int(w)).count('1') for w in np.bitwise_or.reduce(sel, axis=0))) if sel.shape[0] else 0
            counts[it // R, it % R, 4] = n_p[it] - hit
        for j0 in range(0, total, max_items):
            n = min(max_items, total - j0)
            stack_s, stack_t = lesion_expand(planes, comp_l, rank_l, comp_p, rank_p, first_p, R, bits, item, j0, n)
            if crop:
                stack_s, stack_t = _crop_pair(stack_s, stack_t)     # (the penalty below still uses the whole volume's shape)
            c, k = _pair_counts(stack_s, stack_t)
            del stack_s, stack_t
            ck = torch.cat([c.reshape(-1), k.reshape(-1)]).cpu().numpy()
            c, k = ck[:n * 5].reshape(n, 1, 5), ck[n * 5:].reshape(n, 1, 2)
            sc = scores_from_counts(c, k, (H, W, D), spacing)
            rows[j0:j0 + n, 4], rows[j0:j0 + n, 5] = c[:, 0, 1], c[:, 0, 0]
            rows[j0:j0 + n, 6:8] = k[:, 0]
            dice_each[j0:j0 + n], hd_each[j0:j0 + n] = sc['dice'][:, 0].numpy(), sc['hd95'][:, 0].numpy()
            if (c[:, 0, 2] != t_n[j0:j0 + n]).any():
                raise hip.MrdisError('lesion_scores: the expanded ground-truth masks do not hold the voxels the matching counted')
        kept = rows[:, 8] != 0
        np.add.at(counts[..., 1], (rows[kept, 0], rows[kept, 1]), 1)
        missed = kept & (rows[:, 4] == 0)
        np.add.at(counts[..., 2], (rows[missed, 0], rows[missed, 1]), 1)
    dice, hd = lesion_scores_from_rows(rows, dice_each, hd_each, counts, (H, W, D), spacing, has_target)
    return {'lesion_dice': dice, 'lesion_hd95': hd, 'counts': torch.from_numpy(counts), 'lesions': torch.from_numpy(rows),
            'lesion_dice_each': torch.from_numpy(dice_each), 'lesion_hd95_each': torch.from_numpy(hd_each), 'names': names}


def lesion_csv_header(regions=BRATS_REGIONS):
    return ','.join(f'{col}_{name}' for col, _ in LESION_CSV_KEYS for name, _ in regions)


def lesion_csv_values(scores, i):
    """the values of sample i of a `lesion_scores` dict in the order of `lesion_csv_header`: floats written with repr, counts as integers"""
    out = []
    for _, key in LESION_CSV_KEYS:
        src = scores[key][i] if isinstance(key, str) else scores['counts'][i, :, key]
        out += [repr(float(v)) if isinstance(key, str) else str(int(v)) for v in src.tolist()]
    return out
