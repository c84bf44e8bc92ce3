"""Region scoring of predicted label volumes the way BraTS reports them: Dice, sensitivity, specificity and the 95th-percentile Hausdorff
distance (HD95) of nested regions, on the device where `predict_volumes` leaves its labels (csrc/mrdis_surfdist.hip).

    scores = mrdis.region_scores(labels, loader.target_ptrs(batch))          # WT / TC / ET
    d2 = mrdis.edt3d_sq(mask)                                                # exact squared Euclidean distance transform

The per-voxel work is three entry points of the library, integer arithmetic throughout (exact, the same bits from run to run):
`hip.region_surfaces` (surface voxels of every region of prediction and ground truth, and the overlap counts, in one pass),
`hip.surface_hist` (the distance transform of every surface, whose last pass adds the squared distance at the other surface's voxels into a
histogram instead of storing it) and `hip.edt_sq` (the transform alone).  What is left for the host is `scores_from_counts`: a handful of
integers per sample and region.
"""
import numpy as np
import torch

from . import hip

EDT_FAR = hip.EDT_FAR
# BraTS's nested regions over its labels 1 (necrotic core), 2 (oedema), 4 (enhancing): whole tumour, tumour core, enhancing tumour
BRATS_REGIONS = (('wt', (1, 2, 4)), ('tc', (1, 4)), ('et', (4,)))
SCORE_KEYS = ('dice', 'sensitivity', 'specificity', 'hd95')


def region_masks(regions):
    """((name, labels), ...) -> (names, masks): bit l of masks[r] is set iff label l belongs to region r; labels are integers in 0 .. 7"""
    regions = tuple(regions)
    if not 1 <= len(regions) <= hip.SURF_MAX_REGIONS:
        raise ValueError(f'1 .. {hip.SURF_MAX_REGIONS} regions, got {len(regions)}')
    names, masks = [], []
    for name, labels in regions:
        labels = [int(l) for l in labels]
        if not labels or any(not 0 <= l <= 7 for l in labels):
            raise ValueError(f'region {name!r}: labels in 0 .. 7, got {labels}')
        names.append(str(name))
        masks.append(sum(1 << l for l in set(labels)))
    return tuple(names), tuple(masks)


def edt3d_sq(mask):
    """Exact squared Euclidean distance transform: int32, the shape of `mask`; at every voxel the squared distance (voxel units) to the nearest
    non-zero voxel of the same batch item, 0 on such a voxel and `EDT_FAR` (2^30) everywhere in an item without one.  `mask`: a (B, H, W, D)
    or (H, W, D) bool / uint8 device tensor, each of H, W, D in 1 .. 1024 (else MrdisError('... unsupported geometry ...')).  Three kernel
    launches whatever B (hip.edt_sq; counter 'edt')."""
    if mask.dim() not in (3, 4) or mask.dtype not in (torch.bool, torch.uint8):
        raise hip.MrdisError(f'edt3d_sq: a (B, H, W, D) or (H, W, D) bool / uint8 tensor, got {mask.dtype} {tuple(mask.shape)}')
    m = mask if mask.dim() == 4 else mask[None]
    if 0 in m.shape:
        raise hip.MrdisError(f'edt3d_sq: unsupported geometry {tuple(m.shape)}')
    m = m.contiguous()
    out = hip.edt_sq(m.view(torch.uint8) if m.dtype is torch.bool else m)[0]
    return out if mask.dim() == 4 else out[0]


def percentile_ranks(hist, n):
    """The nearest-rank 95th percentile of squared distances, decided in integers: for every row of `hist` (..., bins) the smallest k with
    20 * cum[k] >= 19 * n, cum the running sum of the row and `n` (...) the number of measured voxels (the row's total).  int64 (...);
    0 for a row with n = 0.  Torch ops on whatever device `hist` lives on."""
    cum = torch.cumsum(hist.to(torch.int64), dim=-1)
    reached = 20 * cum >= 19 * n.to(torch.int64).unsqueeze(-1)
    return torch.argmax(reached.to(torch.uint8), dim=-1)            # the first True (argmax returns the first maximum)


def scores_from_counts(counts, ranks, shape, spacing=1.0, has_target=None):
    """The host half of `region_scores`: integers -> float64 scores.  counts (B, R, 5) = [I = |P and T|, P, T, surface voxels of P, of T],
    ranks (B, R, 2) = the squared nearest-rank 95 % distances [at T's surface to P, at P's surface to T], shape = (H, W, D),
    has_target (B,) bools (None: all).  The rules -- this package's convention -- are those of `region_scores`."""
    c = np.asarray(counts).astype(np.int64)
    k = np.asarray(ranks).astype(np.int64)
    H, W, D = (int(x) for x in shape)
    n = H * W * D
    i, p, t = c[..., 0], c[..., 1], c[..., 2]
    f = np.float64
    with np.errstate(divide='ignore', invalid='ignore'):
        dice = np.where(p + t > 0, 2.0 * i.astype(f) / (p + t).astype(f), 1.0)
        sens = np.where(t > 0, i.astype(f) / t.astype(f), 1.0)
        spec = np.where(n - t > 0, (n - p - t + i).astype(f) / (n - t).astype(f), 1.0)
    hd = f(spacing) * np.sqrt(k.max(axis=-1).astype(f))
    one_empty = (p == 0) != (t == 0)
    both_empty = (p == 0) & (t == 0)
    hd = np.where(one_empty, f(spacing) * np.sqrt(f(H * H + W * W + D * D)), hd)
    hd = np.where(both_empty, 0.0, hd)
    out = {'dice': dice, 'sensitivity': sens, 'specificity': spec, 'hd95': hd}
    if has_target is not None:
        none = ~np.asarray(has_target).astype(bool)
        for key in SCORE_KEYS:
            out[key] = np.where(none[:, None], np.nan, out[key])
    return {key: torch.from_numpy(np.ascontiguousarray(out[key], dtype=f)) for key in SCORE_KEYS}


def _target_table(targets, labels):
    """(pointer table (B,) int64 on the device or None, what must stay alive until the kernels ran)"""
    B = labels.shape[0]
    if targets is None:
        return torch.zeros(B, dtype=torch.int64, device=labels.device), None
    if targets.dtype is torch.int64 and targets.dim() == 1:
        if tuple(targets.shape) != (B,) or targets.device != labels.device:
            raise hip.MrdisError(f'region_scores: a pointer table of ({B},) int64 on {labels.device}, got {tuple(targets.shape)} on {targets.device}')
        return targets.contiguous(), None
    if tuple(targets.shape) != tuple(labels.shape) or targets.dtype not in (torch.uint8, torch.float32) or targets.device != labels.device:
        raise hip.MrdisError(f'region_scores: targets must be a uint8 / fp32 {tuple(labels.shape)} tensor on {labels.device} or a pointer table, '
                             f'got {targets.dtype} {tuple(targets.shape)}')
    vol = targets.to(torch.float32).contiguous()
    step = vol[0].numel() * 4
    return torch.tensor([vol.data_ptr() + b * step for b in range(B)], dtype=torch.int64).to(labels.device), vol


def region_scores(labels, targets, regions=BRATS_REGIONS, spacing=1.0):
    """Scores of predicted label volumes by region.  labels: (B, H, W, D) uint8 on the device (what `predict_volumes` yields); targets: a
    (B, H, W, D) uint8 / fp32 tensor of ground-truth labels, or the (B,) int64 pointer table of `VolumeLoader3D.target_ptrs` (addresses of raw
    (H, W, D) fp32 volumes, 0 = no ground truth for that sample); regions: up to 4 (name, labels) pairs over label values 0 .. 7 (a value
    above 7, or a non-integral ground-truth value, belongs to no region); spacing: the isotropic voxel size, a host-side scale of the distances.

    -> {'dice', 'sensitivity', 'specificity', 'hd95': float64 CPU tensors (B, R); 'counts': int64 CPU (B, R, 5) = [I, P, T, surface voxels
    of P, of T]; 'names': the region names}

    The region definitions (`BRATS_REGIONS`: WT = {1, 2, 4}, TC = {1, 4}, ET = {4}) are the standard ones.  The rules below are THIS PACKAGE'S
    CONVENTION -- the empty-region and percentile rules vary between toolkits.  With P, T the voxels of the predicted and the ground-truth
    region, I their intersection, N = H W D and TN = N - P - T + I:
      dice = 2 I / (P + T);  sensitivity = I / T, or 1 if T = 0;  specificity = TN / (N - T), or 1 if N = T.
      A surface voxel lies in the region and has a face neighbour outside it (the volume border counts as outside).  The directed 95 %
      distance from A to B is spacing * sqrt(k), k the smallest squared distance with 20 * cum[k] >= 19 * n_A, where n_A counts the surface
      voxels of A and cum[k] those within squared distance k of B's surface: the nearest rank, decided in integers, no interpolation.
      hd95 = the larger of the two directed distances.
      Both regions empty: dice 1, hd95 0.  Exactly one empty: dice 0, hd95 = spacing * sqrt(H^2 + W^2 + D^2) (373.13 for BraTS geometry,
      the challenge's penalty).  No ground truth for the sample: NaN in all four.

    One `hip.region_surfaces` launch and three for `hip.surface_hist`, whatever B; the running sums over the histograms are torch ops on the
    device; ONE small D2H copy brings the counts, the percentile ranks and the has-ground-truth bits."""
    names, masks = region_masks(regions)
    B, H, W, D = hip._volume_u8(labels, 'region_scores: labels')
    hip._edt_geometry(B, H, W, D, 'region_scores')
    ptrs, keep = _target_table(targets, labels)
    R = len(masks)
    flags, counts = hip.region_surfaces(labels, ptrs, masks)
    hist = hip.surface_hist(flags, R)
    n = torch.stack([counts[..., 4], counts[..., 3]], dim=-1)        # direction 0 is measured at T's surface voxels, 1 at P's
    ranks = percentile_ranks(hist, n)
    host = torch.cat([counts.to(torch.int64).reshape(-1), ranks.reshape(-1), (ptrs != 0).to(torch.int64)]).cpu().numpy()
    del keep
    c = host[:B * R * 5].reshape(B, R, 5)
    k = host[B * R * 5:B * R * 7].reshape(B, R, 2)
    out = scores_from_counts(c, k, (H, W, D), spacing, has_target=host[B * R * 7:] != 0)
    out['counts'] = torch.from_numpy(c.copy())
    out['names'] = names
    return out
