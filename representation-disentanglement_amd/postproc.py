"""Clean-up of predicted label volumes by 3-D connected components, on the device where `predict_volumes` leaves its labels and
`region_scores` reads them (csrc/mrdis_cc.hip).

    comp, size = mrdis.components3d(labels)                                   # canonical component ids and sizes
    cleaned, stats = mrdis.clean_labels(labels, min_voxels=50, et_min_voxels=200)

Two steps that BraTS pipelines commonly run after prediction: drop small (or all but the largest) connected components of the foreground, and
relabel an enhancing tumour of only a few voxels as necrotic core.  Both are integer arithmetic throughout -- exact, the same bits from run to
run -- in a fixed number of kernel launches (three for the labelling, four for the rules) with no host sync.
"""
import torch

from . import hip

CONNECTIVITIES = hip.CC_CONNECTIVITIES
KEEP_MODES = ('all', 'largest')
STATS_COLUMNS = ('components', 'kept', 'foreground', 'removed', 'et_voxels', 'et_replaced')


def fg_mask(fg):
    """labels -> the bit mask of `hip.cc_label`; ValueError for a label outside 1 .. 7 or an empty set"""
    try:
        labels = [int(l) for l in fg]
    except TypeError:
        raise ValueError(f'fg: a sequence of labels in 1 .. 7, got {fg!r}') from None
    if not labels or any(not 0 <= l <= 7 for l in labels):
        raise ValueError(f'fg: labels in 1 .. 7, got {labels}')
    if 0 in labels:
        raise ValueError(f'fg: label 0 is the background and cannot be foreground, got {labels}')
    return sum(1 << l for l in set(labels))


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f'connectivity {connectivity!r}: one of {CONNECTIVITIES}')
    return int(connectivity)


def _volume(labels, what):
    """(a contiguous uint8 (B, H, W, D) view or copy, whether the input was 3-D), as `edt3d_sq` takes its mask"""
    if not torch.is_tensor(labels) or labels.dim() not in (3, 4) or labels.dtype not in (torch.bool, torch.uint8):
        got = f'{labels.dtype} {tuple(labels.shape)}' if torch.is_tensor(labels) else type(labels).__name__
        raise hip.MrdisError(f'{what}: a (B, H, W, D) or (H, W, D) bool / uint8 tensor, got {got}')
    v = labels if labels.dim() == 4 else labels[None]
    hip._cc_geometry(*v.shape, what)
    if not v.is_cuda:
        raise hip.MrdisError(f'{what}: the volume must live on the GPU, got a tensor on {v.device}')
    v = v.contiguous()
    return (v.view(torch.uint8) if v.dtype is torch.bool else v), labels.dim() == 3


def components3d(labels, fg=(1, 2, 4), connectivity=26):
    """Connected components of the foreground of label volumes -> (comp, size), int32 tensors of the shape of `labels` on its device.

    labels: a (B, H, W, D) or (H, W, D) uint8 device tensor (what `predict_volumes` yields), or a bool / uint8 mask with fg=(1,); B in
    1 .. 65535, each of H, W, D in 1 .. 1024 (else MrdisError('... unsupported geometry ...'), before any launch).  A voxel is foreground iff
    its label is one of `fg` (labels in 1 .. 7); every other value, those above 7 included, is background and joins nothing.  connectivity:
    6 (faces), 18 (faces and edges) or 26 (faces, edges and corners).  Components never cross a sample or wrap around a border.

    comp: -1 on background; on foreground the smallest in-sample flat index (h W + w) D + d of the voxel's component -- a canonical id that
    does not depend on scheduling.  size: the component's voxel count at its root voxel (where comp equals the voxel's own index), 0 elsewhere.
    Three kernel launches whatever B, shape and content (hip.cc_label; counter 'cclabel'), no host sync."""
    mask = fg_mask(fg)
    connectivity = _check_connectivity(connectivity)
    v, squeeze = _volume(labels, 'components3d')
    comp, size = hip.cc_label(v, mask, connectivity)
    return (comp[0], size[0]) if squeeze else (comp, size)


def clean_labels(labels, fg=(1, 2, 4), connectivity=26, min_voxels=0, keep='all', et_label=4, et_min_voxels=0, et_replace=1):
    """Clean label volumes by connected components -> (cleaned, stats): cleaned uint8 of the shape of `labels`, stats (B, 6) int32, both on
    the device.  labels, fg, connectivity: as `components3d`.

    Removing small or non-largest components and relabelling a tiny enhancing tumour are common BraTS post-processing steps; the exact rules
    below are THIS PACKAGE'S CONVENTION (thresholds, tie-breaks and the order of the steps vary between pipelines):
      1. The components of the foreground are found under `connectivity`, per sample.
      2. keep='all': a component is kept iff its size is at least `min_voxels`.  keep='largest': only the largest component of the sample is
         a candidate -- a size tie goes to the smaller root index -- and it is kept iff its size is at least `min_voxels`.  Voxels of
         components that are not kept become 0; background voxels pass through unchanged.
      3. With n the voxels of the sample whose label after step 2 equals `et_label`: if et_min_voxels > 0 and 0 < n < et_min_voxels, those
         voxels become `et_replace`.
    stats columns (`STATS_COLUMNS`): components found, components kept, foreground voxels, voxels removed, n of step 3, replaced (0 | 1).
    With the defaults (min_voxels=0, keep='all', et_min_voxels=0) the output equals the input byte for byte.

    ValueError, before any launch: a label outside 0 .. 7 in fg, et_label or et_replace; 0 in fg; connectivity not in {6, 18, 26}; keep not
    in {'all', 'largest'}; a negative threshold.  Three launches for the labelling and four for the rules (hip.cc_label, hip.cc_clean; counters
    'cclabel', 'ccclean'), no host sync."""
    mask = fg_mask(fg)
    connectivity = _check_connectivity(connectivity)
    if keep not in KEEP_MODES:
        raise ValueError(f'keep {keep!r}: one of {KEEP_MODES}')
    for name, val in (('et_label', et_label), ('et_replace', et_replace)):
        if isinstance(val, bool) or int(val) != val or not 0 <= int(val) <= 7:
            raise ValueError(f'{name} {val!r}: a label in 0 .. 7')
    for name, val in (('min_voxels', min_voxels), ('et_min_voxels', et_min_voxels)):
        if isinstance(val, bool) or int(val) != val or int(val) < 0:
            raise ValueError(f'{name} {val!r}: an integer >= 0')
    v, squeeze = _volume(labels, 'clean_labels')
    comp, size = hip.cc_label(v, mask, connectivity)
    out, stats = hip.cc_clean(v, comp, size, int(min_voxels), keep == 'largest', int(et_label), int(et_min_voxels), int(et_replace))
    return (out[0] if squeeze else out), stats


def stats_csv_header():
    return 'subj_id,components,kept,foreground,removed,et_voxels,et_replaced'


def write_stats_csv(path, subj, stats):
    """postprocess.csv: `subj_id,components,kept,foreground,removed,et_voxels,et_replaced`, one row per subject; stats: (n, 6) integers (a
    tensor, an array or nested lists), the rows of `clean_labels`' stats in the order of `subj`."""
    rows = stats.tolist() if hasattr(stats, 'tolist') else [list(r) for r in stats]
    if len(rows) != len(subj) or any(len(r) != len(STATS_COLUMNS) for r in rows):
        raise ValueError(f'write_stats_csv: {len(subj)} subjects need {len(subj)} rows of {len(STATS_COLUMNS)} integers')
    with open(path, 'w') as f:
        f.write(stats_csv_header() + '\n')
        for sid, r in zip(subj, rows):
            f.write(str(sid) + ',' + ','.join(str(int(x)) for x in r) + '\n')
