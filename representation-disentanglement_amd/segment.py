"""Whole-subject tumour segmentation by the 2-D model, per missing-contrast pattern: the subject-wise driver over the HBM-resident `VolumeStore`.

The model's downstream claim is that a task network fed the anatomy maps fused over whichever contrasts a subject HAS keeps segmenting when
contrasts are missing.  `segment_volumes` walks every centre slice of a subject in order (eval mode, no_grad), encodes the anatomy of the batch,
and for every pattern -- a set of contrast names hidden on purpose -- fuses the maps of the contrasts that are left (`ops.fuse_present`), runs the
output decoder and turns the logits of all patterns into label planes with ONE launch per batch (`hip.seg2d_label_planes`); one more launch per
subject (`hip.seg2d_finish`) brings the planes to label volumes in the store's own (H, W, D) geometry and BraTS labels (0 / 1 / 2 / 4).  They are
scored by `surfdist.region_scores` (WT / TC / ET Dice, sensitivity, specificity, HD95) against the subject's `/seg` volume and optionally cleaned
by `postproc.clean_labels`.

The rules (present set, batches, inputs of a hidden contrast, flip views, label per voxel, uncovered planes, scoring) are THIS PACKAGE'S OWN
CONVENTION: the reference scores y_fused per shuffled slice (main_missing.py:529-531), assembles no volume and never fuses for M > 1
(model.py:3230-3258).
  1. present = (contrasts the subject has in the store) minus the pattern's hidden names.  A pattern that leaves a subject nothing gets no volume
     and no launch (the caller writes its row with n_present 0 and NaN scores).
  2. The plan is `synth_plan(D, block_size, batch_size)`: every centre slice in [b, D - 1 - b] ascending, in batches of consecutive centres.  No
     random stream is touched.
  3. Inputs come from `hip.slice_gather` with pointer 0 for hidden and absent contrasts: zeros and mask column 0, exactly what a subject lacking
     them presents (and what `eval_drop` does).  mask_img stays the gather's (inputs[:, 0] == 0): it depends on whether contrast 0 is visible and
     on nothing else of the pattern.  Only the anatomy encoder runs.  In eval mode the map of contrast k depends on its own channels and mask_img
     alone, and the fusion ignores maps whose mask column is 0, so all patterns share at most two encoder passes per batch: contrast 0 visible,
     and contrast 0 hidden (tests/test_gpu_seg2d.py holds the logits of both routes bit-identical).
  4. y = output_decoder(fuse_present(si_list, mask_p, fuse_method))[0], (B, C, H, W), C = out_num_ch.
  5. flip '' uses one view; 'h' / 'w' adds a second: the gathered inputs and mask_img flipped along that axis through the same pipeline, un-flipped
     by the label kernel.
  6. One view: argmax_c y_c over the logits, the lowest c on a tie.  Two views: argmax_c of 0.5 (softmax(y^0)_c + softmax(y^1)_c) in fp32, the
     lowest c on a tie.  Class c is written as label c, class 3 as label 4.
  7. The first and last block_size planes are predicted by nothing: they hold 0 and are scored as such.
  8. Cleaning (optional): clean_labels(labels, connectivity=26, min_voxels, keep, et_min_voxels) on the (H, W, D) volumes.
  9. Scores: region_scores(labels, targets) with BRATS_REGIONS; the target is the subject's `/seg` volume as stored (no 4 -> 3 relabel).  A
     subject without `/seg` gets None.
"""
import itertools

import torch

from . import hip, ops
from .model import flush_batch_counters
from .postproc import KEEP_MODES, clean_labels
from .surfdist import BRATS_REGIONS, region_scores
from .lesion import MAX_DILATION, lesion_csv_header, lesion_csv_values, lesion_scores
from .synth import synth_plan
from .trainer import split_inputs

SEG_FLIPS = ('', 'h', 'w')
SEG_PATTERN_SPECS = ('full', 'leave_one_out', 'all')
# csv column prefix, region_scores key: the column order of the 3-D entry's predict_regions.csv (train3d.region_csv_header)
REGION_CSV_KEYS = (('dice', 'dice'), ('sens', 'sensitivity'), ('spec', 'specificity'), ('hd95', 'hd95'))
REGION_COLUMNS = tuple(f'{col}_{name}' for col, _ in REGION_CSV_KEYS for name, _ in BRATS_REGIONS)


def pattern_name(hidden):
    """'full' for nothing hidden, else 'no_' + the hidden names joined by '_'"""
    return 'no_' + '_'.join(hidden) if hidden else 'full'


def seg_patterns(contrast_list, spec):
    """[(name, [hidden contrast names])] of a pattern spec: 'full' (one pattern, nothing hidden) | 'leave_one_out' (full plus each single contrast
    hidden) | 'all' (every proper subset hidden, i.e. every non-empty present set: 2^M - 1 patterns ordered by the number hidden, then
    lexicographically by index) | an explicit list of lists of names.  Names are 'full', 'no_T1c', 'no_T1_T2', ... (hidden names in contrast
    order).  ValueError for an unknown name, a pattern hiding every contrast, or duplicates.  This package's own convention: the reference has
    no such table."""
    names = [str(c) for c in contrast_list]
    M = len(names)
    if isinstance(spec, str):
        if spec not in SEG_PATTERN_SPECS:
            raise ValueError(f'seg_patterns {spec!r}: one of {SEG_PATTERN_SPECS} or a list of lists of contrast names')
        sizes = {'full': (0,), 'leave_one_out': (0, 1) if M > 1 else (0,), 'all': range(M)}[spec]
        sets = [c for n in sizes for c in itertools.combinations(range(M), n)]
    else:
        if not isinstance(spec, (list, tuple)) or not spec:
            raise ValueError(f'seg_patterns {spec!r}: one of {SEG_PATTERN_SPECS} or a non-empty list of lists of contrast names')
        sets = []
        for item in spec:
            item = [item] if isinstance(item, str) else list(item)
            bad = [str(x) for x in item if str(x) not in names]
            if bad:
                raise ValueError(f'seg_patterns: {bad} not in contrast_list {names}')
            idx = [names.index(str(x)) for x in item]
            if len(set(idx)) != len(idx):
                raise ValueError(f'seg_patterns: pattern {item} names a contrast twice')
            sets.append(tuple(sorted(idx)))
        if len(set(sets)) != len(sets):
            raise ValueError(f'seg_patterns: duplicate patterns in {spec}')
    out = []
    for s in sets:
        if len(s) == M:
            raise ValueError(f'seg_patterns: a pattern hides every contrast of {names}')
        hidden = [names[i] for i in s]
        out.append((pattern_name(hidden), hidden))
    return out


def _as_patterns(contrast_list, patterns):
    """a spec, or the pairs `seg_patterns` returns (validated again)"""
    if not isinstance(patterns, str) and patterns and all(isinstance(p, tuple) and len(p) == 2 and isinstance(p[1], (list, tuple)) for p in patterns):
        got = seg_patterns(contrast_list, [list(p[1]) for p in patterns])
        if [n for n, _ in got] != [str(p[0]) for p in patterns]:
            raise ValueError(f'segment_volumes: pattern names {[p[0] for p in patterns]} are not those of seg_patterns {[n for n, _ in got]}')
        return got
    return seg_patterns(contrast_list, patterns)


def check_seg_options(contrast_list, patterns='full', flip='', post=None):
    """-> (patterns as pairs, post as None or {'min_voxels', 'keep', 'et_min_voxels'}); ValueError for a bad pattern spec, flip or cleaning option"""
    pats = _as_patterns(contrast_list, patterns)
    if flip not in SEG_FLIPS:
        raise ValueError(f'seg_flip {flip!r}: one of {SEG_FLIPS}')
    if post is not None:
        post = {'min_voxels': post.get('min_voxels', 0), 'keep': post.get('keep', 'all'), 'et_min_voxels': post.get('et_min_voxels', 0)}
        if post['keep'] not in KEEP_MODES:
            raise ValueError(f'seg_post_keep {post["keep"]!r}: one of {KEEP_MODES}')
        for k in ('min_voxels', 'et_min_voxels'):
            if isinstance(post[k], bool) or not isinstance(post[k], int) or post[k] < 0:
                raise ValueError(f'seg_post_{k} {post[k]!r}: an integer >= 0')
    return pats, post


LESION_COLUMNS = tuple(lesion_csv_header().split(','))        # the value columns of seg_lesions.csv and seg_lesion_patterns.csv


def check_lesion_options(lesions):
    """None, or {'dilation', 'min_voxels'} for `lesion_scores` (defaults 3 and 50); ValueError for a value it would refuse"""
    if lesions is None:
        return None
    lesions = {'dilation': lesions.get('dilation', 3), 'min_voxels': lesions.get('min_voxels', 50)}
    for k, hi in (('dilation', MAX_DILATION), ('min_voxels', None)):
        v = lesions[k]
        if isinstance(v, bool) or not isinstance(v, int) or v < 0 or (hi is not None and v > hi):
            raise ValueError(f'seg_lesion_{k} {v!r}: an integer ' + (f'in 0 .. {hi}' if hi is not None else '>= 0'))
    return lesions


def _dense_nhwc(x):
    x = x.float()
    return x if x.permute(0, 2, 3, 1).is_contiguous() else x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def encode_anatomy(model, config, inputs, mask_img):
    """the anatomy encoder alone, in eval mode: si_list of one gathered batch"""
    M = len(config['contrast_list'])
    inputs_list = split_inputs(inputs, M, 2 * config['block_size'] + 1)
    if hasattr(model, 'premix'):
        model.premix('enc')
    else:
        ops.premix_all(model, model._type_table)
    return model.compute_anatomy_encoding(inputs_list, mask_img)


@torch.no_grad()
def pattern_logits(model, config, shape, device, ptrs, presents, s0, B, flip='', share_encoder=True):
    """the output decoder's logits of the B consecutive centres s0, s0 + 1, ... of one subject for every pattern: [[view tensors] per pattern], each
    a dense channels-last fp32 (B, C, H, W) tensor; one view, or two with a flip (the second from the flipped inputs, NOT un-flipped).  ptrs: the
    subject's M volume pointers (0: absent); presents: per pattern M bools, at least one True each.  share_encoder: one encoder pass per value of
    "contrast 0 visible" the patterns take -- a hidden contrast k > 0 keeps its real channels there: its map is computed and then ignored by the
    fusion (mask column 0) --; False: one pass per pattern with every hidden pointer zeroed (rule 3 of the module docstring).  The caller holds
    eval mode and the mix cache."""
    H, W, D = shape
    b = int(config['block_size'])
    flip_dim = {'h': 2, 'w': 3}.get(flip)
    slice_idx = torch.arange(s0, s0 + B, dtype=torch.int32).to(device)
    none = torch.full((B,), -1, dtype=torch.int32).to(device)
    encoded = {}

    def maps(row):
        """[si_list per view] of the batch gathered with the pointer row `row` (a tuple)"""
        if row not in encoded:
            inputs, _, mask_img = hip.slice_gather(torch.tensor(row, dtype=torch.int64).repeat(B, 1).to(device), slice_idx, none, H, W, D, b)
            encoded[row] = [encode_anatomy(model, config, inputs, mask_img)]
            if flip:
                encoded[row].append(encode_anatomy(model, config, inputs.flip(flip_dim).contiguous(memory_format=torch.channels_last),
                                                   mask_img.flip(flip_dim - 1).contiguous()))
        return encoded[row]
    out = []
    for pr in presents:
        if share_encoder:
            row = tuple(p if (i > 0 or pr[0]) else 0 for i, p in enumerate(ptrs))
        else:
            row = tuple(p if pr[i] else 0 for i, p in enumerate(ptrs))
        mh = torch.tensor([[1.0 if p else 0.0 for p in pr]], dtype=torch.float32).repeat(B, 1)
        mask_p = mh.to(device)
        out.append([_dense_nhwc(model.output_decoder(ops.fuse_present(si, mask_p, mh, model.fuse_method))[0]) for si in maps(row)])
    return out


@torch.no_grad()
def segment_volumes(model, config, store, subjects, patterns='full', flip='', batch_size=None, post=None, share_encoder=True, lesions=None):
    """generator over `subjects` (subj_id strings of `store`): one dict per subject with
      subj_id; patterns (the pattern names); present (per pattern, M bools: in the store and not hidden);
      labels ((P', H, W, D) uint8 device tensor over the patterns that leave a present contrast, in pattern order; None if there is none);
      scores (the `region_scores` dict of `labels` against the stored `/seg` volume, or None without one);
      post, post_scores, post_stats (the cleaned labels, their scores and the (P', 6) stats of `clean_labels`): only when cleaning is on;
      lesions, post_lesions (the `lesion_scores` dicts of `labels` and of `post`, or None without ground truth): only with `lesions`;
      launches (the deltas of hip.SEG2D_FAMILIES over the subject).
    patterns: a spec of `seg_patterns` or its result; flip '' | 'h' | 'w': a second, flipped view averaged in probability; batch_size: centres
    per batch (None: config['batch_size']); post: None, or {'min_voxels', 'keep', 'et_min_voxels'} for `clean_labels` (connectivity 26).
    lesions: None, or {'dilation', 'min_voxels'} for `lesion_scores` (no lesion kernel launches without it).
    share_encoder=False encodes per pattern instead of sharing the encoder passes (rule 3; the same bits, more work).
    More than hip.SEG2D_MAX_SETS patterns go through the label kernel in chunks of 16.  Needs a built output decoder and dataset_name 'BraTS'
    (ValueError naming lambda_recon_y_fused otherwise).  The rules are this package's own convention (module docstring): the reference
    assembles no volume and never fuses for M > 1.  The model is put in eval mode and its training flag restored.  Single process only."""
    names = [str(c) for c in config['contrast_list']]
    b = int(config['block_size'])
    pats, post = check_seg_options(names, patterns, flip, post)
    lesions = check_lesion_options(lesions)
    if getattr(model, 'output_decoder', None) is None or config.get('dataset_name') != 'BraTS':
        raise ValueError("segment_volumes needs the output decoder of a BraTS model: train with lambda_recon_y_fused > 0 (compute_dtype 'f32' or "
                         f"'bf16m') and dataset_name 'BraTS' (got dataset_name {config.get('dataset_name')!r}, output decoder "
                         f"{'built' if getattr(model, 'output_decoder', None) is not None else 'not built'})")
    H, W, D = store.shape
    dev = store.device
    plan = synth_plan(D, b, config['batch_size'] if batch_size is None else batch_size)
    flips = [0] + ([hip.SEG2D_FLIPS[flip]] if flip else [])
    hidden_idx = [[names.index(h) for h in hid] for _, hid in pats]

    def one(sid):
        before = hip.launch_counts()
        ptrs = [store.ptr(f'{sid}/{c}') for c in names]
        present = [[bool(p) and i not in hid for i, p in enumerate(ptrs)] for hid in hidden_idx]
        live = [k for k, pr in enumerate(present) if any(pr)]
        res = {'subj_id': sid, 'patterns': [n for n, _ in pats], 'present': present, 'labels': None, 'scores': None}
        if post is not None:
            res.update(post=None, post_scores=None, post_stats=None)
        if lesions is not None:
            res.update(lesions=None, **({'post_lesions': None} if post is not None else {}))
        if live:
            planes = torch.zeros((len(live), D, H, W), dtype=torch.uint8, device=dev)          # planes nothing predicts stay 0
            for s0, B in plan:
                views = pattern_logits(model, config, (H, W, D), dev, ptrs, [present[k] for k in live], s0, B, flip, share_encoder)
                for c0 in range(0, len(live), hip.SEG2D_MAX_SETS):
                    hip.seg2d_label_planes(views[c0:c0 + hip.SEG2D_MAX_SETS], flips, planes[c0:c0 + hip.SEG2D_MAX_SETS], s0, relabel=True)
            labels = hip.seg2d_finish(planes)
            res['labels'] = labels
            seg = store.vols.get(f'{sid}/seg')
            table = None
            if seg is not None:
                target = seg.permute(1, 2, 0).contiguous().float()           # the stored labels in (H, W, D), once per subject
                table = torch.full((len(live),), target.data_ptr(), dtype=torch.int64).to(dev)
                res['scores'] = region_scores(labels, table, BRATS_REGIONS)
                if lesions is not None:
                    res['lesions'] = lesion_scores(labels, table, BRATS_REGIONS, dilation=lesions['dilation'], min_voxels=lesions['min_voxels'])
            if post is not None:
                res['post'], res['post_stats'] = clean_labels(labels, connectivity=26, min_voxels=post['min_voxels'], keep=post['keep'],
                                                              et_min_voxels=post['et_min_voxels'])
                if table is not None:
                    res['post_scores'] = region_scores(res['post'], table, BRATS_REGIONS)
                    if lesions is not None:
                        res['post_lesions'] = lesion_scores(res['post'], table, BRATS_REGIONS, dilation=lesions['dilation'],
                                                            min_voxels=lesions['min_voxels'])
        after = hip.launch_counts()
        res['launches'] = {f: after[f] - before[f] for f in hip.SEG2D_FAMILIES}
        return res

    for sid in subjects:
        was = model.training                     # per subject: nothing is held across a yield, so an abandoned generator leaves no state behind
        flush_batch_counters()
        model.eval()
        try:
            with ops.mix_cache():
                res = one(str(sid))
        finally:
            model.train(was)
        yield res


def lesion_rows(res, key='lesions'):
    """[(pattern name, n_present, [the LESION_COLUMNS values as written: floats with repr, counts as integers, 'nan' where there is nothing to
    score])] of one subject's result, one per pattern"""
    live = [k for k, pr in enumerate(res['present']) if any(pr)]
    sc = res.get(key)
    rows = []
    for k, name in enumerate(res['patterns']):
        vals = ['nan'] * len(LESION_COLUMNS)
        if sc is not None and k in live:
            vals = lesion_csv_values(sc, live.index(k))
        rows.append((name, sum(res['present'][k]), vals))
    return rows


def score_rows(res, key='scores'):
    """[(pattern name, n_present, [the REGION_COLUMNS values, NaN where there is nothing to score])] of one subject's result, one per pattern"""
    nan = [float('nan')] * len(REGION_COLUMNS)
    live = [k for k, pr in enumerate(res['present']) if any(pr)]
    sc = res.get(key)
    rows = []
    for k, name in enumerate(res['patterns']):
        vals = nan
        if sc is not None and k in live:
            j = live.index(k)
            vals = [float(sc[skey][j, r]) for _, skey in REGION_CSV_KEYS for r in range(len(BRATS_REGIONS))]
        rows.append((name, sum(res['present'][k]), vals))
    return rows
