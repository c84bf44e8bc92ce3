"""Whole-subject synthesis of missing contrasts by the 2-D model: the subject-wise driver over the HBM-resident `VolumeStore`.

The model's purpose is the contrast a subject lacks, produced from the anatomy of the contrasts it has.  `synthesize_volumes` walks every
centre slice of a subject in order, encodes the batch (eval mode, no_grad, modality code = the encoder's mu), gives every target contrast a
modality code -- its own if the contrast is there, else the nearest gallery row's (`ZGallery.nearest`) or the gallery mean -- decodes it from
every present source's anatomy (`reconstruct_input_si_zj`), and assembles the decoded slice blocks into a volume with two HIP kernels
(csrc/mrdis_synth.hip: `hip.synth_accum` per batch and target, `hip.synth_finish` per target).  A target whose real volume is in the store
(a contrast hidden on purpose with `drop`, or simply present) is scored plane by plane with `hip.recon_metrics`.

The rules (present set, batches, source of the search, block assembly, fill, scoring) are THIS PACKAGE'S OWN CONVENTION: the reference's result
dump (main_missing.py:545-607, util.py:257-309) writes per-slice arrays into an h5 file and assembles no volume.
"""
import torch

from . import hip, ops
from .model import flush_batch_counters
from .trainer import EVAL_INFOS, _encode_batch, nn_source_contrast

SYNTH_BLOCKS = ('centre', 'mean')
ZSCORE_NAMES = ('z-score', 'zscore')            # norm_type values whose volumes carry the z-scored files' background of -10


def synth_plan(D, block_size, batch_size):
    """[(s0, B)]: every centre slice s in [b, D - 1 - b] ascending, cut into batches of `batch_size` consecutive centres (the last may be short)."""
    D, b, n = int(D), int(block_size), int(batch_size)
    if b < 0 or n < 1:
        raise ValueError(f'synth_plan: block_size {b} >= 0 and batch_size {n} >= 1 wanted')
    if D < 2 * b + 1:
        raise ValueError(f'synth_plan: a volume of {D} slices holds no block of {2 * b + 1}')
    last = D - 1 - b
    return [(s0, min(n, last - s0 + 1)) for s0 in range(b, last + 1, n)]


def synth_source(i, present):
    """contrast whose compact anatomy code searches the modality code of the absent target i: nn_source_contrast(i) (the reference's rule) if
    that contrast is present, else the lowest-index present contrast."""
    present = [bool(p) for p in present]
    if not any(present):
        raise ValueError('synth_source: no contrast is present')
    j = nn_source_contrast(i)
    if 0 <= j < len(present) and present[j]:
        return j
    return present.index(True)


def synth_targets(present, info=''):
    """indices synthesised for a subject with the given present flags: a present contrast always (decoded with its own code), an absent one only
    with a searched or mean code (`info`); either needs a present source other than itself."""
    if info not in EVAL_INFOS:
        raise ValueError(f'synth_targets: info {info!r}: one of {EVAL_INFOS}')
    present = [bool(p) for p in present]
    return [i for i, p in enumerate(present) if (p or info) and any(q for j, q in enumerate(present) if j != i)]


def check_synth_options(contrast_list, info='', drop=(), block='centre'):
    """-> the indices of `drop`; ValueError for an unknown info, block or contrast name"""
    if info not in EVAL_INFOS:
        raise ValueError(f'synth info {info!r}: one of {EVAL_INFOS}')
    if block not in SYNTH_BLOCKS:
        raise ValueError(f'synth block {block!r}: one of {SYNTH_BLOCKS}')
    names = [str(c) for c in contrast_list]
    if isinstance(drop, str):
        drop = [drop] if drop else []
    bad = [d for d in (drop or ()) if str(d) not in names]
    if bad:
        raise ValueError(f'synth drop {bad}: not in contrast_list {names}')
    return sorted({names.index(str(d)) for d in (drop or ())})


def default_fill(config):
    """the store's background: -10 in the z-scored files, 0 otherwise"""
    return -10.0 if str(config.get('norm_type', '')) in ZSCORE_NAMES else 0.0


def covered_planes(D, block_size, block):
    """(first, last) plane a whole subject's pass writes: every plane for 'mean', the centres for 'centre'"""
    return (0, D - 1) if block == 'mean' else (block_size, D - 1 - block_size)


def _dense_nhwc(x):
    x = x.float()
    return x if x.permute(0, 2, 3, 1).is_contiguous() else x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@torch.no_grad()
def synthesize_volumes(model, config, store, subjects, info='', gallery=None, drop=(), block='centre', batch_size=None, fill=None):
    """generator over `subjects` (subj_id strings of `store`): one dict per subject with
      subj_id; present (M bools: in the store and not in `drop`); dropped (M bools); targets (indices synthesised); skipped (the others);
      volumes {contrast name: (H, W, D) fp32 device tensor, the store's own geometry}; n_sources {name: sources averaged};
      metrics {name: (mse, psnr, ssim) against the stored volume, averaged over the covered planes; NaN where the store has none};
      nn_rows {name: (centres,) gallery rows whose code decoded the absent target, in slice order} (info 'nearest_neighbour' only).
    info '' | 'nearest_neighbour' | 'mean' chooses the modality code of an absent target (the last two need `gallery`, a ZGallery); drop: contrast
    names hidden on purpose; block 'centre' | 'mean'; batch_size: centres per batch (None: config['batch_size']); fill: value of planes nothing
    predicts (None: the store's background).  The model is put in eval mode and its training flag restored.  Single process only."""
    names = [str(c) for c in config['contrast_list']]
    M, b = len(names), int(config['block_size'])
    drop_idx = check_synth_options(names, info, drop, block)
    if info and gallery is None:
        raise ValueError(f'synthesize_volumes info={info!r} needs a ZGallery (build_z_gallery)')
    if info == 'nearest_neighbour':
        gallery.check_compact_method(model)
    if M - 1 > hip.SYNTH_MAX_SRC:
        raise ValueError(f'synthesize_volumes: at most {hip.SYNTH_MAX_SRC + 1} contrasts')
    H, W, D = store.shape
    dev = store.device
    plan = synth_plan(D, b, config['batch_size'] if batch_size is None else batch_size)
    fill = default_fill(config) if fill is None else float(fill)
    c_lo, c_hi = (0, 2 * b) if block == 'mean' else (b, b)
    k_lo, k_hi = covered_planes(D, b, block)
    nan3 = (float('nan'),) * 3

    def one(sid):
        ptrs = [store.ptr(f'{sid}/{c}') for c in names]
        present = [bool(p) and i not in drop_idx for i, p in enumerate(ptrs)]
        if not any(present):
            raise ValueError(f'synthesize_volumes: subject {sid!r} has no present contrast (store {[bool(p) for p in ptrs]}, drop {list(drop)})')
        targets = synth_targets(present, info)
        sources = {i: [j for j in range(M) if present[j] and j != i] for i in targets}
        acc = {i: torch.zeros((D, H, W), dtype=torch.float32, device=dev) for i in targets}
        cnt = {i: torch.zeros((D,), dtype=torch.int32, device=dev) for i in targets}
        codes = gallery.codes([sid]) if info else None
        nn_rows = {}
        row = torch.tensor([p if present[i] else 0 for i, p in enumerate(ptrs)], dtype=torch.int64)
        for s0, B in (plan if targets else ()):                               # nothing to synthesise: no pass at all
            centres = list(range(s0, s0 + B))
            vol_ptrs = row.repeat(B, 1).to(dev)
            slice_idx = torch.arange(s0, s0 + B, dtype=torch.int32).to(dev)
            none = torch.full((B,), -1, dtype=torch.int32).to(dev)
            inputs, _, mask_img = hip.slice_gather(vol_ptrs, slice_idx, none, H, W, D, b)      # absent and dropped: zeros, mask 0
            si_list, mu_list = _encode_batch(model, config, inputs, mask_img)
            z_dec = list(mu_list)
            found = {}
            for i in targets:
                if present[i]:
                    continue
                if info == 'mean':
                    z_dec[i] = gallery.mean_z(codes * B, i).to(device=dev, dtype=mu_list[i].dtype)
                else:
                    src = synth_source(i, present)
                    if src not in found:
                        found[src] = gallery.nearest(model.compute_compact_s(si_list[src]), codes * B, src).long()
                    z_dec[i] = gallery.z[found[src], i].to(mu_list[i].dtype)
                    nn_rows.setdefault(names[i], []).append(found[src])
            mix = model.reconstruct_input_si_zj(si_list, z_dec)                  # entries (source j, target i), j-major, i != j
            for i in targets:
                recons = [_dense_nhwc(mix[j * (M - 1) + (i if i < j else i - 1)]) for j in sources[i]]
                hip.synth_accum(recons, centres, acc[i], cnt[i], c_lo, c_hi)
        volumes, metrics, rows = {}, {}, []
        for i in targets:
            vol, out = hip.synth_finish(acc[i], cnt[i], fill)
            volumes[names[i]] = out
            if ptrs[i]:
                truth = store.vols[f'{sid}/{names[i]}']
                m = hip.recon_metrics(truth[k_lo:k_hi + 1].unsqueeze(1), vol[k_lo:k_hi + 1].unsqueeze(1))
                rows.append(m.double().mean(0))
        scored = [i for i in targets if ptrs[i]]
        host = torch.stack(rows).cpu().tolist() if rows else []                  # one D2H copy per subject
        for i in targets:
            metrics[names[i]] = tuple(host[scored.index(i)]) if i in scored else nan3
        return {'subj_id': sid, 'present': present, 'dropped': [i in drop_idx and bool(ptrs[i]) for i in range(M)], 'targets': targets,
                'skipped': [i for i in range(M) if i not in targets], 'volumes': volumes,
                'n_sources': {names[i]: len(sources[i]) for i in targets}, 'metrics': metrics,
                'nn_rows': {n: torch.cat(v) for n, v in nn_rows.items()}}

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
