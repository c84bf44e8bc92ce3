"""Training and validation entry of the 3-D nets (`NVNet3D` / `UNet3D`), in the style of `train.Run`:

    python main_3d.py [config3d.yaml] [key=value ...]

The reference ships the 3-D networks and their dataset but no loop, objective or metric call for them; what is restated
here is the package's own: the objective is `nvnet_loss` (Myronenko 2018) -- through the fused HIP kernels (`nvnet_loss_hip`,
csrc/mrdis_loss3d.hip) unless `fused_loss: false` -- the optimizer is `ArenaAdam` with the fused clip, the validation metric is the reference's
Dice / IoU (`compute_segmentation_metrics`, util.py:946-992) from the integer counts of `mrdis_seg_counts`, and stat.csv / `epochNNN.pth.tar` /
`model_best.pth.tar` are written by the same `save_result_stat` / `save_checkpoint` as the 2-D entry.  The best checkpoint is the epoch with the
highest validation Dice.  `phase: predict` loads it and writes one label volume per subject over the FULL depth (sliding window,
model3d.predict_volumes) with its Dice / IoU; with `predict_regions: true` also the BraTS region scores (Dice, sensitivity, specificity, HD95
of WT / TC / ET: surfdist.region_scores) in predict_regions.csv.  `phase: score` writes that file for label volumes that already lie under
result_<predict_set>/ -- predicted earlier or post-processed elsewhere -- without building or loading a model.  `predict_post: true` also
writes, during `phase: predict`, the label volumes cleaned by connected components (postproc.clean_labels: small or non-largest components
removed, a tiny enhancing tumour relabelled) under result_<predict_set>/post/; `phase: postprocess` makes the same files from label volumes
that are already written, again without a model, and `score_subdir: post` lets `phase: score` read and write there.

A checkpoint also carries the host and device RNG states (np.random, torch default, the torch device generator, the loaders' own generator
if any), written after the epoch's validation pass: `continue_train` then continues exactly where the run stopped -- the shuffles, augmentation
draws, dropout masks and VAE noise of epoch k + 1 are those of an uninterrupted run.

World size 1 only: under an initialised process group the constructor raises NotImplementedError.
"""
import glob
import os
import re
import sys

import numpy as np
import torch
import torch.distributed as dist
import yaml

from . import hip
from .data3d import INTENSITY_DEFAULTS, VolumeData3D, VolumeStore3D, patch_args, patch_intensity_args, patch_warp_args
from .prep import build_store_from_raw, ensure_fold_lists, save_nifti
from .postproc import CONNECTIVITIES, KEEP_MODES, STATS_COLUMNS, clean_labels, write_stats_csv
from .model3d import NVNet3D, UNet3D, nvnet_loss, nvnet_loss_hip, predict_volumes, seg_metrics_from_counts
from .model3d import TILE_WEIGHTS, predict_tiles, tile_offsets, tile_views, tile_weights
from .surfdist import BRATS_REGIONS, SCORE_KEYS, region_scores
from .lesion import MAX_DILATION, lesion_csv_header, lesion_csv_values, lesion_scores
from .train import parse_overrides, save_config_file, save_result_stat
from .trainer import ArenaAdam, load_checkpoint_model, save_checkpoint

DEFAULT_CONFIG_3D = {
    'phase': 'train',                  # train | test (load model_best.pth.tar, print the test-set stat) | predict (load it, write whole-volume label maps)
                                       # | score (region scores of the label maps already under result_<predict_set>/: no model)
                                       # | postprocess (clean the label maps already under result_<predict_set>/ into post/: no model)
    'dataset_name': 'BraTS', 'data_path': '../data/', 'norm_type': 'z-score', 'fold': 0,
    'data_source': 'h5',               # h5: the reference's file under data_path | raw: the NIfTI files of a BraTS download under raw_path (prep.py)
    'raw_path': '',                    # data_source raw: the directory of the subjects; fold lists that data_path lacks are written first
    'raw_crop': [[40, 40], [24, 24]],  # data_source raw: voxels removed at the low and high end of H and of W
    'contrast_list': ['T1', 'T1c', 'T2', 'T2_FLAIR'], 'batch_size': 4,
    'model_name': 'NVNet3D',           # NVNet3D | UNet3D (Dice-only objective)
    'init_channels': 16, 'p': 0.2,
    'aug': True, 'dropoff': True,
    'patch_size': None,                # [PH, PW, PD]: train on random patches of the whole scan (data3d.py; each a multiple of 16 for NVNet3D); null: the reference's depth crop
    'patch_fg': 0.33,                  # patch_size only: the share of training patches centred on a tumour voxel (needs label targets: BraTS)
    'patch_flips': 'hwd',              # patch_size only, with aug: the axes a training patch may be mirrored on
    'patch_warp': 0.0,                 # patch_size only, with aug: the share of training patches rotated and zoomed on the device (patch3d.patch_warp); 0: off
    'patch_rot': [30, 30, 30],         # patch_warp only: the largest absolute rotation about the H, W and D axes in degrees, each in 0 .. 45
    'patch_zoom': [0.7, 1.4],          # patch_warp only: [lo, hi] of the zoom, lo <= hi in 0.5 .. 2; above 1 magnifies
    'patch_blur': 0.0,                 # patch_size only, with aug: the share of training items whose contrasts may be blurred on the device (tone3d.py; each contrast with probability 1 / 2); 0: off
    'patch_blur_sigma': [0.5, 1.0],    # patch_blur only: [lo, hi] of sigma in voxels, lo <= hi in 0.25 .. 1 (the tap radius is 4)
    'patch_contrast': 0.0,             # patch_size only, with aug: the share of training items with a contrast change about the tissue mean; 0: off
    'patch_contrast_range': [0.75, 1.25],      # patch_contrast only: [lo, hi] of the factor, lo <= hi in 0.5 .. 2
    'patch_gamma': 0.0,                # patch_size only, with aug: the share of training items with a gamma curve over the tissue range; 0: off
    'patch_gamma_range': [0.7, 1.5],   # patch_gamma only: [lo, hi] of the exponent, lo <= hi in 0.5 .. 2
    'patch_gamma_invert': 0.25,        # patch_gamma only: the share of the gamma'd contrasts that take the inverted curve 1 - (1 - t) ** gamma
    'patch_noise': 0.0,                # patch_size only, with aug: the share of training items with additive noise; 0: off
    'patch_noise_std': [0.0, 0.3],     # patch_noise only: [lo, hi] of the standard deviation in store units, lo <= hi in 0 .. 1
    'epochs': 300, 'lr': 1e-4, 'weight_decay': 1e-5,
    'lr_schedule': 'poly',             # none | poly: lr * (1 - epoch / epochs) ** 0.9
    'fused_loss': True,                # false: the torch composition `nvnet_loss`
    'ckpt_path': '../ckpt3d/', 'continue_train': False,
    'ckpt_name': None,                 # checkpoint file to load; None: the last epochNNN.pth.tar (continue_train) / model_best.pth.tar (test)
    'seed': 10, 'device': 'cuda:0',
    'max_batches': None,               # cap on the batches of every train / validation / test pass (tests)
    'predict_set': 'test',             # phase predict: the loader whose subjects are predicted (train | val | test; it must serve them as stored)
    'predict_stride': None,            # depth stride of the sliding window; None: half the trained depth
    'predict_flip': False,             # also average the prediction of the H-flipped input
    'predict_tile': None,              # [TH, TW, TD]: predict tile by tile (model3d.predict_tiles; each a multiple of 8, at most the volume); null: the depth window over the full planes
    'predict_tile_stride': None,       # predict_tile only: [SH, SW, SD], the stride of the tiles; null: half the tile
    'predict_weight': 'gaussian',      # predict_tile only: gaussian | uniform, the weight of a tile position in the blend
    'predict_sigma': 0.125,            # predict_tile only, gaussian: the standard deviation as a share of the tile extent, 0.05 .. 1
    'predict_mirror': '',              # predict_tile only: the axes of 'hwd' whose mirrored views are averaged in (2^n forwards per tile)
    'predict_regions': False,          # phase predict: also write predict_regions.csv (Dice, sensitivity, specificity, HD95 of WT / TC / ET; BraTS only)
    'predict_lesions': False,          # phase predict / score / postprocess: also write predict_lesions.csv (lesion-wise Dice and HD95 of WT / TC / ET; BraTS only)
    'lesion_dilation': 3,              # lesion.lesion_scores: dilations of the ground truth by the 18-neighbourhood before it is split into lesions, 0 .. 8
    'lesion_min_voxels': 50,           # lesion.lesion_scores: a ground-truth lesion of fewer voxels is not scored
    'predict_post': False,             # phase predict: also write the cleaned label maps under result_<predict_set>/post/ (postproc.clean_labels)
    'post_connectivity': 26,           # connectivity of the components: 6 | 18 | 26
    'post_min_voxels': 0,              # components of fewer voxels are removed
    'post_keep': 'all',                # all | largest (only the largest component of a subject is a candidate)
    'post_et_min_voxels': 0,           # > 0: an enhancing tumour (label 4) of fewer voxels becomes necrotic core (label 1); BraTS only
    'score_subdir': '',                # phase score: the sub-directory of result_<predict_set>/ it reads and writes ('post': the cleaned maps)
    'write_nifti': False,              # phase predict / postprocess: also write <subj_id>_seg.nii.gz beside every <subj_id>_seg.npy, on the scans' own
                                       # 240 x 240 x 155 canvas and in their geometry (prep.save_nifti); needs data_source raw
}
PHASES = ('train', 'test', 'predict', 'score', 'postprocess')
NO_MODEL_PHASES = ('score', 'postprocess')
POST_SUBDIR = 'post'
POST_FG = (1, 2, 3, 4, 5, 6, 7)        # every non-zero label is foreground
REGION_CSV_KEYS = (('dice', 'dice'), ('sens', 'sensitivity'), ('spec', 'specificity'), ('hd95', 'hd95'))      # csv column prefix, region_scores key
MODEL_NAMES = ('NVNet3D', 'UNet3D')
LR_SCHEDULES = ('none', 'poly')
DATA_SOURCES = ('h5', 'raw')
STAT_KEYS = ('loss', 'loss_dice', 'loss_l2', 'loss_kl')


def load_config3d(path=None, overrides=None):
    """DEFAULT_CONFIG_3D <- the yaml file (if `path` is given it must exist) <- overrides; unknown keys are refused."""
    cfg = dict(DEFAULT_CONFIG_3D)
    if path is not None:
        with open(path) as f:
            cfg.update(yaml.safe_load(f) or {})
    cfg.update(overrides or {})
    unknown = sorted(set(cfg) - set(DEFAULT_CONFIG_3D))
    if unknown:
        raise KeyError(f'unknown config key(s) {unknown}: one of {sorted(DEFAULT_CONFIG_3D)}')
    for k, v in cfg.items():                     # yaml reads `lr=1e-4` (no dot) as a string
        if isinstance(DEFAULT_CONFIG_3D[k], float) and not isinstance(v, bool) and isinstance(v, (str, int)):
            cfg[k] = float(v)
    if cfg['model_name'] not in MODEL_NAMES:
        raise ValueError(f'model_name {cfg["model_name"]!r}: one of {MODEL_NAMES}')
    if cfg['lr_schedule'] not in LR_SCHEDULES:
        raise ValueError(f'lr_schedule {cfg["lr_schedule"]!r}: one of {LR_SCHEDULES}')
    if cfg['data_source'] not in DATA_SOURCES:
        raise ValueError(f'data_source {cfg["data_source"]!r}: one of {DATA_SOURCES}')
    if cfg['data_source'] == 'raw' and not cfg['raw_path']:
        raise ValueError('data_source raw needs raw_path: the directory of the subjects')
    if cfg['patch_size'] is not None:          # (patch_fg, patch_flips and the patch_warp keys are read only with it)
        cfg['patch_size'], cfg['patch_fg'], cfg['patch_flips'] = patch_args(cfg['patch_size'], cfg['patch_fg'], cfg['patch_flips'])
        cfg['patch_size'] = list(cfg['patch_size'])
        cfg['patch_warp'], rot, zoom = patch_warp_args(cfg['patch_warp'], cfg['patch_rot'], cfg['patch_zoom'])
        cfg['patch_rot'], cfg['patch_zoom'] = list(rot), list(zoom)
        for key, v in patch_intensity_args(**{key: cfg[key] for key in INTENSITY_DEFAULTS}).items():
            cfg[key] = list(v) if isinstance(v, tuple) else v
        if cfg['model_name'] == 'NVNet3D' and any(v % 16 for v in cfg['patch_size']):
            raise ValueError(f'patch_size {cfg["patch_size"]}: every extent a multiple of 16 for NVNet3D (its VAE branch decodes from 1 / 16 of the input)')
        if cfg['patch_fg'] > 0 and cfg['dataset_name'] != 'BraTS':
            raise ValueError(f'patch_fg > 0 needs label targets (dataset_name BraTS), not {cfg["dataset_name"]!r}: set patch_fg=0')
    if cfg['phase'] not in PHASES:
        raise ValueError(f'phase {cfg["phase"]!r}: one of {PHASES}')
    if cfg['predict_set'] not in ('train', 'val', 'test'):
        raise ValueError(f'predict_set {cfg["predict_set"]!r}: train, val or test')
    if cfg['predict_stride'] is not None:
        cfg['predict_stride'] = int(cfg['predict_stride'])
        if cfg['predict_stride'] < 1:
            raise ValueError(f'predict_stride {cfg["predict_stride"]}: at least 1 (or null: half the trained depth)')
    check_predict_tile(cfg)
    if not isinstance(cfg['predict_regions'], bool):
        raise ValueError(f'predict_regions {cfg["predict_regions"]!r}: true or false')
    if (cfg['predict_regions'] or cfg['phase'] == 'score') and cfg['dataset_name'] != 'BraTS':
        raise ValueError(f'region scores (predict_regions, phase score) are defined for dataset_name BraTS only, not {cfg["dataset_name"]!r}')
    if not isinstance(cfg['predict_lesions'], bool):
        raise ValueError(f'predict_lesions {cfg["predict_lesions"]!r}: true or false')
    if cfg['predict_lesions'] and cfg['dataset_name'] != 'BraTS':
        raise ValueError(f'region scores (predict_lesions) are defined for dataset_name BraTS only, not {cfg["dataset_name"]!r}')
    if isinstance(cfg['lesion_dilation'], bool) or not isinstance(cfg['lesion_dilation'], int) or not 0 <= cfg['lesion_dilation'] <= MAX_DILATION:
        raise ValueError(f'lesion_dilation {cfg["lesion_dilation"]!r}: an integer in 0 .. {MAX_DILATION}')
    if isinstance(cfg['lesion_min_voxels'], bool) or not isinstance(cfg['lesion_min_voxels'], int) or cfg['lesion_min_voxels'] < 0:
        raise ValueError(f'lesion_min_voxels {cfg["lesion_min_voxels"]!r}: an integer >= 0')
    if not isinstance(cfg['predict_post'], bool):
        raise ValueError(f'predict_post {cfg["predict_post"]!r}: true or false')
    if isinstance(cfg['post_connectivity'], bool) or cfg['post_connectivity'] not in CONNECTIVITIES:
        raise ValueError(f'post_connectivity {cfg["post_connectivity"]!r}: one of {CONNECTIVITIES}')
    if cfg['post_keep'] not in KEEP_MODES:
        raise ValueError(f'post_keep {cfg["post_keep"]!r}: one of {KEEP_MODES}')
    for k in ('post_min_voxels', 'post_et_min_voxels'):
        if isinstance(cfg[k], bool) or not isinstance(cfg[k], int) or cfg[k] < 0:
            raise ValueError(f'{k} {cfg[k]!r}: an integer >= 0')
    if cfg['post_et_min_voxels'] > 0 and cfg['dataset_name'] != 'BraTS':
        raise ValueError(f'post_et_min_voxels > 0 (the enhancing-tumour rule) is defined for dataset_name BraTS only, not {cfg["dataset_name"]!r}')
    if not isinstance(cfg['write_nifti'], bool):
        raise ValueError(f'write_nifti {cfg["write_nifti"]!r}: true or false')
    if cfg['write_nifti'] and cfg['data_source'] != 'raw':
        raise ValueError(f'write_nifti needs data_source raw (the crop and the headers of the scans), not {cfg["data_source"]!r}')
    sub = cfg['score_subdir']
    if not isinstance(sub, str) or os.path.isabs(sub) or any(p in ('.', '..') for p in sub.replace('\\', '/').split('/')):
        raise ValueError(f'score_subdir {sub!r}: a relative sub-directory of result_<predict_set>/ (or the empty string)')
    return cfg


NET_DIVISOR = 8                        # UNet3D halves its input three times and adds the skips back: every extent a multiple of 8


def check_predict_tile(cfg, shape=None):
    """the tile-wise prediction keys of a config, normalised in place (lists of int); ValueError naming the key.  `shape`: the stored volumes'
    (H, W, D), where known -- the tile must fit it.  With predict_tile null the other four keys are not read."""
    if cfg['predict_tile'] is None:
        return
    for key in ('predict_tile', 'predict_tile_stride'):
        v = cfg[key]
        if v is None and key == 'predict_tile_stride':
            continue
        try:
            ok = not isinstance(v, str) and len(v) == 3 and all(not isinstance(x, bool) and isinstance(x, int) and x >= 1 for x in v)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f'{key} {v!r}: null or three integers >= 1')
        cfg[key] = [int(x) for x in v]
    if any(t % NET_DIVISOR for t in cfg['predict_tile']):
        raise ValueError(f'predict_tile {cfg["predict_tile"]}: every extent a multiple of {NET_DIVISOR} (the U-Net halves its input three times)')
    if cfg['predict_stride'] is not None:
        raise ValueError('predict_stride belongs to the depth window: with predict_tile set predict_tile_stride: [SH, SW, SD]')
    if cfg['predict_flip']:
        raise ValueError('predict_flip belongs to the depth window: with predict_tile set predict_mirror: h')
    if cfg['predict_weight'] not in TILE_WEIGHTS:
        raise ValueError(f'predict_weight {cfg["predict_weight"]!r}: one of {TILE_WEIGHTS}')
    try:
        tile_weights(1, cfg['predict_weight'], cfg['predict_sigma'])
    except ValueError as e:
        raise ValueError(f'predict_sigma: {e}') from None
    try:
        tile_views(cfg['predict_mirror'])
    except ValueError as e:
        raise ValueError(f'predict_mirror: {e}') from None
    if shape is not None:
        try:
            tile_offsets(shape, cfg['predict_tile'], cfg['predict_tile_stride'])
        except ValueError as e:
            raise ValueError(f'predict_tile: {e}') from None


def region_csv_header():
    return 'subj_id,' + ','.join(f'{col}_{name}' for col, _ in REGION_CSV_KEYS for name, _ in BRATS_REGIONS)


def write_region_csv(path, subj, scores):
    """predict_regions.csv: `subj_id,dice_wt,dice_tc,dice_et,sens_wt,...,spec_et,hd95_wt,hd95_tc,hd95_et`, one row per subject, floats written
    with repr; scores: {key: (n, 3) float64} of `region_scores`.  -> the per-region means {'dice_wt': ..., ...} over the subjects that have a
    value (NaN = no ground truth; NaN if none has one)."""
    cols = [(f'{col}_{name}', scores[key][:, r].tolist()) for col, key in REGION_CSV_KEYS for r, (name, _) in enumerate(BRATS_REGIONS)]
    with open(path, 'w') as f:
        f.write(region_csv_header() + '\n')
        for i, sid in enumerate(subj):
            f.write(sid + ',' + ','.join(repr(v[i]) for _, v in cols) + '\n')
    means = {}
    for name, v in cols:
        have = [x for x in v if x == x]
        means[name] = float(np.mean(have)) if have else float('nan')
    return means


def write_lesion_csv(path, subj, scores):
    """predict_lesions.csv: `subj_id,ldice_wt,ldice_tc,ldice_et,lhd95_wt,...,lesions_wt,...,kept_*,missed_*,comps_*,fp_et`, one row per subject
    (lesion.lesion_csv_header: floats written with repr, counts as integers); scores: the `lesion_scores` dicts of the batches, in the order of
    `subj`.  -> the per-column means {'ldice_wt': ..., ...} over the subjects that have a value (NaN = no ground truth; NaN if none has one)."""
    rows = [lesion_csv_values(sc, i) for sc in scores for i in range(sc['lesion_dice'].shape[0])]
    if len(rows) != len(subj):
        raise ValueError(f'write_lesion_csv: {len(subj)} subjects need {len(subj)} rows of scores, got {len(rows)}')
    names = lesion_csv_header().split(',')
    with open(path, 'w') as f:
        f.write('subj_id,' + ','.join(names) + '\n')
        for sid, row in zip(subj, rows):
            f.write(sid + ',' + ','.join(row) + '\n')
    means = {}
    for c, name in enumerate(names):
        have = [float(r[c]) for r in rows if float(r[c]) == float(r[c])]
        means[name] = float(np.mean(have)) if have else float('nan')
    return means


def parse_argv(argv):
    """`[config3d.yaml] key=value ...` -> (path or None, overrides), as main_missing.py reads its command line."""
    argv = list(argv)
    path = None
    if argv and '=' not in argv[0]:
        path = argv.pop(0)
    return path, parse_overrides(argv)


def poly_lr(lr, epoch, epochs):
    return lr * (1.0 - epoch / float(epochs)) ** 0.9


def epoch_lr(config, epoch):
    return poly_lr(config['lr'], epoch, config['epochs']) if config['lr_schedule'] == 'poly' else config['lr']


def dice_loss_torch(uout, target):
    """the Dice term of `nvnet_loss` alone (UNet3D with fused_loss: false)"""
    p = torch.sigmoid(uout)
    return 1 - 2 * (p * target).sum() / ((p * p).sum() + (target * target).sum() + 1e-6)


def last_epoch_checkpoint(ckpt_path):
    """name of the epochNNN.pth.tar with the highest epoch number (by value: 'epoch1000' comes after 'epoch999')"""
    best = None
    for fn in glob.glob(os.path.join(ckpt_path, 'epoch*.pth.tar')):
        m = re.fullmatch(r'epoch(\d+)\.pth\.tar', os.path.basename(fn))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), os.path.basename(fn))
    if best is None:
        raise ValueError(f'No correct checkpoint under {ckpt_path}')
    return best[1]


class Run3D:
    """model + ArenaAdam + the three loaders of a fold, with train() / evaluate().  `store`: a VolumeStore3D instead of the h5 file under
    `data_path` (the list files are still read from there); `data`: a ready VolumeData3D-like object (trainLoader / valLoader / testLoader)."""

    def __init__(self, config, store=None, data=None, log=print):
        if dist.is_available() and dist.is_initialized():
            raise NotImplementedError('Run3D runs on one process only (world size 1): data-parallel 3-D training is not implemented; '
                                      'start it without a process group')
        self.config = cfg = load_config3d(None, config)
        self.log = log
        self.device = dev = torch.device(cfg['device'])
        torch.manual_seed(cfg['seed']); np.random.seed(cfg['seed'])
        if dev.type == 'cuda':
            torch.cuda.manual_seed(cfg['seed'])
        if data is None and store is None and cfg['data_source'] == 'raw':
            if cfg['dataset_name'] != 'BraTS':
                raise NotImplementedError(f'data_source raw: only the BraTS directory naming is restated (prep.subject_files), not {cfg["dataset_name"]}')
            store, kept = build_store_from_raw(cfg['raw_path'], dev, store_cls=VolumeStore3D, norm_type=cfg['norm_type'], crop=cfg['raw_crop'],
                                               contrasts=cfg['contrast_list'], log=log)
            ensure_fold_lists(kept, cfg['data_path'], VolumeData3D.file_names('BraTS', cfg['norm_type'], cfg['fold'])[1:])
        if data is None:
            data = VolumeData3D(cfg['dataset_name'], cfg['data_path'], norm_type=cfg['norm_type'], batch_size=cfg['batch_size'], fold=cfg['fold'],
                                shuffle=True, contrast_list=cfg['contrast_list'], aug=cfg['aug'], dropoff=cfg['dropoff'], store=store,
                                device=dev, region_channels=3, patch_size=cfg['patch_size'], patch_fg=cfg['patch_fg'], patch_flips=cfg['patch_flips'],
                                patch_warp=cfg['patch_warp'], patch_rot=cfg['patch_rot'], patch_zoom=cfg['patch_zoom'],
                                **({key: cfg[key] for key in INTENSITY_DEFAULTS} if cfg['patch_size'] is not None else {}))
        self.data = data
        self.loaders = {'train': data.trainLoader, 'val': data.valLoader, 'test': data.testLoader}
        if cfg['phase'] == 'predict':
            check_predict_tile(cfg, self.loaders[cfg['predict_set']].dataset.store.shape)      # the tile must fit the volumes: before any launch
        ds = data.trainLoader.dataset
        H, W, _ = ds.store.shape
        patch = getattr(ds, 'patch_size', None)
        self.input_shape = tuple(patch) if patch is not None else (H, W, ds.crop()[1])      # patch training: the net is built for the patch
        self.start_epoch = -1
        self.best_dice = -1.0
        if cfg['phase'] in NO_MODEL_PHASES:    # works on label volumes that are already written: no model, no optimizer, no checkpoint
            self.model = self.optimizer = None
            return
        M = len(cfg['contrast_list'])
        net = NVNet3D if cfg['model_name'] == 'NVNet3D' else UNet3D
        self.model = net(self.input_shape, M, 3, cfg['init_channels'], p=cfg['p']).to(dev)
        self.optimizer = ArenaAdam(self.model.parameters(), lr=cfg['lr'], weight_decay=cfg['weight_decay'], used=list(self.model.parameters()))
        if cfg['continue_train'] or cfg['phase'] in ('test', 'predict'):
            self._load(cfg['ckpt_name'] or (last_epoch_checkpoint(cfg['ckpt_path']) if cfg['phase'] == 'train' else 'model_best.pth.tar'))
        if cfg['phase'] == 'train':
            os.makedirs(cfg['ckpt_path'], exist_ok=True)
            save_config_file(cfg)

    # ---- RNG states in the checkpoint
    def _generators(self):
        return {k: l.generator for k, l in self.loaders.items() if getattr(l, 'generator', None) is not None}

    def rng_state(self):
        st = {'numpy': np.random.get_state(), 'torch': torch.get_rng_state(),
              'loaders': {k: g.get_state() for k, g in self._generators().items()}}
        if self.device.type == 'cuda':
            st['device'] = torch.cuda.get_rng_state(self.device)
        return st

    def set_rng_state(self, st):
        np.random.set_state(st['numpy'])
        torch.set_rng_state(st['torch'].cpu())
        if self.device.type == 'cuda' and 'device' in st:
            torch.cuda.set_rng_state(st['device'].cpu(), self.device)
        for k, g in self._generators().items():
            if k in st.get('loaders', {}):
                g.set_state(st['loaders'][k].cpu())

    def _load(self, name):
        cfg = self.config
        fn = os.path.join(cfg['ckpt_path'], name)
        if not os.path.isfile(fn):
            raise ValueError(f'No correct checkpoint: {fn}')
        ck = torch.load(fn, map_location=self.device, weights_only=False)
        missing = load_checkpoint_model(self.model, ck['model'])
        if missing:
            raise ValueError(f'{fn}: {len(missing)} tensors do not fit {cfg["model_name"]} (init_channels {cfg["init_channels"]}), e.g. {missing[:3]}')
        if cfg['phase'] == 'train':
            self.optimizer.load_state_dict(ck['optimizer'])
            self.best_dice = float(ck.get('best_dice', ck['monitor_metric']))
            if 'rng' in ck:
                self.set_rng_state(ck['rng'])
        self.start_epoch = int(ck['epoch'])
        self.log(f'loaded {name} (epoch {self.start_epoch}, validation dice {float(ck["monitor_metric"]):.4f})')

    # ---- the objective
    def objective(self, out, x, target):
        """(loss, [loss, dice term, l2, kl] as a device vector) of one forward"""
        fused = self.config['fused_loss']
        if self.config['model_name'] == 'NVNet3D':
            uout, vout, mu, logvar = out
            loss, parts = (nvnet_loss_hip if fused else nvnet_loss)(uout, vout, mu, logvar, x, target)
        else:
            uout = out[0]
            if fused:
                loss, parts = nvnet_loss_hip(uout, None, None, None, x, target)
            else:
                loss = dice_loss_torch(uout, target)
                zero = torch.zeros((), dtype=torch.float32, device=uout.device)
                parts = {'dice': loss, 'l2': zero, 'kl': zero}
        vec = torch.stack([loss.detach().reshape(()), parts['dice'].detach().reshape(()), parts['l2'].detach().reshape(()),
                           parts['kl'].detach().reshape(())])
        return loss, vec

    def train_step(self, batch):
        x, target = batch['inputs'], batch['targets']
        loss, vec = self.objective(self.model(x), x, target)
        loss.backward()
        self.optimizer.step(fused_clip=True)
        self.optimizer.zero_grad()
        return vec

    def _batches(self, loader):
        return loader.batches(limit=self.config['max_batches']) if self.config['max_batches'] else iter(loader)

    def train(self):
        """epochs start_epoch + 1 .. epochs - 1"""
        return self._train(self.config['epochs'])

    def _train(self, stop):
        """epochs start_epoch + 1 .. stop - 1; a `stop` below `epochs` ends the run as an interruption would (the schedule still spans `epochs`)"""
        cfg = self.config
        for epoch in range(self.start_epoch + 1, min(cfg['epochs'], stop)):
            self.optimizer.param_groups[0]['lr'] = epoch_lr(cfg, epoch)
            self.model.train()
            acc, n = None, 0
            for batch in self._batches(self.loaders['train']):
                vec = self.train_step(batch)
                acc = vec if acc is None else acc + vec             # device accumulators: one D2H copy per epoch
                n += 1
            if n == 0:
                raise RuntimeError(f'epoch {epoch}: the train loader yielded no batch')
            mean = (acc.double() / n).cpu()
            train_stat = {k: float(mean[i]) for i, k in enumerate(STAT_KEYS)}
            if not np.isfinite(train_stat['loss']):
                raise FloatingPointError(f'epoch {epoch}: loss is {train_stat["loss"]}')
            save_result_stat(train_stat, cfg, info='epoch[%2d]' % epoch)
            stat = self.evaluate('val')
            save_result_stat(stat, cfg, info='val')
            is_best = stat['dice'] > self.best_dice
            if is_best:
                self.best_dice = stat['dice']
            state = {'epoch': epoch, 'monitor_metric': stat['dice'], 'best_dice': self.best_dice, 'stat': stat,
                     'optimizer': self.optimizer.state_dict(), 'scheduler': {'lr_schedule': cfg['lr_schedule']},
                     'model': self.model.state_dict(), 'rng': self.rng_state()}
            save_checkpoint(state, is_best, cfg['ckpt_path'])
            self.last_stat = stat
            self.log(f'epoch {epoch}: train loss {train_stat["loss"]:.4f}, val loss {stat["loss"]:.4f}, dice {stat["dice"]:.4f}, '
                     f'iou {stat["iou"]:.4f}, lr {self.optimizer.lr:g}, best {is_best}')
        return self

    def evaluate(self, set_='val'):
        """eval-mode pass over a loader: the loss means over its batches, the mean Dice / IoU over its volumes"""
        self.model.eval()
        acc, n, counts = None, 0, []
        with torch.no_grad():
            for batch in self._batches(self.loaders[set_]):
                x, target = batch['inputs'], batch['targets']
                out = self.model(x)
                _, vec = self.objective(out, x, target)
                counts.append(hip.seg_counts(out[0], target, logits=True))
                acc = vec if acc is None else acc + vec
                n += 1
        if n == 0:
            raise RuntimeError(f'evaluate({set_!r}): the loader yielded no batch')
        mean = (acc.double() / n).cpu()
        stat = {k: float(mean[i]) for i, k in enumerate(STAT_KEYS)}
        met = seg_metrics_from_counts(torch.cat(counts).cpu().numpy())      # one D2H copy per pass
        stat['dice'], stat['iou'] = float(met['dice'].mean()), float(met['iou'].mean())
        return stat

    def predict(self, set_=None):
        """whole-volume prediction -- the sliding depth window (model3d.predict_volumes) or, with `predict_tile`, overlapping tiles blended by
        `predict_weight` and averaged over the views of `predict_mirror` (model3d.predict_tiles) -- of every subject the `set_` loader serves (None: `predict_set`):
        writes <ckpt_path>/result_<set>/<subj_id>_seg.npy -- uint8 (H, W, D), the store's own geometry and labels (BraTS: 0 / 1 / 2 / 4) -- and
        result_<set>/predict.csv with a header and one `subj_id,dice,iou` row per subject (the reference's Dice / IoU over the FULL depth);
        returns their means.  One D2H copy of the labels per batch, one of all counts at the end; no window syncs with the host.
        `predict_regions: true` also scores every batch by BraTS region on the labels it holds on the device (surfdist.region_scores; one more small
        D2H copy per batch), writes result_<set>/predict_regions.csv (`write_region_csv`) and adds the per-region means to the returned stat.
        `predict_lesions: true` also scores every batch lesion by lesion (lesion.lesion_scores under `lesion_dilation` / `lesion_min_voxels`), writes
        result_<set>/predict_lesions.csv (`write_lesion_csv`; with `predict_post` also post/predict_lesions.csv for the cleaned labels) and adds
        the per-column means to the returned stat; false: no lesion kernel launches and every file is what it is without the key.
        `predict_post: true` also cleans the labels of every batch on the device (`clean`), writes them as result_<set>/post/<subj_id>_seg.npy
        with post/postprocess.csv (and, with `predict_regions`, post/predict_regions.csv: the region scores of the cleaned labels), and adds
        'post_<column>' means to the returned stat: one more D2H copy of the cleaned labels and one small copy of the stats per batch.  The raw
        files are written exactly as without it.
        `write_nifti: true` (data_source raw) also writes <subj_id>_seg.nii.gz beside every <subj_id>_seg.npy, under post/ too: uint8 on the scans'
        own canvas, 0 outside the crop, in the geometry of the subject's seg file (prep.save_nifti); the .npy and csv files do not change."""
        cfg = self.config
        set_ = cfg['predict_set'] if set_ is None else set_
        out_dir = os.path.join(cfg['ckpt_path'], f'result_{set_}')
        os.makedirs(out_dir, exist_ok=True)
        subj, counts, regions, lesions = [], [], [], []
        nifti = self._nifti_writer(set_)
        post = _PostWriter(out_dir, cfg['predict_regions'], nifti, self.lesions if cfg['predict_lesions'] else None) if cfg['predict_post'] else None
        if cfg['predict_tile'] is None:
            results = predict_volumes(self.model, self.loaders[set_], stride=cfg['predict_stride'], flip=cfg['predict_flip'],
                                      limit=cfg['max_batches'] or None)
        else:       # tile by tile (model3d.predict_tiles): the same dict, so everything below is what it was
            check_predict_tile(cfg, self.loaders[set_].dataset.store.shape)
            results = predict_tiles(self.model, self.loaders[set_], cfg['predict_tile'], stride=cfg['predict_tile_stride'], weight=cfg['predict_weight'],
                                    sigma=cfg['predict_sigma'], mirror=cfg['predict_mirror'], limit=cfg['max_batches'] or None)
        for res in results:
            if cfg['predict_regions']:
                regions.append(region_scores(res['labels'], res['target_ptrs']))
            if cfg['predict_lesions']:
                lesions.append(self.lesions(res['labels'], res['target_ptrs']))
            if post is not None:
                post.add(res['subj_id'], *self.clean(res['labels']), res['target_ptrs'])
            labels = res['labels'].cpu().numpy()
            for i, sid in enumerate(res['subj_id']):
                np.save(os.path.join(out_dir, f'{sid}_seg.npy'), labels[i])
            if nifti is not None:
                nifti(out_dir, res['subj_id'], res['labels'])
            subj += res['subj_id']
            counts.append(res['counts'])
        if not subj:
            raise RuntimeError(f'predict({set_!r}): the loader yielded no batch')
        met = seg_metrics_from_counts(torch.cat(counts).cpu().numpy())
        with open(os.path.join(out_dir, 'predict.csv'), 'w') as f:
            f.write('subj_id,dice,iou\n')
            for sid, d, i in zip(subj, met['dice'].tolist(), met['iou'].tolist()):
                f.write(f'{sid},{d!r},{i!r}\n')
        stat = {'dice': float(met['dice'].mean()), 'iou': float(met['iou'].mean()), 'n': len(subj)}
        if cfg['predict_regions']:
            stat.update(write_region_csv(os.path.join(out_dir, 'predict_regions.csv'), subj,
                                         {k: torch.cat([r[k] for r in regions]) for k in SCORE_KEYS}))
        if cfg['predict_lesions']:
            stat.update(write_lesion_csv(os.path.join(out_dir, 'predict_lesions.csv'), subj, lesions))
        if post is not None:
            stat.update({f'post_{k}': v for k, v in post.finish().items()})
        self.log(f'predict {set_}: {len(subj)} volumes under {out_dir}, dice {stat["dice"]:.4f}, iou {stat["iou"]:.4f}')
        return stat

    def _nifti_writer(self, set_):
        """`write_nifti: true`: f(directory, subject ids, (B, H, W, D) labels on the device) that writes <subj_id>_seg.nii.gz per subject (prep.save_nifti:
        one launch, one D2H copy and one file each, in the subject's own geometry); else None, and no export kernel ever launches"""
        if not self.config['write_nifti']:
            return None
        store = self.loaders[set_].dataset.store

        def write(out_dir, ids, labels):
            for i, sid in enumerate(ids):
                save_nifti(os.path.join(out_dir, f'{sid}_seg.nii.gz'), labels[i], store, sid, log=self.log)
        return write

    def lesions(self, labels, target_ptrs):
        """the lesion-wise scores of a batch of label volumes on the device under the `lesion_*` keys (lesion.lesion_scores, BraTS regions)"""
        cfg = self.config
        return lesion_scores(labels, target_ptrs, BRATS_REGIONS, dilation=cfg['lesion_dilation'], min_voxels=cfg['lesion_min_voxels'])

    def clean(self, labels):
        """(cleaned, stats) of a batch of label volumes on the device under the `post_*` keys (postproc.clean_labels; every non-zero label
        is foreground, the ET rule relabels BraTS's 4 as 1)"""
        cfg = self.config
        return clean_labels(labels, fg=POST_FG, connectivity=cfg['post_connectivity'], min_voxels=cfg['post_min_voxels'], keep=cfg['post_keep'],
                            et_label=4, et_min_voxels=cfg['post_et_min_voxels'], et_replace=1)

    def _stored_labels(self, in_dir, set_):
        """the label volumes ALREADY under `in_dir` (`<subj_id>_seg.npy`, uint8 (H, W, D) in the store's geometry), batch by batch in the
        loader's plain order: yields (subject ids, labels (B, H, W, D) on the device, ground-truth pointer table).  A missing file, a wrong
        shape or a wrong dtype raises ValueError naming it."""
        cfg = self.config
        loader = self.loaders[set_]
        shape = tuple(loader.dataset.store.shape)
        for _, _, metas in loader.plain_plan(cfg['max_batches'] or None):
            vols = []
            for m in metas:
                fn = os.path.join(in_dir, f'{m[0]}_seg.npy')
                if not os.path.isfile(fn):
                    raise ValueError(f'{fn}: no such label volume (phase predict writes it)')
                try:
                    v = np.load(fn, allow_pickle=False)
                except Exception as e:
                    raise ValueError(f'{fn}: not a readable .npy file ({e})') from e
                if v.dtype != np.uint8 or tuple(v.shape) != shape:
                    raise ValueError(f'{fn}: a uint8 {shape} label volume is wanted, got {v.dtype} {tuple(v.shape)}')
                vols.append(torch.from_numpy(np.ascontiguousarray(v)))
            labels = torch.stack(vols).to(self.device)
            ptrs = torch.tensor([int(m[4]) for m in metas], dtype=torch.int64).to(self.device)
            yield [m[0] for m in metas], labels, ptrs

    def postprocess(self, set_=None):
        """cleans the label volumes ALREADY under <ckpt_path>/result_<set>/ (as `predict` writes them; the checks of `score`) under the
        `post_*` keys: writes result_<set>/post/<subj_id>_seg.npy and post/postprocess.csv, for BraTS also post/predict_regions.csv (the
        region scores of the cleaned labels; with `predict_lesions` also post/predict_lesions.csv) -- the files `predict` writes with
        `predict_post: true`, byte for byte.  Returns the means of
        the stats columns and, for BraTS, the per-region means."""
        cfg = self.config
        set_ = cfg['predict_set'] if set_ is None else set_
        in_dir = os.path.join(cfg['ckpt_path'], f'result_{set_}')
        post = None
        for ids, labels, ptrs in self._stored_labels(in_dir, set_):
            if post is None:
                post = _PostWriter(in_dir, cfg['dataset_name'] == 'BraTS', self._nifti_writer(set_), self.lesions if cfg['predict_lesions'] else None)
            post.add(ids, *self.clean(labels), ptrs)
        if post is None:
            raise RuntimeError(f'postprocess({set_!r}): the loader serves no subject')
        stat = post.finish()
        stat['n'] = len(post.subj)
        self.log(f'postprocess {set_}: {len(post.subj)} volumes under {post.out_dir}, ' + ', '.join(f'{k} {v:.4f}' for k, v in stat.items() if k != 'n'))
        return stat

    def score(self, set_=None):
        """region scores of the label volumes ALREADY under <ckpt_path>/result_<set>/ (`<subj_id>_seg.npy`, uint8 (H, W, D) in the store's geometry,
        as `predict` writes them) against the store's ground truth: writes result_<set>/predict_regions.csv and returns the per-region means.
        Every subject the `set_` loader serves must have its file; a missing file, a wrong shape or a wrong dtype raises ValueError naming it.
        With `score_subdir` the files are read and written under result_<set>/<score_subdir>/ instead ('post': the cleaned volumes).
        `predict_lesions: true` also writes predict_lesions.csv there (the lesion-wise scores, as `predict` writes them)."""
        cfg = self.config
        set_ = cfg['predict_set'] if set_ is None else set_
        out_dir = os.path.join(cfg['ckpt_path'], f'result_{set_}')
        if cfg['score_subdir']:
            out_dir = os.path.join(out_dir, cfg['score_subdir'])
        subj, regions, lesions = [], [], []
        for ids, labels, ptrs in self._stored_labels(out_dir, set_):
            regions.append(region_scores(labels, ptrs))
            if cfg['predict_lesions']:
                lesions.append(self.lesions(labels, ptrs))
            subj += ids
        if not subj:
            raise RuntimeError(f'score({set_!r}): the loader serves no subject')
        stat = write_region_csv(os.path.join(out_dir, 'predict_regions.csv'), subj, {k: torch.cat([r[k] for r in regions]) for k in SCORE_KEYS})
        if cfg['predict_lesions']:
            stat.update(write_lesion_csv(os.path.join(out_dir, 'predict_lesions.csv'), subj, lesions))
        stat['n'] = len(subj)
        self.log(f'score {set_}: {len(subj)} volumes under {out_dir}, ' + ', '.join(f'{k} {v:.4f}' for k, v in stat.items() if k != 'n'))
        return stat


class _PostWriter:
    """the files under result_<set>/post/: `add` takes a batch of cleaned labels and stats on the device (one D2H copy each, and with
    `regions` their region scores), `finish` writes postprocess.csv (and predict_regions.csv) and returns the column (and region) means"""

    def __init__(self, result_dir, regions, nifti=None, lesions=None):
        self.out_dir = os.path.join(result_dir, POST_SUBDIR)
        self.nifti = nifti                 # Run3D._nifti_writer: also write the cleaned labels as NIfTI files
        os.makedirs(self.out_dir, exist_ok=True)
        self.subj, self.stats, self.regions = [], [], ([] if regions else None)
        self.lesion_fn, self.lesions = lesions, []      # Run3D.lesions: also write predict_lesions.csv for the cleaned labels

    def add(self, ids, cleaned, stats, target_ptrs):
        if self.regions is not None:
            self.regions.append(region_scores(cleaned, target_ptrs))
        if self.lesion_fn is not None:
            self.lesions.append(self.lesion_fn(cleaned, target_ptrs))
        vols = cleaned.cpu().numpy()
        for i, sid in enumerate(ids):
            np.save(os.path.join(self.out_dir, f'{sid}_seg.npy'), vols[i])
        if self.nifti is not None:
            self.nifti(self.out_dir, ids, cleaned)
        self.subj += list(ids)
        self.stats.append(stats.cpu().numpy())

    def finish(self):
        rows = np.concatenate(self.stats)
        write_stats_csv(os.path.join(self.out_dir, 'postprocess.csv'), self.subj, rows)
        stat = {k: float(rows[:, i].mean()) for i, k in enumerate(STATS_COLUMNS)}
        if self.regions is not None:
            stat.update(write_region_csv(os.path.join(self.out_dir, 'predict_regions.csv'), self.subj,
                                         {k: torch.cat([r[k] for r in self.regions]) for k in SCORE_KEYS}))
        if self.lesion_fn is not None:
            stat.update(write_lesion_csv(os.path.join(self.out_dir, 'predict_lesions.csv'), self.subj, self.lesions))
        return stat


def main(argv=None):
    path, overrides = parse_argv(sys.argv[1:] if argv is None else argv)
    if path is None and os.path.exists('config3d.yaml'):
        path = 'config3d.yaml'
    run = Run3D(load_config3d(path, overrides))
    if run.config['phase'] == 'train':
        run.train()
    elif run.config['phase'] == 'predict':
        print(run.predict())
    elif run.config['phase'] == 'score':
        print(run.score())
    elif run.config['phase'] == 'postprocess':
        print(run.postprocess())
    else:
        print(run.evaluate('test'))
    return run
