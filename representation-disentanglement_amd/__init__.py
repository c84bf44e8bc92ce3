"""mrdis -- MI355X-native (gfx950) hot path of the multi-modal MR representation-
disentanglement training step (reference: ouyangjiahong/representation-disentanglement,
src/model.py + src/main_missing.py).

The directory name carries a hyphen (`representation-disentanglement_amd`), so
import it through the `mrdis` alias at the repository root:

    import mrdis
    conv = mrdis.Conv2d(is_cond=True)(7, 32, 4, 2, padding=1)      # reference's factory

Layout: csrc/ (hand-written HIP kernels + C ABI, include/mrdis.h), hip.py (ctypes
binding), ops.py (autograd pairing + torch.ops.mrdis.*), model.py (mirror of the
reference's module interface), trainer.py (train step, flat-arena Adam, gradient
all-reduce), data.py / data3d.py (HBM-resident slice and volume loaders), patch3d.py (patch sampling for the 3-D nets: foreground prefix tables, patch origins, patch gather, rotated and zoomed patches), tone3d.py (blur, contrast, gamma and noise of the patches), tilepred.py (binding of the tile-wise prediction kernels; model3d.predict_tiles drives them), train.py (the runnable main_missing.py-equivalent: epoch loop, scheduler, stat.csv, checkpoints), synth.py (whole-subject synthesis of missing contrasts: phase synthesize), segment.py (whole-subject tumour segmentation per missing-contrast pattern: phase segment), surfdist.py (region scoring of label volumes: Dice, sensitivity, specificity, HD95), postproc.py (clean-up of label volumes by 3-D connected components), lesion.py (lesion-wise Dice and HD95 of label volumes, binary dilation), prep.py (raw NIfTI scans -> a filled volume store on the device, fold lists), train3d.py (the same for the 3-D nets: main_3d.py).  No CPU fallback exists for the hot path.
"""
from . import hip, ops, model, model3d, trainer               # noqa: F401
from .hip import MrdisError, MrdisLibraryError, LIB_PATH      # noqa: F401
from .model import (CondConv2d, Conv2d, HipConv2d, BatchNorm2d, Conv_BN_Act_New,          # noqa: F401
                    Act_Deconv_BN_Concat_New, AnatomyEncoderEncNew, AnatomyEncoderDecNew,
                    ModalityEncoderNew, SPADEBlockNew, SPADENewShared, SPADENewNotShared, SPADENew,
                    Discriminator, MultimodalModel, expand_type)
from .trainer import (TrainStep, GraphedTrainStep, make_train_step, regular_mask, EvalStep, ZGallery, build_z_gallery, nn_source_contrast, ArenaAdam, GradAllReduce, DEFAULT_CONFIG, load_config_yaml,   # noqa: F401
                      derive_config, build_model, synthetic_batch, fit_to_model, forward_losses,
                      save_checkpoint, load_checkpoint_model, LOSS_KEYS)

from .model3d import BasicBlock, VAEBranch, UNet3D, NVNet3D, HipConv3d, nvnet_loss, nvnet_loss_hip, seg_metrics, seg_metrics_from_counts, window_offsets, predict_volumes   # noqa: F401
from .model3d import tile_weights, tile_offsets, tile_norm, tile_views, predict_tiles   # noqa: F401
from .data import VolumeStore, SliceDataset, BatchLoader, load_idx_list   # noqa: F401
from .data3d import VolumeStore3D, VolumeDataset3D, VolumeLoader3D, VolumeData3D, load_subj_list   # noqa: F401
from . import patch3d, warp3d   # noqa: F401,E402
# warp3d imports patch3d, never the reverse; its three functions are reached through patch3d as well, bound here once both are loaded
patch3d.patch_warp, patch3d.warp_matrix, patch3d.pack_warp = warp3d.patch_warp, warp3d.warp_matrix, warp3d.pack_warp
from . import tone3d   # noqa: F401,E402
# the intensity augmentation of the patches (tone3d.py) is reached through patch3d as well, as the warp is
for _n in ('patch_blur', 'patch_stats', 'patch_tone', 'patch_intensify', 'blur_taps', 'pack_tone', 'TONE_EXTRA'):
    setattr(patch3d, _n, getattr(tone3d, _n))
patch3d.TONE_BLUR, patch3d.TONE_CONTRAST, patch3d.TONE_GAMMA, patch3d.TONE_INVERT, patch3d.TONE_NOISE = tone3d.BLUR, tone3d.CONTRAST, tone3d.GAMMA, tone3d.INVERT, tone3d.NOISE
from . import tilepred   # noqa: F401,E402
# the binding of the tile-wise prediction kernels lives in tilepred.py (it imports hip); reached through hip under the same names as well
hip.tile_accum, hip.tile_label_volume = tilepred.tile_accum, tilepred.tile_label_volume
from .patch3d import fg_block_counts, fg_prefix, patch_origins, patch_gather, patch_warp, warp_matrix, patch_intensify   # noqa: F401,E402
from .synth import synthesize_volumes, synth_plan, synth_source, synth_targets, SYNTH_BLOCKS   # noqa: F401,E402
from . import synth   # noqa: F401,E402
from . import segment   # noqa: F401,E402
from .segment import segment_volumes, seg_patterns   # noqa: F401,E402
from . import surfdist   # noqa: F401,E402
from .surfdist import EDT_FAR, BRATS_REGIONS, edt3d_sq, region_scores, scores_from_counts, percentile_ranks, region_masks   # noqa: F401,E402
from . import postproc   # noqa: F401,E402
from .postproc import components3d, clean_labels   # noqa: F401,E402
from . import lesion   # noqa: F401,E402
from .lesion import dilate3d, lesion_scores, lesion_scores_from_rows   # noqa: F401,E402
from . import prep   # noqa: F401,E402
from .prep import read_nifti, prep_stats, prep_write, prep_volume, build_store_from_raw, write_fold_lists, write_nifti, save_nifti, export_store_volume   # noqa: F401,E402
from . import train   # noqa: F401,E402
from . import train3d   # noqa: F401,E402
from .train3d import Run3D   # noqa: F401,E402

__version__ = '0.1.0'
