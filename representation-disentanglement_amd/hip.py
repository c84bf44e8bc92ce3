"""ctypes binding of libmrdis_hip.so (include/mrdis.h) for torch tensors.

Plumbing only: torch owns device memory and the HIP stream; every function
here turns tensors into (device pointer, leading dimension) views and
enqueues the hand-written gfx950 kernels on torch's current stream.  There is
NO fallback: if the shared library is missing, importing the product path on
a GPU box fails loudly (`MrdisLibraryError`).
"""
import collections
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libmrdis_hip.so')


class MrdisLibraryError(RuntimeError):
    pass


class MrdisError(RuntimeError):
    pass


_lib = None
_c = ctypes
_P, _I, _L, _F, _Z = _c.c_void_p, _c.c_int, _c.c_longlong, _c.c_float, _c.c_size_t

_SIGS = {
    'mrdis_strerror': (_c.c_char_p, [_I]),
    'mrdis_version': (_I, []),
    'mrdis_set_option': (_I, [_c.c_char_p, _L]),
    'mrdis_get_option': (_L, [_c.c_char_p]),
    'mrdis_launch_count': (_L, [_c.c_char_p]),
    'mrdis_launch_count_reset': (None, []),
    'mrdis_dynamic_lds_table': (_I, [_c.c_char_p, _I]),
    'mrdis_mix_experts_fwd': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'mrdis_mix_experts_bwd_workspace': (_Z, [_I, _I, _I, _I]),
    'mrdis_mix_experts_bwd': (_I, [_P, _P, _P, _P, _P, _P, _Z, _I, _I, _I, _I, _P]),
    'mrdis_mix_experts_routed_fwd': (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    'mrdis_mix_experts_routed_bwd': (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _Z, _I, _I, _I, _I, _P]),
    'mrdis_copy_bytes': (_I, [_P, _P, _L, _P]),
    'mrdis_stream_fill': (_I, [_P, _L, _F, _P]),
    'mrdis_instnorm_stats': (_I, [_P, _I, _P, _P, _P, _Z, _I, _L, _I, _F, _I, _P]),
    'mrdis_conv2d_fwd_spade': (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    'mrdis_wino_u_job_bytes': (_Z, []),
    'mrdis_wino_u_format': (_I, [_I, _I, _I]),
    'mrdis_wino_u_image_floats': (_L, [_I, _I, _I]),
    'mrdis_s6_filter_image_bytes': (ctypes.c_size_t, [_I, _I, _I]),
    'mrdis_s6_filter_image': (_I, [_P, _I, _I, _I, _P, ctypes.c_size_t, _P]),
    'mrdis_wino_u_image_floats_fmt': (_L, [_I, _I, _I, _I]),
    'mrdis_wino_u_job_blocks': (_I, [_I, _I, _I]),
    'mrdis_wino_u_jobs': (_I, [_P, _I, _I, _P]),
    'mrdis_mix_experts_routed_multi_fwd': (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _I, _P]),
    'mrdis_mix_experts_routed_multi_bwd_workspace': (_Z, [_I, _I, _I, _I, _I]),
    'mrdis_mix_experts_routed_multi_bwd': (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _P, _Z, _I, _I, _I, _I, _P]),
    'mrdis_mix_job_bytes': (_Z, []),
    'mrdis_mix_job_blocks': (_I, [_I, _I, _I]),
    'mrdis_mix_jobs_fwd': (_I, [_P, _I, _I, _P, _I, _I, _P]),
    'mrdis_mix_jobs_bwd': (_I, [_P, _I, _I, _P, _P, _I, _I, _P]),
    'mrdis_conv2d_fwd': (_I, [_P, _I, _P, _P, _P, _P, _I] + [_I] * 11 + [_P, _I, _P]),
    'mrdis_conv2d_bwd_data': (_I, [_P, _I, _P, _P, _P, _I] + [_I] * 10 + [_P, _I, _P]),
    'mrdis_cast_bf16': (_I, [_P, _P, _L, _P]),
    'mrdis_cast_view': (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _L, _P]),
    'mrdis_conv2d_bwd_weight_workspace': (_Z, [_I] * 9),
    'mrdis_conv2d_bwd_weight': (_I, [_P, _I, _P, _I, _P, _P, _P, _Z] + [_I] * 11 + [_P]),
    'mrdis_lrelu_bwd': (_I, [_P, _I, _P, _I, _P, _I, _L, _I, _F, _I, _P]),
    'mrdis_norm_workspace': (_Z, [_I, _L, _I]),
    'mrdis_bn_train_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _L, _I, _F, _F, _I, _I, _P]),
    'mrdis_bn_eval_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _L, _I, _F, _I, _P]),
    'mrdis_bn_train_bwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _Z, _L, _I, _I, _I, _P]),
    'mrdis_instnorm_spade_fwd': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _Z, _I, _L, _I, _F, _I, _P]),
    'mrdis_instnorm_spade_bwd_workspace': (_Z, [_I, _L, _I]),
    'mrdis_instnorm_spade_bwd': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _I, _P, _Z, _I, _L, _I, _I, _P]),
    'mrdis_instnorm_spade_bwd_up2_workspace': (_Z, [_I, _I, _I, _I, _I]),
    'mrdis_instnorm_spade_bwd_up2': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _I, _P, _Z, _I, _I, _I, _I, _P, _I, _I, _P]),
    'mrdis_bilinear_fwd': (_I, [_P, _I, _P, _I] + [_I] * 8 + [_P]),
    'mrdis_bilinear_bwd': (_I, [_P, _I, _P, _I] + [_I] * 8 + [_P]),
    'mrdis_bilinear_up2_stats_workspace': (_Z, [_I, _I, _I]),
    'mrdis_bilinear_up2_stats_applies': (_I, [_I, _I, _I]),
    'mrdis_bilinear_up2_stats_fwd': (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _L, _P, _P, _F, _P, _Z, _I, _P]),
    'mrdis_softmax_mask_drop_fwd': (_I, [_P, _I, _P, _P, _I, _L, _I, _F, _P]),
    'mrdis_softmax_mask_drop_bwd': (_I, [_P, _I, _P, _I, _P, _I, _L, _I, _P]),
    'mrdis_recon_err_workspace': (_Z, [_I, _L, _I]),
    'mrdis_recon_err_fwd': (_I, [_P, _I, _P, _I, _P, _P, _Z, _I, _L, _I, _I, _P]),
    'mrdis_recon_err_bwd': (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _L, _I, _I, _P]),
    'mrdis_recon_metrics_workspace': (_Z, [_I, _I]),
    'mrdis_recon_metrics': (_I, [_P, _I, _P, _I, _P, _P, _Z, _I, _I, _I, _P]),
    'mrdis_slice_gather': (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_volume_gather': (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_fg_block_counts': (_I, [_P, _P, _I, _P, _I, _I, _I, _P]),
    'mrdis_patch_origins': (_I, [_P, _I, _P, _P, _I] + [_I] * 8 + [_P]),
    'mrdis_patch_gather': (_I, [_P, _I, _P, _P, _P] + [_I] * 11 + [_P]),
    'mrdis_patch_warp': (_I, [_P, _I, _P, _P, _P] + [_I] * 11 + [_P]),
    'mrdis_patch_blur_workspace': (_Z, [_I] * 5),
    'mrdis_patch_blur': (_I, [_P, _P, _P] + [_I] * 7 + [_P, _Z, _P]),
    'mrdis_patch_stats_workspace': (_Z, [_I] * 5),
    'mrdis_patch_stats': (_I, [_P, _P] + [_I] * 5 + [_P, _Z, _P]),
    'mrdis_patch_tone': (_I, [_P, _P, _P] + [_I] * 7 + [_P]),
    'mrdis_nvnet_loss_workspace': (_Z, [_L, _L]),
    'mrdis_nvnet_loss_fwd': (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _c.c_double, _P, _P, _P, _Z, _P]),
    'mrdis_nvnet_loss_bwd': (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _c.c_double, _P, _P, _P, _P, _P]),
    'mrdis_seg_counts': (_I, [_P, _P, _P, _I, _L, _I, _I, _P]),
    'mrdis_seg_accum': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_seg_label_volume': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_tile_accum': (_I, [_P, _P, _P, _P, _P] + [_I] * 12 + [_P]),
    'mrdis_tile_label_volume': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_synth_accum': (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_synth_finish': (_I, [_P, _P, _P, _I, _I, _I, _F, _P]),
    'mrdis_seg2d_label_planes': (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_seg2d_finish': (_I, [_P, _P, _I, _I, _I, _I, _P]),
    'mrdis_fuse_present_fwd': (_I, [_P, _P, _I, _P, _I, _P, _I, _I, _L, _I, _P]),
    'mrdis_fuse_present_bwd': (_I, [_P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _L, _I, _P]),
    'mrdis_region_surfaces': (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P]),
    'mrdis_edt_workspace': (_Z, [_I, _I, _I, _I, _I]),
    'mrdis_edt_sq': (_I, [_P, _c.c_char_p, _I, _P, _P, _Z, _I, _I, _I, _I, _P]),
    'mrdis_surface_hist': (_I, [_P, _I, _P, _L, _P, _Z, _I, _I, _I, _I, _P]),
    'mrdis_cc_label': (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _I, _P]),
    'mrdis_cc_clean_workspace': (_Z, [_I]),
    'mrdis_cc_clean': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _I, _I, _I, _I, _P]),
    'mrdis_region_planes': (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    'mrdis_dilate_workspace': (_Z, [_I, _I, _I, _I, _I]),
    'mrdis_dilate': (_I, [_P, _P, _I, _I, _P, _Z, _I, _I, _I, _I, _P]),
    'mrdis_lesion_match': (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_lesion_expand': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_maxpool_fwd': (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_maxpool_bwd': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_sumsq_workspace': (_Z, []),
    'mrdis_sumsq_finite': (_I, [_P, _L, _P, _P, _Z, _P]),
    'mrdis_adam_amsgrad_step': (_I, [_P, _P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _P, _P, _F, _F, _P, _P, _I, _P, _P, _I, _P]),
    'mrdis_conv3d_fwd': (_I, [_P, _I, _P, _P, _P, _I, _P, _I] + [_I] * 9 + [_P]),
    'mrdis_conv3d_bwd_data': (_I, [_P, _I, _P, _P, _I] + [_I] * 9 + [_P]),
    'mrdis_conv3d_bwd_weight_workspace': (_Z, [_I] * 9),
    'mrdis_conv3d_bwd_weight': (_I, [_P, _I, _P, _I, _P, _P, _P, _Z] + [_I] * 9 + [_P]),
    'mrdis_groupnorm_workspace': (_Z, [_I, _L, _I, _I]),
    'mrdis_groupnorm_relu_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _Z, _I, _L, _I, _I, _F, _I, _P]),
    'mrdis_groupnorm_relu_bwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _Z, _I, _L, _I, _I, _I, _P]),
    'mrdis_groupnorm_relu_bwd_add': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _Z, _I, _L, _I, _I, _I, _P]),
    'mrdis_upsample2x_add_fwd': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_upsample2x_bwd': (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_cosine_top1_workspace': (_Z, [_I, _I, _I]),
    'mrdis_cosine_top1': (_I, [_P, _L, _P, _I, _I, _P, _P, _I, _P, _P, _P, _Z, _P]),
    'mrdis_conv2d_2src_fwd': (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _I] + [_I] * 9 + [_P]),
    'mrdis_conv2d_2src_bwd_data': (_I, [_P, _I, _P, _P, _I, _I, _P, _I, _I] + [_I] * 8 + [_P]),
    'mrdis_conv2d_2src_bwd_weight_workspace': (_Z, [_I] * 10),
    'mrdis_conv2d_2src_bwd_weight': (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _P, _P, _I, _P, _Z] + [_I] * 8 + [_P]),
    'mrdis_softplus_fwd': (_I, [_P, _I, _P, _I, _L, _I, _P]),
    'mrdis_softplus_bwd': (_I, [_P, _I, _P, _I, _P, _I, _L, _I, _P]),
    'mrdis_softmax_fwd': (_I, [_P, _I, _P, _I, _L, _I, _P]),
    'mrdis_softmax_bwd': (_I, [_P, _I, _P, _I, _P, _I, _L, _I, _P]),
    'mrdis_kl_fwd': (_I, [_P, _P, _I, _I, _P, _P, _L, _I, _P, _P, _I, _I, _I, _P]),
    'mrdis_kl_bwd': (_I, [_P, _P, _P, _I, _I, _P, _P, _L, _I, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P]),
    'mrdis_avgpool_fwd': (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_avgpool_bwd': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'mrdis_chatt_workspace': (_Z, [_I, _L, _I, _I]),
    'mrdis_chatt_fwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _Z, _I, _L, _I, _I, _P]),
    'mrdis_chatt_bwd': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _Z, _I, _L, _I, _I, _P]),
    'mrdis_symdiff_fwd': (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_symdiff_bwd': (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_rgate_fwd': (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    'mrdis_rgate_bwd': (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    'mrdis_prep_workspace': (_Z, [_I, _I, _I]),
    'mrdis_prep_stats': (_I, [_P, _I, _L, _L, _L] + [_I] * 9 + [_c.c_double, _c.c_double, _P, _P, _Z, _P]),
    'mrdis_prep_write': (_I, [_P, _I, _L, _L, _L] + [_I] * 7 + [_c.c_double, _c.c_double, _P, _I, _I, _P, _P]),
    'mrdis_export_volume': (_I, [_P] + [_I] * 11 + [_P, _c.c_double, _P, _I, _P]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)


def load(path=None):
    """Load (once) and type the C-ABI library.  Raises MrdisLibraryError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise MrdisLibraryError(
            f'{path} not found: build it with `python __graft_entry__.py` / `make -C '
            f'{os.path.dirname(path)}`.  There is no CPU or eager fallback for the hot path.')
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError if the ABI drifted from include/mrdis.h
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _chk(rc, what):
    if rc != 0:
        raise MrdisError(f'{what}: {load().mrdis_strerror(rc).decode()} ({rc})')


def set_option(name, value):
    """process-wide kernel-selection switch (include/mrdis.h: "wino", "nt_mb", "debug_*")."""
    _chk(load().mrdis_set_option(name.encode(), int(value)), f'set_option({name})')


def get_option(name):
    return int(load().mrdis_get_option(name.encode()))


# every switch of csrc/mrdis_common.h MRDIS_OPTIONS (tests/test_abi.py checks that the library knows each name)
OPTION_NAMES = ('wino', 'nt_mb', 'wino_pipe', 'wino_u', 'wino4', 'wino4r', 'bconv4', 'split6', 'debug_no16', 'debug_nothin', 'debug_noc4', 'debug_nodma',
                'debug_no16_3d', 'debug_bilgen', 'debug_now16', 'debug_nopack', 'debug_mode', 'debug_bn', 'debug_kc', 'debug_bm', 'debug_c4_tw',
                'debug_wgsplit', 'debug_bn3', 'debug_kc3', 'c4_grid', 'debug_c4_blocks', 'zsearch_grid', 'debug_volgen')


def options_snapshot():
    """{name: value} of every process-wide switch; `options_restore(snap)` puts them back (tests/conftest.py does so around every test)."""
    return {n: get_option(n) for n in OPTION_NAMES}


def options_restore(snap):
    for n, v in snap.items():
        if get_option(n) != v:
            set_option(n, v)


KERNEL_FAMILIES = WINO_FAMILIES = ('wino', 'wino_spade', 'wino2', 'wino2_spade', 'wino4', 'wino4_spade', 'wino4n', 'wino4r', 'wino_wgrad', 'wino_wgrad2', 'wino4_wgrad', 'bconv3', 'bconv3_spade', 'bconv4', 'bconv4_spade',
                                   'split6_c4', 'split6_c16', 'split6_wgrad16', 'split6_co4', 'split6_c3d', 'split6_w3d', 'split6_tap',
                                   'bwgrad', 'bwgrad2', 'bwgrad3', 'bwgrad_s2',      # the bf16 weight gradients (csrc/mrdis_bf16.hip): bwgrad_kernel, its two pipelined forms, the stride-2 parity-class launch
                                   'all',        # 'all': every kernel launch of the library (bench.py: library_launches_per_step)
                                   'zsearch')    # mrdis_cosine_top1 (nearest-neighbour modality-code search)
# the kernels of the `others` variants (csrc/mrdis_encs.hip): the modality encoder's two-source first layer (mod_enc_s) and the anatomy
# activations (ana_dec_act).  Kept out of KERNEL_FAMILIES, whose every entry the convolution-path table must cover.
VARIANT_FAMILIES = ('conv2src', 'ana_act')
# the kernels of the latent-code options (csrc/mrdis_latent.hip): the masked KL term (lambda_kl, is_distri_z) and the mean compaction
# (s_compact_method 'mean').  Outside KERNEL_FAMILIES for the same reason.
LATENT_FAMILIES = ('kl', 'avgpool')
# the kernels of the attention output decoders 'U+SA+CA' / 'U+SSA+CA' (csrc/mrdis_outdec.hip): channel attention with the skip sum, the
# symmetric difference of the gate and the residual gate.  Outside KERNEL_FAMILIES for the same reason.
OUTDEC_FAMILIES = ('chatt', 'symdiff', 'rgate')
# the uncounted-until-now kernels of the 3-D convolutions (csrc/mrdis_conv3d.hip, mrdis_wino.hip): the tap-table direct kernel (tapconv3d_kernel),
# the 16-cout fp32 kernel (conv3d16_kernel), the generic and narrow weight gradients (wgrad3d_kernel, wgrad3d16_kernel; their reductions are not
# counted) and the hybrid Winograd weight gradient (one count per depth-tap launch, three per call).  The hybrid 3-D Winograd forward / data
# gradient keeps counting under 'wino_spade' and the six-product 3-D kernels under 'split6_c3d' / 'split6_w3d' (KERNEL_FAMILIES): renaming
# them would only churn the 2-D table.  Outside KERNEL_FAMILIES for the same reason as the tables above (tests/test_gpu_conv3d_paths.py covers them).
CONV3D_FAMILIES = ('direct3d', 'c3d16', 'wgrad3d', 'wgrad3d16', 'wino_wgrad3d')
# the 3-D batch gather (csrc/mrdis_volgather.hip): one count per mrdis_volume_gather call, whichever of its two kernels ran.
DATA_FAMILIES = ('volgather',)
# patch training for the 3-D nets (csrc/mrdis_patch.hip; the wrappers live in patch3d.py): one count per mrdis_fg_block_counts call (once per
# subject), per mrdis_patch_origins call (one per batch) and per mrdis_patch_gather call (two per batch: inputs and targets).
PATCH_FAMILIES = ('fgcount', 'patchorigin', 'patchgather')
PATCH_MAX_CLASSES = 8             # include/mrdis.h MRDIS_PATCH_MAX_CLASSES
# rotated and zoomed training patches (csrc/mrdis_warp.hip; the wrapper lives in warp3d.py): one count, and one launch, per mrdis_patch_warp call
# (two per batch of a loader with patch_warp > 0, in place of the two 'patchgather').
WARP_FAMILIES = ('patchwarp',)
# intensity augmentation of the training patches (csrc/mrdis_tone.hip; the wrappers live in tone3d.py): one count per mrdis_patch_blur /
# mrdis_patch_stats / mrdis_patch_tone call (one each per batch of a loader with a patch_blur / _contrast / _gamma / _noise share above 0).
TONE_FAMILIES = ('patchblur', 'patchstats', 'patchtone')
# the fused objective of the 3-D nets and the segmentation counts (csrc/mrdis_loss3d.hip): 'loss3d' counts one per mrdis_nvnet_loss_fwd and one per
# mrdis_nvnet_loss_bwd call, 'segcounts' one per mrdis_seg_counts call.
LOSS3D_FAMILIES = ('loss3d', 'segcounts')
# whole-volume sliding-window prediction (csrc/mrdis_segvol.hip): 'segaccum' counts one per mrdis_seg_accum call (one per window and flip),
# 'seglabels' one per mrdis_seg_label_volume call (one per batch).
SEGVOL_FAMILIES = ('segaccum', 'seglabels')
# tile-wise prediction (csrc/mrdis_segvol.hip; model3d.predict_tiles): 'tileaccum' counts one per mrdis_tile_accum call (one per tile and view),
# 'tilelabels' one per mrdis_tile_label_volume call (one per batch).
TILEPRED_FAMILIES = ('tileaccum', 'tilelabels')
TILE_FLIPS = 1 | 4 | 8            # the flip bits mrdis_tile_accum takes: h | w | d, the gather table's (patch3d.FLIP_H | FLIP_W | FLIP_D)
# whole-subject synthesis of missing contrasts by the 2-D model (csrc/mrdis_synth.hip): 'synthaccum' counts one per mrdis_synth_accum call (one per
# batch and target), 'synthfinish' one per mrdis_synth_finish call (one per target).
SYNTH_FAMILIES = ('synthaccum', 'synthfinish')
# whole-subject segmentation by the 2-D model per missing-contrast pattern (csrc/mrdis_seg2d.hip): 'seg2dlabels' counts one per
# mrdis_seg2d_label_planes call (one per batch, whatever the number of patterns), 'seg2dfinish' one per mrdis_seg2d_finish call (one per subject).
SEG2D_FAMILIES = ('seg2dlabels', 'seg2dfinish')
# the fusion of the anatomy maps over the contrasts a sample has (csrc/mrdis_fuse.hip; lambda_recon_y_fused): 'fuse' counts one per
# mrdis_fuse_present_fwd and one per mrdis_fuse_present_bwd call.  Outside KERNEL_FAMILIES for the same reason as the tables above.
FUSE_FAMILIES = ('fuse',)
# region scoring of label volumes (csrc/mrdis_surfdist.hip): 'regsurf' counts one per mrdis_region_surfaces call, 'edt' one per LAUNCH of a
# distance-transform pass (three per mrdis_edt_sq call, two per mrdis_surface_hist call), 'surfhist' one per mrdis_surface_hist call (its last
# pass, which adds into the histogram instead of storing distances).  None depends on the batch size.
SURFDIST_FAMILIES = ('regsurf', 'edt', 'surfhist')
# connected components of label volumes and their clean-up (csrc/mrdis_cc.hip): 'cclabel' counts one per LAUNCH of a labelling pass (three per
# mrdis_cc_label call, whatever B, shape and content), 'ccclean' one per mrdis_cc_clean call.
CC_FAMILIES = ('cclabel', 'ccclean')
# lesion-wise scoring (csrc/mrdis_lesion.hip): 'dilate' counts one per LAUNCH of mrdis_region_planes (one) and mrdis_dilate (one per iteration),
# 'lesmatch' one per mrdis_lesion_match call, 'lesexpand' one per mrdis_lesion_expand call.
LESION_FAMILIES = ('dilate', 'lesmatch', 'lesexpand')
# preprocessing of raw scans into store volumes (csrc/mrdis_prep.hip): 'prepstats' counts one per mrdis_prep_stats call (four launches),
# 'prepwrite' one per mrdis_prep_write call.
PREP_FAMILIES = ('prepstats', 'prepwrite')
# store volumes back to a NIfTI file's order and canvas (csrc/mrdis_export.hip): one count, and one launch, per mrdis_export_volume call.
EXPORT_FAMILIES = ('export',)
# the dispatch choices of the statistics, norm and resize entry points (csrc/mrdis_elem.hip), host-side counts only: which partial-sum kernel a
# statistics pass took ('stat_vec' | 'stat_scalar' | 'stat_interp': one per pass), the route of mrdis_instnorm_spade_bwd_up2 (one per call), the
# kernel of mrdis_bilinear_fwd / _bwd (one per call), and 'elem_v1': an element-wise pass that took its one-channel-per-thread instantiation (also, once per call, the chatt / symdiff / rgate
# entry points of csrc/mrdis_outdec.hip in their scalar forms; tests/test_gpu_attn_paths.py).
# Outside KERNEL_FAMILIES for the same reason as the tables above (tests/test_gpu_elem_paths.py covers them).
ELEM_FAMILIES = ('stat_vec', 'stat_scalar', 'stat_interp', 'spade_up2_onepass', 'spade_up2_twopass', 'bil_fwd_x2', 'bil_fwd_general',
                 'bil_bwd_x2', 'bil_bwd_tight3', 'bil_bwd_tight5', 'bil_bwd_general', 'elem_v1')
# every name of csrc/mrdis_common.h MRDIS_COUNTERS: what launch_counts() hands out, ELEM_FAMILIES on request (tests/test_abi.py pins the union)
LAUNCH_COUNTERS = (WINO_FAMILIES + VARIANT_FAMILIES + LATENT_FAMILIES + OUTDEC_FAMILIES + CONV3D_FAMILIES + DATA_FAMILIES + PATCH_FAMILIES + WARP_FAMILIES + TONE_FAMILIES + LOSS3D_FAMILIES + SEGVOL_FAMILIES + TILEPRED_FAMILIES
                    + SYNTH_FAMILIES + SEG2D_FAMILIES + FUSE_FAMILIES + SURFDIST_FAMILIES + CC_FAMILIES + PREP_FAMILIES + EXPORT_FAMILIES + LESION_FAMILIES)
ALL_COUNTERS = LAUNCH_COUNTERS + ELEM_FAMILIES
SYNTH_MAX_SRC = 8                 # include/mrdis.h MRDIS_SYNTH_MAX_SRC
SEG2D_MAX_SETS = 16               # include/mrdis.h MRDIS_SEG2D_MAX_SETS
SEG2D_MAX_VIEWS = 2               # include/mrdis.h MRDIS_SEG2D_MAX_VIEWS
SEG2D_FLIPS = {'': 0, 'h': 1, 'w': 2}      # the flip codes of mrdis_seg2d_label_planes
FUSE_MAX_SRC = 8                  # include/mrdis.h MRDIS_FUSE_MAX_SRC
FUSE_METHODS = ('mean', 'max', 'mean-max-min')      # MRDIS_FUSE_MEAN | _MAX | _MEAN_MAX_MIN, in this order
EDT_FAR = 1 << 30                 # include/mrdis.h MRDIS_EDT_FAR
EDT_MAX_SRC = 8                   # include/mrdis.h MRDIS_EDT_MAX_SRC
EDT_MAX_EXTENT = 1024             # each of H, W, D of a distance transform
SURF_MAX_REGIONS = 4              # include/mrdis.h MRDIS_SURF_MAX_REGIONS
CC_MAX_EXTENT = 1024              # each of H, W, D of a connected-component labelling
CC_LABEL_LAUNCHES = 3             # kernel launches of one mrdis_cc_label call
CC_CONNECTIVITIES = (6, 18, 26)
DILATE_MAX_ITERATIONS = 8         # include/mrdis.h MRDIS_DILATE_MAX_ITERATIONS


def stream_fill(t, value=0.0):
    """store-only probe over a dense fp32 tensor (include/mrdis.h mrdis_stream_fill)"""
    if (t.dtype is not torch.float32 or t.numel() % 4 != 0
            or not (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last))): _refuse('stream_fill', 'vec dtype dense', t)
    _chk(load().mrdis_stream_fill(t.data_ptr(), t.numel(), float(value), _stream()), 'stream_fill')
    return t


def dynamic_lds():
    """{kernel family: largest dynamic LDS bytes it was launched with in this process} (include/mrdis.h mrdis_dynamic_lds_table; template arguments folded)"""
    import re
    buf = _c.create_string_buffer(16384)
    load().mrdis_dynamic_lds_table(buf, 16384)
    out = {}
    for line in buf.value.decode().splitlines():
        expr, _, b = line.rpartition('=')
        if not expr or not b.isdigit():        # (the library only hands out whole lines; never let a diagnostic take the caller down)
            continue
        name = re.sub(r'<.*', '', expr.strip().lstrip('(')).strip()
        out[name] = max(out.get(name, 0), int(b))
    return out


def launch_counts(reset=False, elem=False):
    """{family: launches since load / the last reset} of the Winograd, bf16 LDS-DMA and six-product (split6) kernel families (include/mrdis.h mrdis_launch_count).
    elem=True adds ELEM_FAMILIES: they count dispatch choices of passes that run beside almost every counted kernel (the statistics in front of a fused
    SPADE convolution, say), so callers that assert "this family and no other" over the whole dictionary only see them when they ask."""
    lib = load()
    out = {f: int(lib.mrdis_launch_count(f.encode())) for f in (ALL_COUNTERS if elem else LAUNCH_COUNTERS)}
    if reset:
        lib.mrdis_launch_count_reset()
    return out


class option:
    """`with hip.option('wino', 0): ...` -- set a switch for a scope (tests, A/B timing)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = get_option(self.name)
        set_option(self.name, self.value)

    def __exit__(self, *exc):
        set_option(self.name, self.prev)


_DEV_INDEX = None


def _stream():
    """raw hipStream_t of torch's CURRENT stream on this process's device (one process per GPU).  `torch.cuda.current_stream()`
    costs ~9 us of Python per call (2,000 calls per step); the raw query is a C call."""
    global _DEV_INDEX
    if _DEV_INDEX is None:
        _DEV_INDEX = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(_DEV_INDEX)


def _ptr(t):
    return None if t is None else t.data_ptr()


_WS = {}          # (device, raw stream) -> grow-only scratch buffer


def _ws(nbytes, device):
    """Scratch memory of one call.  Every kernel that uses it runs on the current stream, so consecutive calls can share ONE buffer per
    (device, stream): stream order keeps them apart, and no caller keeps workspace contents beyond its own launches.  (A fresh
    torch.empty per call was ~1,000 allocator round trips per training step.)"""
    n = max(int(nbytes), 16)
    key = (device, _stream())
    buf = _WS.get(key)
    if buf is None or buf.numel() < n:
        size = max(n, 1 << 20) if buf is None else max(n, 2 * buf.numel())
        buf = _WS[key] = torch.empty(size, dtype=torch.uint8, device=device)
    return buf


_WS_BYTES = {}    # (entry point, geometry) -> workspace bytes: the queries are pure functions of their arguments


def _ws_bytes(fn, *args):
    key = (fn.__name__, args)
    v = _WS_BYTES.get(key)
    if v is None:
        v = _WS_BYTES[key] = fn(*args)
    return v


# ---------------------------------------------------------------- NHWC views
def nhwc(t):
    """(tensor, ld) for a logical (N,C,H,W) fp32 or bf16 tensor whose memory is NHWC with pixel
    stride ld in elements (channels_last tensors and channel slices of them qualify as they are)."""
    if t.dim() != 4 or not (t.dtype is torch.float32 or t.dtype is torch.bfloat16): _refuse('nhwc', 'dtype', t)
    if t.is_contiguous(memory_format=torch.channels_last) and t.shape[1] > 1 and t.shape[3] > 1:
        return t, t.shape[1]                         # the common case: a dense channels_last tensor
    N, C, H, W = t.shape
    s = t.stride()
    ld = s[3] if W > 1 else (s[2] if H > 1 else (s[0] if N > 1 else C))
    ok = (ld >= C and (C == 1 or s[1] == 1) and (W == 1 or s[3] == ld) and
          (H == 1 or s[2] == W * ld) and (N == 1 or s[0] == H * W * ld))
    if not ok:
        t = t.contiguous(memory_format=torch.channels_last)
        if t.stride()[1] != 1 and C > 1:      # degenerate shapes: force a real NHWC copy
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        ld = C
    return t, ld


def empty_nhwc(N, C, H, W, device, dtype=torch.float32):
    return torch.empty((N, C, H, W), dtype=dtype, device=device, memory_format=torch.channels_last)


def _dt(*tensors):
    """MRDIS_DT_* storage code of a set of activation views (all fp32 or all bf16)."""
    kind = None
    for t in tensors:
        if t is None:
            continue
        d = t.dtype
        if kind is None:
            kind = d
        elif d is not kind:
            raise MrdisError(f'activation views must be all fp32 or all bf16, got {kind} and {d}')
    if kind is torch.float32:
        return 0
    if kind is torch.bfloat16:
        return 2
    raise MrdisError(f'activation views must be fp32 or bf16, got {kind}')


# ---------------------------------------------------------------- what a wrapper establishes before a library call
# DESIGN.md "The binding's contract": hot wrappers (a training step's) check inline, without device compares; the cold ones through the helpers below.
_CLAIMS = {'like': 'operands of one shape', 'layer': 'the shape the layer\'s kernel, stride and padding make of the input', 'filter': 'a (taps, reduce, out) filter for the layer',
           'out': 'an output view of the result\'s shape, written in place', 'vec': 'vectors, tables and buffers of the element count the shapes and integers imply',
           'dtype': 'the dtype the entry point reads', 'dense': 'dense memory (contiguous, NHWC or NDHWC as documented)', 'arg': 'arguments in their documented range'}


def _refuse(what, claims, *ts):
    """the failure path of every inline check: MrdisError naming the wrapper, the claims (keys of _CLAIMS) of which the call breaks one, and the operands"""
    raise MrdisError(f'{what} wants ' + '; '.join(_CLAIMS[c] for c in claims.split()) + ', ' + _got(*ts))


def _got(*ts):
    """the operands of a refused call, for its message"""
    return 'got ' + ', '.join(f'{t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}' if isinstance(t, torch.Tensor) else repr(t) for t in ts)


def _want(t, what, dtype, shape=None, device=None, cl=False, dense=True):
    """tuple(t.shape) of a contiguous tensor of that dtype, and of that shape (a name stands for any extent) and device where given, else MrdisError.
    cl: dense channels-last / channels-last-3d memory instead of contiguous; dense=False: any strides (the caller copies)."""
    ok = isinstance(t, torch.Tensor) and t.dtype is dtype and (device is None or t.device == device)
    if ok and shape is not None:
        ok = t.dim() == len(shape) and all(isinstance(w, str) or w == n for w, n in zip(shape, t.shape))
    if not (ok and (not dense or (t.movedim(1, -1) if cl else t).is_contiguous())):
        claim = ' '.join(str(v) for v in (dtype, shape) if v is not None) + (' tensor' if device is None else f' tensor on {device}')
        raise MrdisError(f'{what} must be a {"dense channels-last" if cl else "contiguous"} {claim}, {_got(t)}')
    return tuple(t.shape)


def _crop(crop, what):
    """(h0, h1, w0, w1) of crop = ((h0, h1), (w0, w1))"""
    try:
        (h0, h1), (w0, w1) = [[int(v) for v in c] for c in crop]
    except (TypeError, ValueError):
        raise MrdisError(f'{what}: crop {crop!r}: ((h0, h1), (w0, w1))') from None
    return h0, h1, w0, w1


class _Mailbox:
    """Small host -> device transfers by a KERNEL that reads pinned host memory (mrdis_copy_bytes) instead of hipMemcpyAsync:
    a ring of pinned slots; a slot is rewritten only after the event recorded behind its last copy kernel has completed."""
    SLOT = 1 << 16          # bytes per slot = the largest tensor that goes through the mailbox
    NSLOT = 64

    def __init__(self):
        self.buf = torch.empty(self.SLOT * self.NSLOT, dtype=torch.uint8).pin_memory()
        self.events = [None] * self.NSLOT
        self.next = 0

    def send(self, t_cpu, device):
        nbytes = t_cpu.numel() * t_cpu.element_size()
        k = self.next
        self.next = (k + 1) % self.NSLOT
        ev = self.events[k]
        if ev is not None:
            ev.synchronize()                           # 64 transfers ago: long done unless the host is a whole ring ahead of the GPU
        slot = self.buf[k * self.SLOT:k * self.SLOT + nbytes]
        slot.copy_(t_cpu.contiguous().view(-1).view(torch.uint8))
        out = torch.empty(t_cpu.shape, dtype=t_cpu.dtype, device=device)
        _chk(load().mrdis_copy_bytes(slot.data_ptr(), _ptr(out), nbytes, _stream()), 'copy_bytes')
        if ev is None:
            ev = self.events[k] = torch.cuda.Event()
        ev.record()
        return out


_mailbox = None


def copy_bytes(src, dst, nbytes):
    """word-wise copy by a kernel on the current stream (include/mrdis.h mrdis_copy_bytes); src may be a PINNED host tensor"""
    if (nbytes % 4 != 0 or not 0 <= nbytes <= min(src.numel() * src.element_size(), dst.numel() * dst.element_size())
            or not (src.is_contiguous() and dst.is_contiguous())): _refuse('copy_bytes', 'vec dense', src, dst)
    _chk(load().mrdis_copy_bytes(src.data_ptr(), _ptr(dst), int(nbytes), _stream()), 'copy_bytes')


def to_device_small(t_cpu, device):
    """CPU tensor (<= 64 KB, element size 4 or 8) -> new device tensor, stream-ordered, without the copy engine; None if it does not qualify."""
    global _mailbox
    nbytes = t_cpu.numel() * t_cpu.element_size()
    if nbytes == 0 or nbytes > _Mailbox.SLOT or nbytes % 4 != 0 or t_cpu.dtype in (torch.bool,):
        return None
    if _mailbox is None:
        _mailbox = _Mailbox()
    return _mailbox.send(t_cpu, device)


class MixJob(_c.Structure):
    """csrc/mrdis_conv.hip `MixJob`: one CondConv2d layer (or one half of a fused gamma | beta pair) of the all-layers mixing launches."""
    _fields_ = [('W', _c.c_void_p), ('fcw', _c.c_void_p), ('fcb', _c.c_void_p), ('r', _c.c_void_p),
                ('tck', _c.c_void_p * 8), ('tkc', _c.c_void_p * 8), ('btck', _c.c_void_p * 8), ('btkc', _c.c_void_p * 8),
                ('dW', _c.c_void_p), ('dfcw', _c.c_void_p), ('dfcb', _c.c_void_p), ('part', _c.c_void_p),
                ('tap_tkc', _c.c_longlong),
                ('E', _c.c_int), ('Co', _c.c_int), ('Ci', _c.c_int), ('T', _c.c_int), ('ld_tck', _c.c_int), ('ld_dw', _c.c_int),
                ('block0', _c.c_int), ('nblk', _c.c_int), ('accumulate', _c.c_int), ('ci_pitch', _c.c_int)]


class WinoUJob(_c.Structure):
    """csrc/mrdis_wino2.hip `WinoUJob`: one (filter, role) of the Winograd filter-image launch (include/mrdis.h)."""
    _fields_ = [('w', _c.c_void_p), ('img', _c.c_void_p), ('R', _c.c_int), ('S', _c.c_int), ('flip', _c.c_int), ('spadeC', _c.c_int),
                ('block0', _c.c_int), ('nblk', _c.c_int), ('fmt', _c.c_int), ('pad_', _c.c_int)]


def wino_u_format(R, S, spadeC=0):
    """2: the F(2x2,3x3) image (csrc/mrdis_wino2.hip), 4: the F(4x4,3x3) image (csrc/mrdis_wino4.hip) -- a function of the filter's shape and
    the option 'wino4' alone, so the image built once per step fits every call of the layer."""
    return int(load().mrdis_wino_u_format(R, S, spadeC))


def _struct_table(jobs, struct, lib_bytes, device):
    """list of ctypes structs -> device tensor holding the table (checked against the library's struct size)"""
    nb = _c.sizeof(struct)
    if nb != lib_bytes:
        raise MrdisError(f'{struct.__name__} layout mismatch: binding {nb} bytes, library {lib_bytes}')
    arr = (struct * len(jobs))(*jobs)
    return torch.frombuffer(bytearray(_c.string_at(_c.addressof(arr), nb * len(jobs))), dtype=torch.uint8).to(device)


def wino_u_table(jobs, device):
    for j in jobs:
        if not j.fmt:                              # a caller may pin the format (MixPlan records the one it sized the image for)
            j.fmt = wino_u_format(j.R, j.S, j.spadeC)
    return _struct_table(jobs, WinoUJob, load().mrdis_wino_u_job_bytes(), device)


def wino_u_image_floats(R, S, spadeC=0, fmt=None):
    """floats of the filter image in format `fmt` (default: the format an image built NOW gets); -1 if that shape never has the format"""
    if fmt is None:
        return int(load().mrdis_wino_u_image_floats(R, S, spadeC))
    return int(load().mrdis_wino_u_image_floats_fmt(R, S, spadeC, fmt))


S6_IMAGE_FMT = 6


def s6_filter_image_bytes(taps, Cred, Cout):
    return int(load().mrdis_s6_filter_image_bytes(int(taps), int(Cred), int(Cout)))


def s6_filter_image(w):
    """w [taps][Cred][Cout] fp32 (w_tck for the forward pass, w_tkc for the data gradient) -> its six-product image (mrdis_s6conv.hip), a float32-typed
    tensor that travels in the auxiliary-filter slot of conv2d_fwd / conv2d_bwd_data (attribute mrdis_fmt = 6); None where the layer has no such image."""
    if w.dim() != 3: _refuse('s6_filter_image', 'filter', w)
    T, R, S = w.shape
    nb = s6_filter_image_bytes(T, R, S)
    if nb == 0 or nb >= 2 ** 31 or w.dtype is not torch.float32:
        return None
    w = w.contiguous()
    img = torch.empty(nb // 4, dtype=torch.float32, device=w.device)
    _chk(load().mrdis_s6_filter_image(_ptr(w), T, R, S, _ptr(img), nb, _stream()), 's6_filter_image')
    img.mrdis_fmt = S6_IMAGE_FMT
    return img


def wino_image_fmt(img, R, S, spadeC=0, taps=0):
    """The format a Winograd filter image was BUILT in: it travels with the image (attribute `mrdis_fmt`, set by whoever built it) and goes to
    the library beside the pointer -- never re-derived from the current value of the option 'wino4', which may have changed since.  Images
    without the attribute (tests, tools) are recognised by their size, which differs between the formats of one filter shape."""
    fmt = getattr(img, 'mrdis_fmt', None)
    n = img.numel()
    if fmt == S6_IMAGE_FMT or (fmt is None and taps and s6_filter_image_bytes(taps, R, S) == 4 * n):
        if s6_filter_image_bytes(taps, R, S) != 4 * n:
            raise MrdisError(f'six-product image of {4 * n} bytes, a [{taps}][{R}][{S}] filter needs {s6_filter_image_bytes(taps, R, S)}')
        return S6_IMAGE_FMT
    if fmt is None:
        hits = [f for f in (2, 4, 5) if wino_u_image_floats(R, S, spadeC, f) == n]
        if len(hits) != 1:
            raise MrdisError(f'Winograd image of {n} floats fits no single format of a [9][{R}][{S}] filter (spadeC {spadeC}): candidates {hits}')
        fmt = hits[0]
    elif wino_u_image_floats(R, S, spadeC, fmt) != n:
        raise MrdisError(f'Winograd image tagged format {fmt} has {n} floats, a [9][{R}][{S}] filter (spadeC {spadeC}) needs {wino_u_image_floats(R, S, spadeC, fmt)}')
    return fmt


def _image_fmt(img, R, S, taps, kh, kw, what, spadeC=0):
    """format code of the filter image in a convolution's auxiliary slot (0: none), which must be fp32, dense, and of the size its format has for the filter"""
    if img is None:
        return 0
    if img.dtype is not torch.float32 or not img.is_contiguous(): _refuse(what, 'filter dtype dense', img)
    fmt = wino_image_fmt(img, R, S, spadeC, taps)
    if fmt != S6_IMAGE_FMT and (kh, kw) != (3, 3): _refuse(f'{what}: a Winograd image (format {fmt}) goes with a 3x3 filter, not {kh}x{kw}', 'arg', img)
    return fmt


def wino_u_job_blocks(R, S, spadeC=0):
    return int(load().mrdis_wino_u_job_blocks(R, S, spadeC))


def _job_table(table, njobs, job, what, types=None):
    """a device table of `njobs` structs as wino_u_table / mix_job_table built it and, for the mixing launches, their dense fp32 (M, emb) type rows"""
    if table.dtype is not torch.uint8 or not table.is_contiguous() or not 1 <= njobs <= table.numel() // _c.sizeof(job): _refuse(what, 'vec dtype dense', table, njobs)
    if types is not None and (types.dtype is not torch.float32 or types.dim() != 2 or not types.is_contiguous()): _refuse(what, 'dtype dense', types)


def wino_u_jobs(table, njobs, total_blocks):
    _job_table(table, njobs, WinoUJob, 'wino_u_jobs')
    _chk(load().mrdis_wino_u_jobs(_ptr(table), njobs, total_blocks, _stream()), 'wino_u_jobs')


def mix_job_table(jobs, device):
    """list of MixJob -> device tensor holding the table (checked against the library's struct size)."""
    return _struct_table(jobs, MixJob, load().mrdis_mix_job_bytes(), device)


def mix_job_blocks(Co, Ci, T):
    return int(load().mrdis_mix_job_blocks(Co, Ci, T))


def mix_jobs_fwd(table, njobs, total_blocks, types):
    _job_table(table, njobs, MixJob, 'mix_jobs_fwd', types)
    M, emb = types.shape
    _chk(load().mrdis_mix_jobs_fwd(_ptr(table), njobs, total_blocks, _ptr(types), emb, M, _stream()), 'mix_jobs_fwd')


def mix_jobs_bwd(table, njobs, total_blocks, dw_table, types):
    _job_table(table, njobs, MixJob, 'mix_jobs_bwd', types)
    M, emb = types.shape
    if not dw_table.is_contiguous() or dw_table.numel() * dw_table.element_size() < njobs * 64: _refuse('mix_jobs_bwd', 'vec dense', dw_table)      # [njobs][8] addresses
    _chk(load().mrdis_mix_jobs_bwd(_ptr(table), njobs, total_blocks, _ptr(dw_table), _ptr(types), emb, M, _stream()), 'mix_jobs_bwd')


def cast_view(x, dtype, channels=None):
    """NHWC view -> new NHWC tensor of storage type `dtype` (fp32 / bf16, round to nearest even) with `channels` channels
    (default: unchanged): the first min(C, channels) are copied, a wider result is zero-padded."""
    lib = load()
    x, ldx = nhwc(x)
    N, C, H, W = x.shape
    Cd = C if channels is None else int(channels)
    if x.dtype == dtype and Cd == C:
        return x
    y = empty_nhwc(N, Cd, H, W, x.device, dtype)
    _chk(lib.mrdis_cast_view(_ptr(x), ldx, _dt(x), C, _ptr(y), Cd, _dt(y), Cd, N * H * W, _stream()), 'cast_view')
    return y


def bconv_eligible(c_reduce, c_out):
    """geometry the bf16 MFMA convolution kernels cover (csrc/mrdis_bf16.hip): reduction axis % 16, >= 16 outputs, % 4."""
    return c_reduce % 16 == 0 and c_out % 4 == 0 and c_out >= 16


# ---------------------------------------------------------------- expert mixing
def mix_experts_fwd(W, r):
    """W (E,Co,Ci,kh,kw), r (E) -> (w_tck [T,Ci,Co], w_tkc [T,Co,Ci])."""
    lib = load()
    E, Co, Ci, kh, kw = W.shape
    T = kh * kw
    if W.dtype is not torch.float32 or r.dtype is not torch.float32 or r.numel() != E: _refuse('mix_experts_fwd', 'vec dtype', W, r)
    W = W.contiguous(); r = r.contiguous()
    w_tck = torch.empty((T, Ci, Co), dtype=torch.float32, device=W.device)
    w_tkc = torch.empty((T, Co, Ci), dtype=torch.float32, device=W.device)
    _chk(lib.mrdis_mix_experts_fwd(_ptr(W), _ptr(r), _ptr(w_tck), _ptr(w_tkc), E, Co, Ci, T, _stream()), 'mix_experts_fwd')
    return w_tck, w_tkc


def mix_experts_bwd(dw_tck, W, r):
    lib = load()
    E, Co, Ci, kh, kw = W.shape
    T = kh * kw
    if (not (W.dtype is r.dtype is dw_tck.dtype is torch.float32)
            or r.numel() != E or dw_tck.numel() != T * Ci * Co): _refuse('mix_experts_bwd', 'vec dtype', dw_tck, W, r)
    W = W.contiguous(); r = r.contiguous(); dw_tck = dw_tck.contiguous()
    dW = torch.empty_like(W)
    dr = torch.zeros(E, dtype=torch.float32, device=W.device)
    nb = _ws_bytes(lib.mrdis_mix_experts_bwd_workspace, E, Co, Ci, T)
    ws = _ws(nb, W.device)
    _chk(lib.mrdis_mix_experts_bwd(_ptr(dw_tck), _ptr(W), _ptr(r), _ptr(dW), _ptr(dr), _ptr(ws), nb, E, Co, Ci, T, _stream()),
         'mix_experts_bwd')
    return dW, dr


def mix_experts_routed_fwd(W, fcw, fcb, t_row):
    """W (E,Co,Ci,kh,kw), routing Linear (fcw (E,emb), fcb (E)), t_row (1,emb) -> (w_tck, w_tkc, r)."""
    lib = load()
    E, Co, Ci, kh, kw = W.shape
    T = kh * kw
    emb = fcw.shape[-1]
    if (not (W.dtype is fcw.dtype is fcb.dtype is t_row.dtype is torch.float32)
            or tuple(fcw.shape) != (E, emb) or fcb.numel() != E or t_row.numel() != emb): _refuse('mix_experts_routed_fwd', 'dtype', W, fcw, fcb, t_row)
    W = W.contiguous(); fcw = fcw.contiguous(); fcb = fcb.contiguous(); t_row = t_row.contiguous()
    w_tck = torch.empty((T, Ci, Co), dtype=torch.float32, device=W.device)
    w_tkc = torch.empty((T, Co, Ci), dtype=torch.float32, device=W.device)
    r = torch.empty(E, dtype=torch.float32, device=W.device)
    _chk(lib.mrdis_mix_experts_routed_fwd(_ptr(W), _ptr(fcw), _ptr(fcb), _ptr(t_row), emb, _ptr(r), _ptr(w_tck), _ptr(w_tkc),
                                          E, Co, Ci, T, _stream()), 'mix_experts_routed_fwd')
    return w_tck, w_tkc, r


def mix_experts_routed_bwd(dw_tck, W, r, t_row, emb):
    lib = load()
    E, Co, Ci, kh, kw = W.shape
    T = kh * kw
    if (not (W.dtype is r.dtype is dw_tck.dtype is t_row.dtype is torch.float32) or r.numel() != E
            or dw_tck.numel() != T * Ci * Co or t_row.numel() != emb): _refuse('mix_experts_routed_bwd', 'vec dtype', dw_tck, W, r, t_row)
    W = W.contiguous(); dw_tck = dw_tck.contiguous(); t_row = t_row.contiguous(); r = r.contiguous()
    dW = torch.empty_like(W)
    dfcw = torch.empty((E, emb), dtype=torch.float32, device=W.device)
    dfcb = torch.empty(E, dtype=torch.float32, device=W.device)
    nb = _ws_bytes(lib.mrdis_mix_experts_bwd_workspace, E, Co, Ci, T)
    ws = _ws(nb, W.device)
    _chk(lib.mrdis_mix_experts_routed_bwd(_ptr(dw_tck), _ptr(W), _ptr(r), _ptr(t_row), emb, _ptr(dW), _ptr(dfcw), _ptr(dfcb),
                                          _ptr(ws), nb, E, Co, Ci, T, _stream()), 'mix_experts_routed_bwd')
    return dW, dfcw, dfcb


def mix_experts_routed_multi_fwd(W, fcw, fcb, types, want_bf16=False, into=None):
    """all M type rows at once: -> ([w_tck_m], [w_tkc_m], r (M,E)); want_bf16: + ([bf16(w_tck_m)], [bf16(w_tkc_m)]) from the same launch.
    into = (tck, tkc, btck, btkc, col0, co_total): write into column block [col0, col0 + Co) of existing WIDER filters (lists of M tensors
    (T, Ci, co_total) / (T, co_total, Ci); btck / btkc None or the bf16 twins) -- the halves of a fused gamma | beta filter; -> r only."""
    lib = load()
    E, Co, Ci, kh, kw = W.shape
    T = kh * kw
    if (not (W.dtype is fcw.dtype is fcb.dtype is types.dtype is torch.float32)
            or types.dim() != 2 or tuple(fcw.shape) != (E, types.shape[1]) or fcb.numel() != E): _refuse('mix_experts_routed_multi_fwd', 'dtype', W, fcw, fcb, types)
    W = W.contiguous(); fcw = fcw.contiguous(); fcb = fcb.contiguous(); types = types.contiguous()
    M, emb = types.shape
    r = torch.empty((M, E), dtype=torch.float32, device=W.device)
    if into is not None:
        tck, tkc, btck, btkc, col0, cot = into
        for ts, dtype, shape in ((tck, torch.float32, (T, Ci, cot)), (tkc, torch.float32, (T, cot, Ci)), (btck, torch.bfloat16, (T, Ci, cot)), (btkc, torch.bfloat16, (T, cot, Ci))):
            if ts is None and dtype is torch.bfloat16 and btck is None:
                continue
            if (ts is None or not 0 <= col0 <= cot - Co or len(ts) != M
                    or any(t.dtype is not dtype or tuple(t.shape) != shape or not t.is_contiguous() for t in ts)): _refuse('mix_experts_routed_multi_fwd', 'filter dtype dense arg', *(ts or ()))
        a = (_c.c_void_p * M)(*[t.data_ptr() + 4 * col0 for t in tck]); b = (_c.c_void_p * M)(*[t.data_ptr() + 4 * col0 * Ci for t in tkc])
        ba = bb = None
        if btck is not None:
            ba = (_c.c_void_p * M)(*[t.data_ptr() + 2 * col0 for t in btck]); bb = (_c.c_void_p * M)(*[t.data_ptr() + 2 * col0 * Ci for t in btkc])
        _chk(lib.mrdis_mix_experts_routed_multi_fwd(_ptr(W), _ptr(fcw), _ptr(fcb), _ptr(types), emb, M, _ptr(r), a, b, ba, bb, cot, cot * Ci,
                                                    E, Co, Ci, T, _stream()), 'mix_experts_routed_multi_fwd')
        return r
    tck = [torch.empty((T, Ci, Co), dtype=torch.float32, device=W.device) for _ in range(M)]
    tkc = [torch.empty((T, Co, Ci), dtype=torch.float32, device=W.device) for _ in range(M)]
    a = (_c.c_void_p * M)(*[t.data_ptr() for t in tck]); b = (_c.c_void_p * M)(*[t.data_ptr() for t in tkc])
    ba = bb = None
    if want_bf16:
        btck = [torch.empty((T, Ci, Co), dtype=torch.bfloat16, device=W.device) for _ in range(M)]
        btkc = [torch.empty((T, Co, Ci), dtype=torch.bfloat16, device=W.device) for _ in range(M)]
        ba = (_c.c_void_p * M)(*[t.data_ptr() for t in btck]); bb = (_c.c_void_p * M)(*[t.data_ptr() for t in btkc])
    _chk(lib.mrdis_mix_experts_routed_multi_fwd(_ptr(W), _ptr(fcw), _ptr(fcb), _ptr(types), emb, M, _ptr(r), a, b, ba, bb, 0, 0, E, Co, Ci, T, _stream()),
         'mix_experts_routed_multi_fwd')
    if want_bf16:
        return tck, tkc, r, btck, btkc
    return tck, tkc, r


def mix_experts_routed_multi_bwd(dw_list, W, r, types, sinks=None, col0=0, ld=0):
    """dw_list: M tensors (T,Ci,Co) or None -> (dW, dfcw, dfcb) summed over the types.  sinks = (gW, gfcw, gfcb): contiguous fp32
    gradient buffers the three results are ADDED to in-kernel (returned as they are).  col0 / ld: the gradients are the column block
    [col0, col0 + Co) of contiguous (T, Ci, ld) tensors (one half of a fused gamma | beta filter gradient)."""
    lib = load()
    E, Co, Ci, kh, kw = W.shape
    T = kh * kw
    if (not (W.dtype is r.dtype is types.dtype is torch.float32) or types.dim() != 2
            or tuple(r.shape) != (types.shape[0], E) or len(dw_list) != types.shape[0]): _refuse('mix_experts_routed_multi_bwd', 'dtype', W, r, types)
    W = W.contiguous(); types = types.contiguous(); r = r.contiguous()
    M, emb = types.shape
    dw_list = [None if g is None else g.contiguous() for g in dw_list]
    if (not 0 <= col0 <= max(ld - Co, 0)
            or any(g is not None and (g.dtype is not torch.float32 or g.numel() != T * Ci * (ld or Co)) for g in dw_list)): _refuse('mix_experts_routed_multi_bwd', 'vec dtype arg', *dw_list)
    a = (_c.c_void_p * M)(*[None if g is None else g.data_ptr() + 4 * col0 for g in dw_list])
    if sinks is not None:
        dW, dfcw, dfcb = sinks
        if (any(s.dtype is not torch.float32 or not s.is_contiguous() for s in sinks)
                or (dW.numel(), dfcw.numel(), dfcb.numel()) != (W.numel(), E * emb, E)): _refuse('mix_experts_routed_multi_bwd', 'vec dtype dense', *sinks)
    else:
        dW = torch.empty_like(W)
        dfcw = torch.empty((E, emb), dtype=torch.float32, device=W.device)
        dfcb = torch.empty(E, dtype=torch.float32, device=W.device)
    nb = _ws_bytes(lib.mrdis_mix_experts_routed_multi_bwd_workspace, M, E, Co, Ci, T)
    ws = _ws(nb, W.device)
    _chk(lib.mrdis_mix_experts_routed_multi_bwd(a, _ptr(W), _ptr(r), _ptr(types), emb, M, _ptr(dW), _ptr(dfcw), _ptr(dfcb),
                                                1 if sinks is not None else 0, ld, _ptr(ws), nb, E, Co, Ci, T, _stream()), 'mix_experts_routed_multi_bwd')
    return dW, dfcw, dfcb


# ---------------------------------------------------------------- convolution
def conv_out_hw(H, W, kh, kw, stride, pad):
    return (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1


DT_F32, DT_F32_BF16M, DT_BF16 = 0, 1, 2          # include/mrdis.h MRDIS_DT_*
DT_DW_PAD16 = 0x100                            # conv2d_bwd_weight(pad16=True): dw in the stored 16-row / 16-column shape of the filter (mrdis.h)
DT_XBF16_YF32, DT_XF32_YBF16 = 3, 4              # mixed storage at the ends of a bf16 stretch (layer input x / output y)


def _dt_xy(x, y):
    """storage code of a layer whose input-side view is x (or dx) and output-side view y (or dy)"""
    if x.dtype is y.dtype:
        return _dt(x)
    if x.dtype is torch.bfloat16 and y.dtype is torch.float32:
        return DT_XBF16_YF32
    if x.dtype is torch.float32 and y.dtype is torch.bfloat16:
        return DT_XF32_YBF16
    raise MrdisError(f'activation views must be fp32 or bf16, got {x.dtype} and {y.dtype}')


def cast_bf16(t):
    """fp32 tensor -> bf16 copy (round to nearest even) through the library's cast kernel."""
    lib = load()
    if t.dtype is not torch.float32: _refuse('cast_bf16', 'dtype', t)
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
    _chk(lib.mrdis_cast_bf16(_ptr(t), _ptr(out), t.numel(), _stream()), 'cast_bf16')
    return out


def conv2d_fwd(x, w_tck, bias, kh, kw, stride, pad, lrelu=False, out=None, w_bf16=None, out_dtype=None, may_decline=False, w_wino=None):
    """w_bf16: bf16 [T][Co][Ci] copy of the filter (reduction axis contiguous) -> bf16 MFMA operands, fp32 accumulate
    (MRDIS_DT_F32_BF16M) where the geometry allows; None -> exact fp32.
    Mixed storage (out / out_dtype differ from x.dtype): the 1x1 head reads bf16 and writes fp32 (MRDIS_DT_XBF16_YF32); the 3x3
    4 -> C si_layers read the fp32 anatomy map and write bf16 (MRDIS_DT_XF32_YBF16, w_tck in the 16-row layout of the mixing launch).
    may_decline: return None instead of raising when the library has no kernel for a mixed-storage geometry."""
    lib = load()
    x, ldx = nhwc(x)
    N, Ci, H, W = x.shape
    T, Ci2, Co = w_tck.shape
    Ho, Wo = conv_out_hw(H, W, kh, kw, stride, pad)
    if out is None:
        out = empty_nhwc(N, Co, Ho, Wo, x.device, out_dtype or x.dtype)
    y, ldy = nhwc(out)
    mixed = _dt_xy(x, y)
    if mixed == DT_XBF16_YF32 and kh == 3 and Co == 16 and out.shape[1] == 4:
        Co = 4                       # the C -> 4 layer with its filter in the column-padded [9][Ci][16] layout (ana_dec.output under bf16 storage)
    if (y is not out or tuple(y.shape) != (N, Co, Ho, Wo) or T != kh * kw      # (bias: at least Co values; the column-padded C -> 4 layer comes with its 16)
            or not (Ci2 == Ci or (mixed == DT_XF32_YBF16 and Ci2 == max(Ci, 16))) or (bias is not None and bias.numel() < Co)): _refuse('conv2d_fwd', 'filter out vec', out, w_tck, bias)
    if mixed in (DT_XBF16_YF32, DT_XF32_YBF16):
        rc = lib.mrdis_conv2d_fwd(_ptr(x), ldx, _ptr(w_tck), None, _ptr(bias), _ptr(y), ldy, N, H, W, Ci, Co, kh, kw, stride, pad,
                                  1 if lrelu else 0, mixed, None, 0, _stream())
        if rc == -2 and may_decline:
            return None
        _chk(rc, 'conv2d_fwd (mixed storage)')
        return out
    if w_bf16 is not None and w_bf16.dtype is torch.float32:      # the auxiliary-filter slot carries the Winograd image on the fp32 path
        w_wino, w_bf16 = w_bf16, None
    if w_bf16 is not None and (w_bf16.dtype is not torch.bfloat16 or tuple(w_bf16.shape) != (T, Co, Ci) or not w_bf16.is_contiguous()): _refuse('conv2d_fwd', 'filter dtype dense', w_bf16)
    wfmt = 0 if w_wino is None else _image_fmt(w_wino, Ci, Co, T, kh, kw, 'conv2d_fwd')
    dt = DT_BF16 if mixed == DT_BF16 else (DT_F32 if w_bf16 is None else DT_F32_BF16M)     # bf16 views: bf16 kernels only
    rc = lib.mrdis_conv2d_fwd(_ptr(x), ldx, _ptr(w_tck), _ptr(w_bf16), _ptr(bias), _ptr(y), ldy, N, H, W, Ci, Co, kh, kw, stride, pad,
                              1 if lrelu else 0, dt, _ptr(w_wino) if dt == DT_F32 else None, wfmt, _stream())
    if rc == -2 and dt == DT_BF16:
        # a tile geometry the bf16 kernel cannot stage (or a view it cannot address): the fp32 kernel between two view casts
        y32 = conv2d_fwd(cast_view(x, torch.float32), w_tck, bias, kh, kw, stride, pad, lrelu)
        lib.mrdis_cast_view(_ptr(y32), Co, DT_F32, Co, _ptr(y), ldy, DT_BF16, Co, N * Ho * Wo, _stream())
        return out
    _chk(rc, 'conv2d_fwd')
    return out


def conv2d_bwd_data(dy, w_tkc, in_hw, kh, kw, stride, pad, w_bf16=None, out=None, w_wino=None, may_decline=False):
    """w_bf16: bf16 [T][Ci][Co] copy (the data gradient reduces over Co).  out: a dense NHWC (N, Ci, H, W) view to write into.
    Mixed storage (fp32 dy, bf16 out: the 1x1 head; the 3x3 C <- 4 layer with the filter in its 16-row layout [9][16][Ci]; bf16 dy, fp32
    out: the si_layers' 4 <- C data gradient with the filter as [9][Co][16]) has only its dedicated kernels: may_decline returns None
    instead of raising outside them."""
    lib = load()
    dy, lddy = nhwc(dy)
    N, Co, Ho, Wo = dy.shape
    T, Co2, Ci = w_tkc.shape
    H, W = in_hw
    mixed = out is not None and out.dtype != dy.dtype
    if mixed and kh == 3 and Ci == 16 and out.shape[1] == 4:
        Ci = 4                       # the si_layers' data gradient with the filter in the column-padded [9][Co][16] layout (bf16 dy -> fp32 dx: MRDIS_DT_XF32_YBF16)
    if (T != kh * kw or not (Co2 == Co or (mixed and Co2 == 16 and Co == 4 and kh == 3))
            or conv_out_hw(H, W, kh, kw, stride, pad) != (Ho, Wo)): _refuse('conv2d_bwd_data', 'layer filter', w_tkc, dy)
    if out is None:
        dx = empty_nhwc(N, Ci, H, W, dy.device, dy.dtype); ldo = Ci
    else:
        dx, ldo = nhwc(out)          # a channel slice of a wider NHWC buffer is fine (ldo > Ci)
        if dx is not out or ldo < Ci or tuple(out.shape) != (N, Ci, H, W): _refuse('conv2d_bwd_data', 'out', out)
        if mixed:                    # bf16 storage: dy fp32 -> dx bf16 (MRDIS_DT_XBF16_YF32), or dy bf16 -> dx fp32 (MRDIS_DT_XF32_YBF16)
            rc = lib.mrdis_conv2d_bwd_data(_ptr(dy), lddy, _ptr(w_tkc), None, _ptr(dx), ldo, N, H, W, Ci, Co, kh, kw, stride, pad, _dt_xy(dx, dy), None, 0, _stream())
            if rc == -2 and may_decline:
                return None
            _chk(rc, 'conv2d_bwd_data (mixed storage)')
            return dx
    if w_bf16 is not None and w_bf16.dtype is torch.float32:
        w_wino, w_bf16 = w_bf16, None
    if w_bf16 is not None and (w_bf16.dtype is not torch.bfloat16 or tuple(w_bf16.shape) != (T, Ci, Co) or not w_bf16.is_contiguous()): _refuse('conv2d_bwd_data', 'filter dtype dense', w_bf16)
    wfmt = 0 if w_wino is None else _image_fmt(w_wino, Co, Ci, T, kh, kw, 'conv2d_bwd_data')
    dt = DT_BF16 if _dt(dy) == DT_BF16 else (DT_F32 if w_bf16 is None else DT_F32_BF16M)
    rc = lib.mrdis_conv2d_bwd_data(_ptr(dy), lddy, _ptr(w_tkc), _ptr(w_bf16), _ptr(dx), ldo, N, H, W, Ci, Co, kh, kw, stride, pad, dt,
                                   _ptr(w_wino) if dt == DT_F32 else None, wfmt, _stream())
    if rc == -2 and dt == DT_BF16:
        # a geometry outside the bf16 kernels (e.g. a reduction axis that is not a multiple of 16): fp32 kernel between two view casts
        res = cast_view(conv2d_bwd_data(cast_view(dy, torch.float32), w_tkc, in_hw, kh, kw, stride, pad), torch.bfloat16)
        if out is None:
            return res
        out.copy_(res)
        return out
    _chk(rc, 'conv2d_bwd_data')
    return dx


fallbacks = collections.Counter()      # routes that left the bf16 kernels for fp32 kernels between view casts (tests read it)


def conv2d_bwd_weight(x, dy, kh, kw, stride, pad, need_bias=True, bias_sink=None, dtype=DT_F32, may_decline=False, pad16=False):
    """-> (dw_tck, dbias).  bias_sink: a (Co,) buffer the bias gradient is ADDED to in the reduce launch
    (then dbias is returned as None).  dtype DT_F32_BF16M: bf16 MFMA operands where the geometry allows.
    may_decline: mixed-storage views (x fp32 / dy bf16: the si_layers; x bf16 / dy fp32: the 1x1 head) only have their dedicated
    kernels -- return None instead of raising when the geometry is outside them (the caller then casts a view).
    pad16 (mixed-storage views with a four-channel side only): dw_tck comes back in the stored shape of a filter of the mixing launch,
    (T, 16, Co) for a 4 -> C layer / (T, Ci, 16) for a C -> 4 layer, zeros beyond the layer's own rows / columns (MRDIS_DT_DW_PAD16)."""
    lib = load()
    x, ldx = nhwc(x)
    dy, lddy = nhwc(dy)
    N, Ci, H, W = x.shape
    Co = dy.shape[1]
    sink = bias_sink if (need_bias and bias_sink is not None) else None
    mixed = x.dtype is not dy.dtype  # bf16 storage: the 1x1 head (x bf16, dy fp32: MRDIS_DT_XBF16_YF32), the si_layers (x fp32, dy bf16: MRDIS_DT_XF32_YBF16)
    if (dy.shape[0] != N or conv_out_hw(H, W, kh, kw, stride, pad) != (dy.shape[2], dy.shape[3])
            or (pad16 and not (mixed and 4 in (Ci, Co))) or (sink is not None and sink.numel() < Co)): _refuse('conv2d_bwd_weight', 'layer vec arg', x, dy, sink)
    dw = torch.empty((kh * kw, 16 if (pad16 and Ci == 4) else Ci, 16 if (pad16 and Co == 4 and Ci != 4) else Co), dtype=torch.float32, device=x.device)
    db = torch.empty(Co, dtype=torch.float32, device=x.device) if (need_bias and bias_sink is None) else None
    nb = _ws_bytes(lib.mrdis_conv2d_bwd_weight_workspace, N, H, W, Ci, Co, kh, kw, stride, pad)
    if nb == 0:
        raise MrdisError('conv2d_bwd_weight: unsupported geometry')
    ws = _ws(nb, x.device)
    dt = (_dt_xy(x, dy) | (DT_DW_PAD16 if pad16 else 0)) if mixed else (DT_BF16 if _dt(x, dy) == DT_BF16 else int(dtype))
    rc = lib.mrdis_conv2d_bwd_weight(_ptr(x), ldx, _ptr(dy), lddy, _ptr(dw), _ptr(sink if sink is not None else db), _ptr(ws), nb,
                                     N, H, W, Ci, Co, kh, kw, stride, pad, 1 if sink is not None else 0, dt, _stream())
    if rc == -2 and mixed and may_decline:      # mixed storage has only its dedicated kernels
        return None
    if rc == -2 and x.dtype is dy.dtype is torch.bfloat16:      # tiny maps / shapes outside the bf16 kernels' domain: the fp32 weight-gradient kernels on fp32 copies of the two views
        fallbacks['conv2d_bwd_weight_bf16'] += 1
        return conv2d_bwd_weight(cast_view(x, torch.float32), cast_view(dy, torch.float32), kh, kw, stride, pad, need_bias, bias_sink, DT_F32)
    _chk(rc, 'conv2d_bwd_weight (mixed storage)' if mixed else 'conv2d_bwd_weight')
    return dw, db


def lrelu_bwd(dy, y, slope=0.2):
    lib = load()
    dy, lddy = nhwc(dy); y, ldy = nhwc(y)
    N, C, H, W = y.shape
    if dy.shape != y.shape: _refuse('lrelu_bwd', 'like', dy, y)
    dx = empty_nhwc(N, C, H, W, y.device, y.dtype)
    _chk(lib.mrdis_lrelu_bwd(_ptr(dy), lddy, _ptr(y), ldy, _ptr(dx), C, N * H * W, C, slope, _dt(dy, y), _stream()), 'lrelu_bwd')
    return dx


# ---------------------------------------------------------------- norms
def bn_train_fwd(x, gamma, beta, running_mean, running_var, eps, momentum, out=None, groups=1):
    """groups = G: the batch holds G equal sample blocks that the reference normalises in G separate calls of this layer
    (statistics per block: mean / rstd are (G * C); running statistics updated block by block)."""
    lib = load()
    x, ldx = nhwc(x)
    N, C, H, W = x.shape
    P = (N // groups) * H * W
    if out is None:
        out = empty_nhwc(N, C, H, W, x.device, x.dtype)
    y, ldy = nhwc(out)
    if (y is not out or out.shape != x.shape or N % groups != 0 or gamma.numel() != C or beta.numel() != C or running_mean.numel() != C
            or running_var.numel() != C or not (gamma.dtype is beta.dtype is running_mean.dtype is running_var.dtype is torch.float32)):
        _refuse('bn_train_fwd', 'like out vec dtype arg', out, gamma, beta, running_mean, running_var)
    mean = torch.empty(groups * C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(groups * C, dtype=torch.float32, device=x.device)
    nb = groups * _ws_bytes(lib.mrdis_norm_workspace, 1, P, C)
    ws = _ws(nb, x.device)
    _chk(lib.mrdis_bn_train_fwd(_ptr(x), ldx, _ptr(y), ldy, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                _ptr(mean), _ptr(rstd), _ptr(ws), nb, P, C, eps, momentum, groups, _dt(x, y), _stream()), 'bn_train_fwd')
    return out, mean, rstd


def bn_eval_fwd(x, gamma, beta, running_mean, running_var, eps):
    lib = load()
    x, ldx = nhwc(x)
    N, C, H, W = x.shape
    if (gamma.numel() != C or beta.numel() != C or running_mean.numel() != C or running_var.numel() != C
            or not (gamma.dtype is beta.dtype is running_mean.dtype is running_var.dtype is torch.float32)): _refuse('bn_eval_fwd', 'vec dtype', gamma, beta)
    y = empty_nhwc(N, C, H, W, x.device, x.dtype)
    _chk(lib.mrdis_bn_eval_fwd(_ptr(x), ldx, _ptr(y), C, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                               N * H * W, C, eps, _dt(x), _stream()), 'bn_eval_fwd')
    return y


def bn_train_bwd(dy, x, gamma, mean, rstd, sink=None, groups=1):
    """-> (dx, dgamma, dbeta).  sink = (acc_dgamma, acc_dbeta): buffers this call's parameter gradients are also added to.
    groups: as bn_train_fwd (dgamma / dbeta are then summed over the groups here)."""
    lib = load()
    dy, lddy = nhwc(dy); x, ldx = nhwc(x)
    N, C, H, W = x.shape
    ag, ab = sink if sink is not None else (None, None)
    if (dy.shape != x.shape or N % groups != 0 or gamma.numel() != C or mean.numel() != groups * C or rstd.numel() != groups * C
            or (ag is not None and (ag.numel() != C or ab.numel() != C)) or not (gamma.dtype is mean.dtype is rstd.dtype is torch.float32)):
        _refuse('bn_train_bwd', 'like vec dtype arg', dy, x, gamma, mean, rstd, ag, ab)
    P = (N // groups) * H * W
    dx = empty_nhwc(N, C, H, W, x.device, x.dtype)
    dg = torch.empty(groups * C, dtype=torch.float32, device=x.device)
    db = torch.empty(groups * C, dtype=torch.float32, device=x.device)
    nb = groups * _ws_bytes(lib.mrdis_norm_workspace, 1, P, C)
    ws = _ws(nb, x.device)
    _chk(lib.mrdis_bn_train_bwd(_ptr(dy), lddy, _ptr(x), ldx, _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx), C, _ptr(dg), _ptr(db),
                                _ptr(ag), _ptr(ab), _ptr(ws), nb, P, C, groups, _dt(dy, x), _stream()), 'bn_train_bwd')
    if groups > 1 and sink is None:
        dg, db = dg.view(groups, C).sum(0), db.view(groups, C).sum(0)
    return dx, dg, db


def instnorm_spade_fwd(z, gamma, beta, eps=1e-5, stats=None):
    """stats = (mean, rstd) of z already computed (bilinear_up2_stats): the statistics pass is skipped"""
    lib = load()
    z, ldz = nhwc(z); gamma, ldg = nhwc(gamma); beta, ldb = nhwc(beta)
    N, C, H, W = z.shape
    if (gamma.shape != z.shape or beta.shape != z.shape
            or (stats is not None and not (stats[0].numel() == stats[1].numel() == N * C and stats[0].dtype is stats[1].dtype is torch.float32 and stats[0].is_contiguous() and stats[1].is_contiguous()))):
        _refuse('instnorm_spade_fwd', 'like vec dense', z, gamma, beta, *(stats or ()))
    out = empty_nhwc(N, C, H, W, z.device, z.dtype)
    if stats is not None:
        mean, rstd = stats
        _chk(lib.mrdis_instnorm_spade_fwd(_ptr(z), ldz, _ptr(gamma), ldg, _ptr(beta), ldb, _ptr(out), C, _ptr(mean), _ptr(rstd),
                                          None, 0, N, H * W, C, eps, _dt(z, gamma, beta), _stream()), 'instnorm_spade_fwd')
        return out, mean, rstd
    mean = torch.empty(N * C, dtype=torch.float32, device=z.device)
    rstd = torch.empty(N * C, dtype=torch.float32, device=z.device)
    nb = _ws_bytes(lib.mrdis_norm_workspace, N, H * W, C)
    ws = _ws(nb, z.device)
    _chk(lib.mrdis_instnorm_spade_fwd(_ptr(z), ldz, _ptr(gamma), ldg, _ptr(beta), ldb, _ptr(out), C, _ptr(mean), _ptr(rstd),
                                      _ptr(ws), nb, N, H * W, C, eps, _dt(z, gamma, beta), _stream()), 'instnorm_spade_fwd')
    return out, mean, rstd


def gb_spade_fwd(si_out, w_tck, bias, z, eps=1e-5, out=None, w_bf16=None, stats_ready=False, w_wino=None):
    """fused gamma | beta convolution + InstanceNorm modulation (mrdis_conv2d_fwd_spade): -> (mix, gamma, mean, rstd), or None where the
    fused kernel does not apply (the caller then runs conv2d_fwd + instnorm_spade_fwd).  fp32 views, or bf16 views with w_bf16 = the bf16
    [9][2C][Ci] filter.  out = (mix, gamma, mean, rstd) dense views to fill."""
    lib = load()
    if si_out.dtype is not z.dtype or (z.dtype is torch.bfloat16 and w_bf16 is None):
        return None
    x, ldx = nhwc(si_out); z, ldz = nhwc(z)
    N, C, H, W = z.shape
    Ci = x.shape[1]
    if tuple(w_tck.shape) != (9, Ci, 2 * C) or x.shape[0] != N or x.shape[2] != H or x.shape[3] != W:
        return None
    dt = _dt(x, z)
    if out is None:
        mean = torch.empty(N * C, dtype=torch.float32, device=z.device)
        rstd = torch.empty(N * C, dtype=torch.float32, device=z.device)
        mix = empty_nhwc(N, C, H, W, z.device, z.dtype)
        gamma = empty_nhwc(N, C, H, W, z.device, z.dtype)
    else:
        mix, gamma, mean, rstd = out
    if (mix.shape != z.shape or gamma.shape != z.shape or mean.numel() != N * C or rstd.numel() != N * C or not (mean.dtype is rstd.dtype is torch.float32)
            or (bias is not None and (bias.numel() != 2 * C or bias.dtype is not torch.float32))
            or (w_bf16 is not None and w_bf16.numel() != w_tck.numel())): _refuse('gb_spade_fwd', 'like out vec dtype', mix, gamma, mean, rstd, bias, w_bf16)
    wfmt = 0 if w_wino is None else _image_fmt(w_wino, Ci, 2 * C, 0, 3, 3, 'gb_spade_fwd', spadeC=C)
    nb = _ws_bytes(lib.mrdis_norm_workspace, N, H * W, C)
    ws = _ws(nb, z.device)
    st = _stream()
    # the statistics first (stream order); if the fused kernel then declines, they are simply recomputed by the two-step path
    # (stats_ready: `out`'s mean / rstd already hold them -- the x2 resize that produced z took them on the way, bilinear_up2_stats)
    if not stats_ready:
        _chk(lib.mrdis_instnorm_stats(_ptr(z), ldz, _ptr(mean), _ptr(rstd), _ptr(ws), nb, N, H * W, C, eps, dt, st), 'instnorm_stats')
    rc = lib.mrdis_conv2d_fwd_spade(_ptr(x), ldx, _ptr(w_tck), _ptr(w_bf16), _ptr(bias), _ptr(z), ldz, _ptr(mean), _ptr(rstd), _ptr(mix), C, _ptr(gamma), C,
                                    N, H, W, Ci, C, dt, _ptr(w_wino) if dt == DT_F32 else None, wfmt, st)
    if rc == -2:
        return None
    _chk(rc, 'conv2d_fwd_spade')
    return mix, gamma, mean, rstd


def gb_slot(t):
    """the (N, 2C, H, W) NHWC buffer whose channels [C, 2C) are exactly the NCHW-shaped tensor `t`, or None"""
    base = t._base
    if base is None or base.dim() != 4 or t.dim() != 4 or not getattr(base, '_mrdis_gb_private', False):
        return None      # only buffers a grouped convolution allocated for this purpose: any other upper-half channel slice (a torch.cat adjoint,
                         # a skip-connection half) shares its lower half with another consumer
    N, C, H, W = t.shape
    if tuple(base.shape) != (N, 2 * C, H, W) or base.dtype != t.dtype or not base.is_contiguous(memory_format=torch.channels_last):
        return None
    if t.stride() != (H * W * 2 * C, 1, W * 2 * C, 2 * C) or t.storage_offset() != base.storage_offset() + C:
        return None
    return base


def instnorm_spade_bwd(dout, z, gamma, mean, rstd, fused_gb=False, up2=False, xlo=None):
    """returns (dz, dgamma); dbeta == dout and is not materialised.
    fused_gb=True: returns (dz, dgb) with dgb (N,2C,H,W) = [dgamma | dout] in one buffer (the gradient of
    a fused gamma+beta convolution output).
    up2=True (with fused_gb): z is the x2 bilinear resize of a map x -- the first result is d x (N, C, H/2, W/2), the resize's adjoint applied inside
    the kernel (mrdis_instnorm_spade_bwd_up2); None when the library declines the geometry.  xlo = x: z may be None, the kernels interpolate it from x."""
    lib = load()
    dout, lddo = nhwc(dout); gamma, ldg = nhwc(gamma)
    N, C, H, W = gamma.shape
    if z is not None:
        z, ldz = nhwc(z)
    else:
        ldz = 0
    if (dout.shape != gamma.shape or mean.numel() != N * C or rstd.numel() != N * C or not (mean.dtype is rstd.dtype is torch.float32)
            or (z.shape != gamma.shape if z is not None else not (up2 and xlo is not None))): _refuse('instnorm_spade_bwd', 'like vec dtype arg', dout, z, gamma, mean, rstd)
    dt = _dt(dout, gamma) if z is None else _dt(dout, z, gamma)
    xl, ldxl = (None, 0) if xlo is None or not up2 else nhwc(xlo)
    if up2 and (not fused_gb or H % 2 or W % 2
                or (xl is not None and (tuple(xl.shape) != (N, C, H // 2, W // 2) or xl.dtype is not gamma.dtype))): _refuse('instnorm_spade_bwd', 'dtype arg', gamma, xlo)
    nb = _ws_bytes(lib.mrdis_instnorm_spade_bwd_up2_workspace, N, H // 2, W // 2, C, dt) if up2 else _ws_bytes(lib.mrdis_instnorm_spade_bwd_workspace, N, H * W, C)
    ws = _ws(nb, gamma.device)
    dg, lddg, dbp, lddb = gb_slot(dout) if fused_gb else None, 2 * C, None, 0
    if not fused_gb:
        dg, lddg = empty_nhwc(N, C, H, W, gamma.device, gamma.dtype), C
    elif dg is None:
        dg = empty_nhwc(N, 2 * C, H, W, gamma.device, gamma.dtype)
        dbp, lddb = dg.data_ptr() + dg.element_size() * C, 2 * C
    # (else dout already IS channels [C, 2C) of a 2C-channel buffer -- its producer wrote it there, ops._GroupedConvFn: only dgamma is written, into
    # the first half -- one pass over the tensor less)
    if up2:
        dx = empty_nhwc(N, C, H // 2, W // 2, gamma.device, gamma.dtype)
        rc = lib.mrdis_instnorm_spade_bwd_up2(_ptr(dout), lddo, _ptr(z), ldz, _ptr(gamma), ldg, _ptr(mean), _ptr(rstd), _ptr(dx), C, dg.data_ptr(), lddg, dbp, lddb,
                                              _ptr(ws), nb, N, H // 2, W // 2, C, _ptr(xl), ldxl, dt, _stream())
        if rc == -2:
            return None
        _chk(rc, 'instnorm_spade_bwd_up2')
        return dx, dg
    dz = empty_nhwc(N, C, H, W, z.device, z.dtype)
    _chk(lib.mrdis_instnorm_spade_bwd(_ptr(dout), lddo, _ptr(z), ldz, _ptr(gamma), ldg, _ptr(mean), _ptr(rstd), _ptr(dz), C, dg.data_ptr(), lddg, dbp, lddb,
                                      _ptr(ws), nb, N, H * W, C, dt, _stream()), 'instnorm_spade_bwd')
    return dz, dg


# ---------------------------------------------------------------- resize / softmax / losses
def bilinear_fwd(x, out_hw, align_corners):
    lib = load()
    x, ldx = nhwc(x)
    N, C, Hi, Wi = x.shape
    Ho, Wo = out_hw
    y = empty_nhwc(N, C, Ho, Wo, x.device, x.dtype)
    _chk(lib.mrdis_bilinear_fwd(_ptr(x), ldx, _ptr(y), C, N, Hi, Wi, Ho, Wo, C, 1 if align_corners else 0, _dt(x), _stream()), 'bilinear_fwd')
    return y


def bilinear_up2_stats_applies(N, Wi, C):
    return bool(load().mrdis_bilinear_up2_stats_applies(int(N), int(Wi), int(C)))


def bilinear_up2_stats(x, eps, out_blocks=None):
    """x2 bilinear (align_corners=False) + instance statistics of the result: -> (y, mean, rstd), or None where the fused kernel does not apply.
    out_blocks: a (G, Bb, C, 2 Hi, 2 Wi) view, G * Bb = N, each out_blocks[g] a dense NHWC block: image n is written to out_blocks[n // Bb][n % Bb]
    (then y is out_blocks itself)."""
    lib = load()
    x, ldx = nhwc(x)
    N, C, Hi, Wi = x.shape
    if C % 4 != 0:
        return None
    blk, bstride = 0, 0
    if out_blocks is None:
        y = empty_nhwc(N, C, 2 * Hi, 2 * Wi, x.device, x.dtype)
        yptr = _ptr(y)
    else:
        if (out_blocks.dim() != 5 or out_blocks.shape[0] * out_blocks.shape[1] != N
                or tuple(out_blocks.shape[2:]) != (C, 2 * Hi, 2 * Wi) or out_blocks.dtype is not x.dtype): _refuse('bilinear_up2_stats', 'out dtype', out_blocks)
        G, Bb = out_blocks.shape[0], out_blocks.shape[1]
        y0, ld0 = nhwc(out_blocks[0])
        if (ld0 != C or y0.data_ptr() != out_blocks.data_ptr()
                or (G > 1 and out_blocks.stride(0) < Bb * 4 * Hi * Wi * C)): _refuse('bilinear_up2_stats', 'out dense', out_blocks)
        y, yptr, blk, bstride = out_blocks, _ptr(y0), Bb, out_blocks.stride(0)
    mean = torch.empty(N * C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(N * C, dtype=torch.float32, device=x.device)
    nb = _ws_bytes(lib.mrdis_bilinear_up2_stats_workspace, N, Hi, C)
    ws = _ws(nb, x.device)
    rc = lib.mrdis_bilinear_up2_stats_fwd(_ptr(x), ldx, yptr, C, N, Hi, Wi, C, blk, bstride, _ptr(mean), _ptr(rstd), eps, _ptr(ws), nb, _dt(x), _stream())
    if rc == -2:
        return None
    _chk(rc, 'bilinear_up2_stats_fwd')
    return y, mean, rstd


def bilinear_bwd(dy, in_hw, align_corners, out=None):
    lib = load()
    dy, lddy = nhwc(dy)
    N, C, Ho, Wo = dy.shape
    Hi, Wi = in_hw
    if out is None:
        dx = empty_nhwc(N, C, Hi, Wi, dy.device, dy.dtype)
    else:
        dx, ldo = nhwc(out)
        if dx is not out or ldo != C or tuple(out.shape) != (N, C, Hi, Wi) or out.dtype is not dy.dtype: _refuse('bilinear_bwd', 'out dtype dense', out, dy)
    _chk(lib.mrdis_bilinear_bwd(_ptr(dy), lddy, _ptr(dx), C, N, Hi, Wi, Ho, Wo, C, 1 if align_corners else 0, _dt(dy), _stream()), 'bilinear_bwd')
    return dx


def softmax_mask_drop_fwd(s, mask_img, scale=100.0):
    lib = load()
    s, lds = nhwc(s)
    N, C, H, W = s.shape
    if (s.dtype is not torch.float32
            or (mask_img is not None and (mask_img.dtype is not torch.float32 or mask_img.numel() != N * H * W))): _refuse('softmax_mask_drop_fwd', 'vec dtype', s, mask_img)
    out = empty_nhwc(N, C, H, W, s.device)
    m = None if mask_img is None else mask_img.contiguous()
    _chk(lib.mrdis_softmax_mask_drop_fwd(_ptr(s), lds, _ptr(m), _ptr(out), C, N * H * W, C, scale, _stream()), 'softmax_mask_drop_fwd')
    return out


def softmax_mask_drop_bwd(dout, out):
    lib = load()
    dout, lddo = nhwc(dout); out, ldo = nhwc(out)
    N, C, H, W = out.shape
    if dout.shape != out.shape or not (dout.dtype is out.dtype is torch.float32): _refuse('softmax_mask_drop_bwd', 'like out dtype', dout, out)
    ds = empty_nhwc(N, C, H, W, out.device)
    _chk(lib.mrdis_softmax_mask_drop_bwd(_ptr(dout), lddo, _ptr(out), ldo, _ptr(ds), C, N * H * W, C, _stream()), 'softmax_mask_drop_bwd')
    return ds


def recon_err_fwd(gt, x, p):
    lib = load()
    gt, ldgt = nhwc(gt); x, ldx = nhwc(x)
    N, C, H, W = x.shape
    if gt.shape != x.shape or not (gt.dtype is x.dtype is torch.float32): _refuse('recon_err_fwd', 'like dtype', gt, x)
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    nb = _ws_bytes(lib.mrdis_recon_err_workspace, N, H * W, C)
    ws = _ws(nb, x.device)
    _chk(lib.mrdis_recon_err_fwd(_ptr(gt), ldgt, _ptr(x), ldx, _ptr(out), _ptr(ws), nb, N, H * W, C, p, _stream()), 'recon_err_fwd')
    return out


def recon_metrics(target, pred):
    """(N, 3) = MSE / PSNR / SSIM of channel 0 of each sample (util.py:935-978)."""
    lib = load()
    target, ldt = nhwc(target); pred, ldp = nhwc(pred)
    N, _, H, W = pred.shape
    if ((target.shape[0], target.shape[2], target.shape[3]) != (N, H, W)
            or not (target.dtype is pred.dtype is torch.float32)): _refuse('recon_metrics', 'dtype', target, pred)
    out = torch.empty(N, 3, dtype=torch.float32, device=pred.device)
    nb = _ws_bytes(lib.mrdis_recon_metrics_workspace, N, H)
    ws = _ws(nb, pred.device)
    _chk(lib.mrdis_recon_metrics(_ptr(target), ldt, _ptr(pred), ldp, _ptr(out), _ptr(ws), nb, N, H, W, _stream()), 'recon_metrics')
    return out


def slice_gather(vol_ptrs, slice_idx, drop, H, W, D, block):
    """vol_ptrs (B,M) int64, slice_idx (B) int32, drop (B) int32 on the device -> inputs (B,(2b+1)M,H,W) NHWC, mask (B,M),
    mask_img (B,H,W)."""
    lib = load()
    B, M = _want(vol_ptrs, 'slice_gather: vol_ptrs', torch.int64, ('B', 'M'))
    _want(slice_idx, 'slice_gather: slice_idx', torch.int32, (B,), vol_ptrs.device)
    _want(drop, 'slice_gather: drop', torch.int32, (B,), vol_ptrs.device)
    C = M * (2 * block + 1)
    inputs = empty_nhwc(B, C, H, W, vol_ptrs.device)
    mask = torch.empty((B, M), dtype=torch.float32, device=vol_ptrs.device)
    mask_img = torch.empty((B, H, W), dtype=torch.float32, device=vol_ptrs.device)
    _chk(lib.mrdis_slice_gather(_ptr(vol_ptrs), _ptr(slice_idx), _ptr(drop), _ptr(inputs), C, _ptr(mask), _ptr(mask_img),
                                B, M, H, W, D, block, _stream()), 'slice_gather')
    return inputs, mask, mask_img


def volume_gather(table, M, H, W, D, z0, Dz, targets=False, K=0, relabel=False):
    """table (B, >= 2M+3) int64 on the device (include/mrdis.h mrdis_volume_gather) -> inputs (B,M,H,W,Dz) channels-last-3d and mask (B,M), or
    with `targets` the label volume (B,H,W,Dz) / its K region channels (B,K,H,W,Dz) channels-last-3d.  One launch."""
    lib = load()
    B, ld = _want(table, 'volume_gather: table', torch.int64, ('B', 'ld'))
    if ld < 2 * M + 3: _refuse(f'volume_gather: table rows of at least 2 M + 3 = {2 * M + 3} words', 'vec', table)
    return _gather3d(lib.mrdis_volume_gather, 'volume_gather', table, None, M, (H, W, D), (H, W, Dz), (z0, Dz), targets, K, relabel)


def _gather3d(entry, what, table, origins, M, vol, box, box_args, targets, K, relabel):
    """the call of the three gathers of the 3-D store -- volume_gather, patch3d.patch_gather, warp3d.patch_warp -- whose caller has checked
    every argument: `entry` on table (B, ld) (and origins, where the entry point takes them), the stored volumes `vol` = (H, W, D), the
    output `box` of a sample, `box_args` the integers the entry point takes for it -> inputs (B, M, *box) channels-last-3d and mask (B, M),
    or with `targets` the labels (B, *box) / their K region channels (B, K, *box) channels-last-3d.  One launch."""
    B, ld = table.shape
    dev = table.device
    head = (_ptr(table), ld) + (() if origins is None else (_ptr(origins),))
    if not targets:
        out = torch.empty((B, *box, M), dtype=torch.float32, device=dev)
        mask = torch.empty((B, M), dtype=torch.float32, device=dev)
        _chk(entry(*head, _ptr(out), _ptr(mask), B, M, *vol, *box_args, 0, 0, 0, _stream()), what)
        return out.permute(0, 4, 1, 2, 3), mask
    out = torch.empty((B, *box, K) if K else (B, *box), dtype=torch.float32, device=dev)
    _chk(entry(*head, _ptr(out), None, B, M, *vol, *box_args, 1, K, int(bool(relabel)), _stream()), what)
    return out.permute(0, 4, 1, 2, 3) if K else out


def _layout_args(a, b, what):
    """(stride array of a, of b, shape array, ndim) for the entry points that take two tensors of one shape and check their layout themselves"""
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.device != b.device: _refuse(what, 'dtype', a, b)
    if tuple(a.shape) != tuple(b.shape) or not 1 <= a.dim() <= 8: _refuse(what + ' (1 to 8 dimensions)', 'like', a, b)
    nd = a.dim()
    arr = _c.c_longlong * nd
    return arr(*a.stride()), arr(*b.stride()), arr(*a.shape), nd


def _nvnet_layouts(what, uout, target, vout, x):
    """the layout arguments of the pairs (uout, target) and (vout, x) of the 3-D objective: the second pair comes whole or not at all"""
    if (vout is None) != (x is None) or (vout is not None and vout.device != uout.device): _refuse(what + ': vout and x, together or not at all, on the device of uout', 'arg', vout, x)
    second = (None, None, None, 0) if vout is None else _layout_args(vout, x, f'{what} (vout, x)')
    return _layout_args(uout, target, f'{what} (uout, target)') + second


def nvnet_loss_fwd(uout, target, vout=None, x=None, w_l2=0.1):
    """-> (sums (4,) float64 = [sum p t, sum p^2, sum t^2, sum (v - x)^2], terms (3,) float32 = [dice, l2, dice + w_l2 * l2]), both on the device
    (include/mrdis.h mrdis_nvnet_loss_fwd).  uout / target and vout / x: one shape and one dense layout per pair, else MrdisError; nothing is copied."""
    lib = load()
    su, st, shu, ndu, sv, sx, shv, ndv = _nvnet_layouts('nvnet_loss_fwd', uout, target, vout, x)
    dev = uout.device
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    terms = torch.empty(3, dtype=torch.float32, device=dev)
    nb = _ws_bytes(lib.mrdis_nvnet_loss_workspace, uout.numel(), 0 if vout is None else vout.numel())
    ws = _ws(nb, dev)
    _chk(lib.mrdis_nvnet_loss_fwd(_ptr(uout), su, _ptr(target), st, shu, ndu, _ptr(vout), sv, _ptr(x), sx, shv, ndv, float(w_l2),
                                  _ptr(sums), _ptr(terms), _ptr(ws), nb, _stream()), 'nvnet_loss_fwd')
    return sums, terms


def nvnet_loss_bwd(g, sums, uout, target, vout=None, x=None, w_l2=0.1, need_du=True, need_dv=True):
    """-> (du, dv) in the layouts of uout / vout (None where not wanted); g: the gradient of terms[2], one fp32 value on the device."""
    lib = load()
    su, st, shu, ndu, sv, sx, shv, ndv = _nvnet_layouts('nvnet_loss_bwd', uout, target, vout, x)
    _want(sums, 'nvnet_loss_bwd: sums', torch.float64, (4,), uout.device)
    need_dv = need_dv and vout is not None
    if not (need_du or need_dv):
        return None, None
    g = g.reshape(1)
    if g.dtype != torch.float32 or g.device != uout.device:
        raise MrdisError('nvnet_loss_bwd: the incoming gradient must be one fp32 value on the tensors\' device')
    du = torch.empty_like(uout) if need_du else None          # (preserve_format: a dense tensor keeps its strides)
    dv = torch.empty_like(vout) if need_dv else None
    if (du is not None and du.stride() != uout.stride()) or (dv is not None and dv.stride() != vout.stride()):
        raise MrdisError('nvnet_loss_bwd: non-dense input')
    _chk(lib.mrdis_nvnet_loss_bwd(_ptr(uout), su, _ptr(target), st, shu, ndu, _ptr(vout), sv, _ptr(x), sx, shv, ndv, float(w_l2),
                                  _ptr(sums), _ptr(g), _ptr(du), _ptr(dv), _stream()), 'nvnet_loss_bwd')
    return du, dv


def seg_counts(pred, target, logits=False):
    """(B, C, 3) int32 on the device = per sample and channel [|pred > 0.5 and target == 1|, |pred > 0.5|, |target == 1|] of (B, C, D, H, W) tensors
    (include/mrdis.h mrdis_seg_counts); `logits`: the kernel applies the sigmoid.  One launch on channels-last-3d inputs (what the nets and the
    loader write); an input in any other layout is first COPIED into that layout (`ndhwc`), unlike the objective's entry points, which refuse."""
    lib = load()
    if tuple(pred.shape) != tuple(target.shape) or pred.device != target.device: _refuse('seg_counts', 'like', pred, target)
    pred, _ = ndhwc(pred); target, _ = ndhwc(target)
    B, C = pred.shape[:2]
    P = pred[0, 0].numel()
    out = torch.zeros((B, C, 3), dtype=torch.int32, device=pred.device)
    _chk(lib.mrdis_seg_counts(_ptr(pred), _ptr(target), _ptr(out), B, P, C, int(bool(logits)), _stream()), 'seg_counts')
    return out


def seg_accum(logits, acc, z0, flip_h=False):
    """acc[:, :, :, z0:z0 + Dz, :] += sigmoid(logits), un-flipped along H if `flip_h` (include/mrdis.h mrdis_seg_accum), in place; returns acc.
    logits (B, C, H, W, Dz) fp32 dense channels-last-3d (the net's output), acc (B, H, W, D, C) fp32 contiguous.  Any other layout raises
    MrdisError: nothing is copied."""
    lib = load()
    B, C, H, W, Dz = _want(logits, 'seg_accum: logits', torch.float32, ('B', 'C', 'H', 'W', 'Dz'), cl=True)
    D = _want(acc, 'seg_accum: acc', torch.float32, (B, H, W, 'D', C), logits.device)[3]
    _chk(lib.mrdis_seg_accum(_ptr(logits), _ptr(acc), B, H, W, Dz, D, C, int(z0), int(bool(flip_h)), _stream()), 'seg_accum')
    return acc


def seg_label_volume(acc, cover, target_ptrs=None, relabel=False):
    """-> (labels (B, H, W, D) uint8, counts (B, C, 3) int32), both on the device (include/mrdis.h mrdis_seg_label_volume).  acc (B, H, W, D, C)
    fp32 contiguous as `seg_accum` leaves it, cover (D,) int32 on the device, target_ptrs (B,) int64 on the device: addresses of raw (H, W, D)
    fp32 label volumes, 0 = none (None: none for any sample).  A tensor that is not dense in that layout raises MrdisError; nothing is copied."""
    lib = load()
    B, H, W, D, C = _want(acc, 'seg_label_volume: acc', torch.float32, ('B', 'H', 'W', 'D', 'C'))
    _want(cover, 'seg_label_volume: cover', torch.int32, (D,), acc.device)
    target_ptrs is None or _want(target_ptrs, 'seg_label_volume: target_ptrs', torch.int64, (B,), acc.device)      # addresses of raw label volumes
    labels = torch.empty((B, H, W, D), dtype=torch.uint8, device=acc.device)
    counts = torch.zeros((B, C, 3), dtype=torch.int32, device=acc.device)
    _chk(lib.mrdis_seg_label_volume(_ptr(acc), _ptr(cover), _ptr(target_ptrs), _ptr(labels), _ptr(counts), B, H, W, D, C, int(bool(relabel)),
                                    _stream()), 'seg_label_volume')
    return labels, counts


def _volume_u8(t, what):
    """(B, H, W, D) of a contiguous uint8 device volume, else MrdisError; nothing is copied"""
    return _want(t, what, torch.uint8, ('B', 'H', 'W', 'D'))


def edt_bins(H, W, D):
    """bins of a surface-distance histogram: every squared distance inside an (H, W, D) volume, 0 included"""
    return (H - 1) ** 2 + (W - 1) ** 2 + (D - 1) ** 2 + 1


def _edt_geometry(B, H, W, D, what):
    if not (1 <= B <= 65535 and all(1 <= n <= EDT_MAX_EXTENT for n in (H, W, D)) and edt_bins(H, W, D) - 1 < EDT_FAR):
        raise MrdisError(f'{what}: unsupported geometry {(B, H, W, D)}: each of H, W, D in 1 .. {EDT_MAX_EXTENT}')


def region_surfaces(labels, target_ptrs, region_masks):
    """-> (flags (B, H, W, D) uint8, counts (B, R, 5) int32), both on the device (include/mrdis.h mrdis_region_surfaces).  labels (B, H, W, D)
    uint8 contiguous; target_ptrs (B,) int64 on the device: addresses of raw (H, W, D) fp32 label volumes, 0 = none (None: none for any
    sample); region_masks: R <= 4 host integers, bit l of region_masks[r] set = label l belongs to region r.  flags bit r: surface voxel of
    predicted region r, bit 4 + r: of ground-truth region r; counts = [|P and T|, |P|, |T|, surface voxels of P, surface voxels of T]."""
    lib = load()
    B, H, W, D = _volume_u8(labels, 'region_surfaces: labels')
    masks = [int(m) for m in region_masks]
    R = len(masks)
    if not 1 <= R <= SURF_MAX_REGIONS or any(not 0 <= m <= 255 for m in masks):
        raise MrdisError(f'region_surfaces: 1 .. {SURF_MAX_REGIONS} region masks in 0 .. 255, got {masks}')
    if B < 1 or H < 1 or W < 1 or D < 1: _refuse(f'region_surfaces: unsupported geometry {(B, H, W, D)}', 'arg', labels)
    target_ptrs is None or _want(target_ptrs, 'region_surfaces: target_ptrs', torch.int64, (B,), labels.device)
    flags = torch.empty((B, H, W, D), dtype=torch.uint8, device=labels.device)
    counts = torch.zeros((B, R, 5), dtype=torch.int32, device=labels.device)
    _chk(lib.mrdis_region_surfaces(_ptr(labels), _ptr(target_ptrs), (_I * R)(*masks), R, _ptr(flags), _ptr(counts), B, H, W, D, _stream()),
         'region_surfaces')
    return flags, counts


def edt_sq(src, src_masks=(0xFF,)):
    """-> (S, B, H, W, D) int32 on the device: the exact squared Euclidean distance of every voxel to the nearest voxel of the same batch item
    with (src & src_masks[s]) != 0; 0 on such a voxel, EDT_FAR everywhere in an item without one (include/mrdis.h mrdis_edt_sq).  src
    (B, H, W, D) uint8 contiguous; each of H, W, D in 1 .. 1024, else MrdisError('... unsupported geometry ...')."""
    lib = load()
    B, H, W, D = _volume_u8(src, 'edt_sq: src')
    _edt_geometry(B, H, W, D, 'edt_sq')
    vals = [int(m) for m in src_masks]
    S = len(vals)
    if not 1 <= S <= EDT_MAX_SRC or any(not 0 <= m <= 255 for m in vals):
        raise MrdisError(f'edt_sq: 1 .. {EDT_MAX_SRC} source masks in 0 .. 255, got {vals}')
    masks = bytes(vals)
    out = torch.empty((S, B, H, W, D), dtype=torch.int32, device=src.device)
    nws = _ws_bytes(lib.mrdis_edt_workspace, S, B, H, W, D)
    ws = torch.empty(nws, dtype=torch.uint8, device=src.device)      # 6 bytes per voxel and source: its own allocation, returned after the call
    _chk(lib.mrdis_edt_sq(_ptr(src), masks, S, _ptr(out), _ptr(ws), nws, B, H, W, D, _stream()), 'edt_sq')
    return out


def surface_hist(flags, R):
    """-> hist (B, R, 2, bins) int32 on the device, bins = edt_bins(H, W, D) (include/mrdis.h mrdis_surface_hist): hist[b, r, 0, d2] = surface
    voxels of ground-truth region r at squared distance d2 from the nearest surface voxel of predicted region r, hist[b, r, 1, d2] the other
    way round; a direction whose source surface is empty stays 0.  flags as `region_surfaces` wrote them for R regions.  The distance volumes
    are never stored."""
    lib = load()
    B, H, W, D = _volume_u8(flags, 'surface_hist: flags')
    _edt_geometry(B, H, W, D, 'surface_hist')
    if not 1 <= int(R) <= SURF_MAX_REGIONS:
        raise MrdisError(f'surface_hist: 1 .. {SURF_MAX_REGIONS} regions, got {R}')
    bins = edt_bins(H, W, D)
    hist = torch.zeros((B, int(R), 2, bins), dtype=torch.int32, device=flags.device)
    nws = _ws_bytes(lib.mrdis_edt_workspace, 2 * int(R), B, H, W, D)
    ws = torch.empty(nws, dtype=torch.uint8, device=flags.device)    # (1.29 GB for four BraTS subjects: not kept in the binding's grow-only scratch)
    _chk(lib.mrdis_surface_hist(_ptr(flags), int(R), _ptr(hist), bins, _ptr(ws), nws, B, H, W, D, _stream()), 'surface_hist')
    return hist


def _cc_geometry(B, H, W, D, what):
    if not (1 <= B <= 65535 and all(1 <= n <= CC_MAX_EXTENT for n in (H, W, D)) and H * W * D < (1 << 31)):
        raise MrdisError(f'{what}: unsupported geometry {(B, H, W, D)}: B in 1 .. 65535, each of H, W, D in 1 .. {CC_MAX_EXTENT}, H W D < 2^31')


def cc_label(labels, fg_mask, connectivity=26):
    """-> (comp, size), both (B, H, W, D) int32 on the device (include/mrdis.h mrdis_cc_label).  labels (B, H, W, D) uint8 contiguous; a voxel
    is foreground iff its label l <= 7 and bit l of `fg_mask` (2 .. 254, bit 0 clear) is set.  comp: -1 on background, else the smallest
    in-sample flat index of the voxel's component; size: the component's voxel count at its root voxel, 0 elsewhere.  Three launches."""
    lib = load()
    B, H, W, D = _volume_u8(labels, 'cc_label: labels')
    _cc_geometry(B, H, W, D, 'cc_label')
    fg_mask, connectivity = int(fg_mask), int(connectivity)
    if not 2 <= fg_mask <= 255 or fg_mask & 1 or connectivity not in CC_CONNECTIVITIES:
        raise MrdisError(f'cc_label: fg_mask in 2 .. 254 with bit 0 clear and connectivity in {CC_CONNECTIVITIES}, got {fg_mask} and {connectivity}')
    comp = torch.empty((B, H, W, D), dtype=torch.int32, device=labels.device)
    size = torch.empty((B, H, W, D), dtype=torch.int32, device=labels.device)
    _chk(lib.mrdis_cc_label(_ptr(labels), fg_mask, connectivity, _ptr(comp), _ptr(size), B, H, W, D, _stream()), 'cc_label')
    return comp, size


def cc_clean(labels, comp, size, min_voxels=0, keep_largest=False, et_label=4, et_min_voxels=0, et_replace=1):
    """-> (cleaned (B, H, W, D) uint8, stats (B, 6) int32), both on the device (include/mrdis.h mrdis_cc_clean): the keep rule and the ET rule
    of `postproc.clean_labels` on `labels` and the (comp, size) `cc_label` made of them.  Four launches."""
    lib = load()
    B, H, W, D = _volume_u8(labels, 'cc_clean: labels')
    _cc_geometry(B, H, W, D, 'cc_clean')
    _want(comp, 'cc_clean: comp', torch.int32, (B, H, W, D), labels.device)
    _want(size, 'cc_clean: size', torch.int32, (B, H, W, D), labels.device)
    args = [int(min_voxels), int(bool(keep_largest)), int(et_label), int(et_min_voxels), int(et_replace)]
    if args[0] < 0 or args[3] < 0 or not 0 <= args[2] <= 7 or not 0 <= args[4] <= 7:
        raise MrdisError(f'cc_clean: thresholds >= 0 and labels in 0 .. 7, got min_voxels={min_voxels} et_label={et_label} '
                         f'et_min_voxels={et_min_voxels} et_replace={et_replace}')
    out = torch.empty((B, H, W, D), dtype=torch.uint8, device=labels.device)
    stats = torch.empty((B, 6), dtype=torch.int32, device=labels.device)
    nws = _ws_bytes(lib.mrdis_cc_clean_workspace, B)
    ws = _ws(nws, labels.device)
    _chk(lib.mrdis_cc_clean(_ptr(labels), _ptr(comp), _ptr(size), *args, _ptr(out), _ptr(stats), _ptr(ws), nws, B, H, W, D, _stream()), 'cc_clean')
    return out, stats


def synth_accum(recons, centres, acc, cnt, c_lo, c_hi):
    """acc[k] += every prediction of plane k the batch holds in channels c_lo .. c_hi, cnt[k] += their number (include/mrdis.h mrdis_synth_accum),
    in place; returns acc.  recons: 1 .. 8 fp32 (B, C, H, W) dense channels-last reconstructions of one target, one per source, in the order they
    add; centres: the B centre slices of the samples (host integers), which must be consecutive; acc (D, H, W) fp32 and cnt (D,) int32
    contiguous on the same device.  Any other layout raises MrdisError: nothing is copied."""
    lib = load()
    recons = list(recons)
    if not 1 <= len(recons) <= SYNTH_MAX_SRC:
        raise MrdisError(f'synth_accum: 1 to {SYNTH_MAX_SRC} sources, got {len(recons)}')
    B, C, H, W = _want(recons[0], 'synth_accum: every source', torch.float32, ('B', 'C', 'H', 'W'), acc.device, cl=True)
    for x in recons[1:]:
        _want(x, 'synth_accum: every source', torch.float32, (B, C, H, W), acc.device, cl=True)
    centres = [int(c) for c in centres]
    if len(centres) != B or any(centres[r] != centres[0] + r for r in range(B)):
        raise MrdisError(f'synth_accum: the {B} samples need consecutive centre slices, got {centres}')
    D = _want(acc, 'synth_accum: acc', torch.float32, ('D', H, W))[0]
    _want(cnt, 'synth_accum: cnt', torch.int32, (D,), acc.device)
    ptrs = (_c.c_void_p * len(recons))(*[x.data_ptr() for x in recons])
    _chk(lib.mrdis_synth_accum(ptrs, len(recons), _ptr(acc), _ptr(cnt), B, C, H, W, D, centres[0], int(c_lo), int(c_hi), _stream()), 'synth_accum')
    return acc


def synth_finish(acc, cnt, fill=0.0):
    """acc (D, H, W) becomes acc / cnt[d] in place (`fill` where cnt[d] == 0; include/mrdis.h mrdis_synth_finish) -> (acc, the same volume as a new
    contiguous (H, W, D) tensor, the volume store's layout).  acc fp32 and cnt (D,) int32 contiguous on one device, else MrdisError."""
    lib = load()
    D, H, W = _want(acc, 'synth_finish: acc', torch.float32, ('D', 'H', 'W'))
    _want(cnt, 'synth_finish: cnt', torch.int32, (D,), acc.device)
    out = torch.empty((H, W, D), dtype=torch.float32, device=acc.device)
    _chk(lib.mrdis_synth_finish(_ptr(acc), _ptr(cnt), _ptr(out), D, H, W, float(fill), _stream()), 'synth_finish')
    return acc, out


PREP_DTYPES = {torch.uint8: 2, torch.int16: 4, torch.int32: 8, torch.float32: 16, torch.float64: 64, torch.uint16: 512}     # include/mrdis.h MRDIS_PREP_U8 ...: the NIfTI-1 datatype codes
PREP_KINDS = ('zscore', 'mean', 'label')          # MRDIS_PREP_ZSCORE | _MEAN | _LABEL, in this order
PREP_LAYOUTS = ('dhw', 'hwd')                     # MRDIS_PREP_DHW | _HWD, in this order
PREP_ORDERS = ('file', 'c')                       # raw is (D, W, H) as a NIfTI file holds it | (H, W, D)
PREP_MAX_EXTENT = 1024                            # each of H, W, D


def _prep_view(raw, crop, order, what):
    """-> (dtype code, (stride_h, stride_w, stride_d), (H, W, D), (h0, h1, w0, w1)) of a raw device volume; MrdisError for anything the kernels do not
    take, 'unsupported geometry' for extents and crops outside include/mrdis.h's limits."""
    if not isinstance(raw, torch.Tensor) or raw.dim() != 3 or raw.dtype not in PREP_DTYPES or not raw.is_cuda:
        raise MrdisError(f'{what}: raw must be a 3-D device tensor of dtype uint8, int16, uint16, int32, float32 or float64, {_got(raw)}')
    if order not in PREP_ORDERS:
        raise MrdisError(f'{what}: order {order!r}: one of {PREP_ORDERS}')
    (H, W, D), (sh, sw, sd) = (raw.shape[::-1], raw.stride()[::-1]) if order == 'file' else (raw.shape, raw.stride())
    h0, h1, w0, w1 = _crop(crop, what)
    if min(sh, sw, sd) < 1:
        raise MrdisError(f'{what}: raw needs positive strides, got {raw.stride()}')
    if not (1 <= min(H, W, D) and max(H, W, D) <= PREP_MAX_EXTENT and H * W * D < 2 ** 31 and min(h0, h1, w0, w1) >= 0 and h0 + h1 < H and w0 + w1 < W):
        raise MrdisError(f'{what}: unsupported geometry: (H, W, D) = {(H, W, D)} with crop {((h0, h1), (w0, w1))}; each extent in 1 .. {PREP_MAX_EXTENT}, '
                         f'H W D < 2^31, and the crop must leave at least one voxel per axis')
    return PREP_DTYPES[raw.dtype], (sh, sw, sd), (H, W, D), (h0, h1, w0, w1)


def prep_stats(raw, crop, slope=1.0, inter=0.0, order='file', inner=(50, 50)):
    """(5,) float64 device tensor (n, sum, ssd, vmax, nan_inner) of a raw volume (include/mrdis.h mrdis_prep_stats): n, sum and ssd over the volume
    cropped by crop = ((h0, h1), (w0, w1)), vmax and the NaN count of the planes [inner[0], D - inner[1]) over the whole one.  raw: a device tensor in
    the file's order (D, W, H) (order 'file') or (H, W, D) (order 'c'), any strides.  No host read."""
    lib = load()
    code, strides, (H, W, D), cr = _prep_view(raw, crop, order, 'prep_stats')
    d_lo, d_hi = int(inner[0]), int(inner[1])
    stats = torch.empty(5, dtype=torch.float64, device=raw.device)
    nws = int(lib.mrdis_prep_workspace(H, W, D))
    ws = _ws(nws, raw.device)
    _chk(lib.mrdis_prep_stats(_ptr(raw), code, *strides, H, W, D, *cr, d_lo, d_hi, float(slope), float(inter), _ptr(stats), _ptr(ws), nws, _stream()), 'prep_stats')
    return stats


def prep_write(raw, stats, kind, crop, layout, slope=1.0, inter=0.0, order='file', out=None):
    """the fp32 store volume of a raw one (include/mrdis.h mrdis_prep_write): kind 'zscore' | 'mean' | 'label', layout 'dhw' -> (D, H', W') (VolumeStore) |
    'hwd' -> (H', W', D) (VolumeStore3D); stats: what prep_stats gave for the same raw, crop, slope and inter, read on the device.  `out`: a contiguous
    fp32 tensor of that shape to write into.  No host read."""
    lib = load()
    code, strides, (H, W, D), cr = _prep_view(raw, crop, order, 'prep_write')
    if kind not in PREP_KINDS or layout not in PREP_LAYOUTS:
        raise MrdisError(f'prep_write: kind {kind!r} must be one of {PREP_KINDS} and layout {layout!r} one of {PREP_LAYOUTS}')
    _want(stats, 'prep_write: stats', torch.float64, (5,), raw.device)
    Hc, Wc = H - cr[0] - cr[1], W - cr[2] - cr[3]
    shape = (D, Hc, Wc) if layout == 'dhw' else (Hc, Wc, D)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=raw.device)
    else:
        _want(out, 'prep_write: out', torch.float32, shape, raw.device)
    _chk(lib.mrdis_prep_write(_ptr(raw), code, *strides, H, W, D, *cr, float(slope), float(inter), _ptr(stats), PREP_KINDS.index(kind),
                              PREP_LAYOUTS.index(layout), _ptr(out), _stream()), 'prep_write')
    return out


EXPORT_KINDS = ('copy', 'unzscore', 'unmean')     # MRDIS_EXPORT_COPY | _UNZSCORE | _UNMEAN, in this order
EXPORT_SRC_DTYPES = (torch.uint8, torch.float32)
EXPORT_DST_DTYPES = (torch.uint8, torch.int16, torch.float32)
EXPORT_MAX_B = 65535


def export_volume(src, crop, layout, kind='copy', stats=None, fill=0.0, dtype=torch.uint8, out=None):
    """store volumes back in a NIfTI file's order, on the canvas the crop was cut from (include/mrdis.h mrdis_export_volume): the inverse of prep_write.
    src: a device volume or a (B, ...) stack of them, uint8 or fp32, (H', W', D) each for layout 'hwd' or (D, H', W') for 'dhw'; a non-contiguous one is
    copied.  -> (D, W, H) or (B, D, W, H) of `dtype` (uint8 | int16 | float32) with H = H' + h0 + h1, W = W' + w0 + w1 for crop = ((h0, h1), (w0, w1)):
    `fill` outside the crop; inside the source voxel (kind 'copy'), s (std + 1e-8) + norm with -10 -> 0 ('unzscore') or s norm ('unmean') in float64,
    converted once (integers: NaN -> 0, ties to even, clamped).  stats: what prep_stats gave, (5,) for every volume or (B, 5), read on the device.
    `out`: a dense tensor of the result's shape and dtype to write into (it may start at any element of a larger buffer).  One launch whatever B, no
    host read.  What the entry point refuses raises MrdisError('... unsupported geometry ...') before any launch."""
    lib = load()
    if not isinstance(src, torch.Tensor) or src.dim() not in (3, 4) or not src.is_cuda:
        raise MrdisError(f'export_volume: src must be a 3-D device volume or a 4-D stack of them, {_got(src)}')
    h0, h1, w0, w1 = _crop(crop, 'export_volume')
    stacked = src.dim() == 4
    B = src.shape[0] if stacked else 1
    vol = tuple(src.shape[1:]) if stacked else tuple(src.shape)
    D, Hc, Wc = vol if layout == 'dhw' else (vol[2], vol[0], vol[1])
    H, W = Hc + h0 + h1, Wc + w0 + w1
    why = None
    if layout not in PREP_LAYOUTS or kind not in EXPORT_KINDS or src.dtype not in EXPORT_SRC_DTYPES or dtype not in EXPORT_DST_DTYPES:
        why = (f'layout {layout!r} must be one of {PREP_LAYOUTS}, kind {kind!r} one of {EXPORT_KINDS}, the source uint8 or float32 (got {src.dtype}) '
               f'and the destination uint8, int16 or float32 (got {dtype})')
    elif src.dtype == torch.uint8 and kind != 'copy':
        why = f'a uint8 source takes kind copy only, got {kind!r}'
    elif kind != 'copy' and stats is None:
        why = f'kind {kind!r} reads stats, got None'
    elif not (min(h0, h1, w0, w1) >= 0 and 1 <= min(Hc, Wc, D) and max(H, W, D) <= PREP_MAX_EXTENT and H * W * D < 2 ** 31 and 1 <= B <= EXPORT_MAX_B):
        why = (f'each of H\', W\', D, H, W in 1 .. {PREP_MAX_EXTENT}, H W D < 2^31, B in 1 .. {EXPORT_MAX_B} and no negative crop')
    if why:
        raise MrdisError(f'export_volume: unsupported geometry: B = {B}, (H\', W\', D) = {(Hc, Wc, D)} with crop {((h0, h1), (w0, w1))}: {why}')
    if stats is not None and kind != 'copy':
        if not isinstance(stats, torch.Tensor) or stats.dtype != torch.float64 or stats.device != src.device or tuple(stats.shape) not in ((5,), (1, 5), (B, 5)):
            raise MrdisError(f'export_volume: stats must be a (5,) or ({B}, 5) float64 tensor of prep_stats on {src.device}')
        stats = stats.reshape(-1, 5).expand(B, 5).contiguous()
    else:
        stats = None
    shape = (B, D, W, H) if stacked else (D, W, H)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=src.device)
    else:
        _want(out, 'export_volume: out', dtype, shape, src.device)
    src = src.contiguous()
    rc = lib.mrdis_export_volume(_ptr(src), PREP_DTYPES[src.dtype], PREP_LAYOUTS.index(layout), Hc, Wc, D, h0, h1, w0, w1, B, EXPORT_KINDS.index(kind),
                                 _ptr(stats), float(fill), _ptr(out), PREP_DTYPES[dtype], _stream())
    if rc == -2:        # MRDIS_EUNSUPPORTED: the entry point's list is the authority; the checks above only have to come before the allocation of `out`
        raise MrdisError(f'export_volume: unsupported geometry: B = {B}, (H\', W\', D) = {(Hc, Wc, D)} with crop {((h0, h1), (w0, w1))}')
    _chk(rc, 'export_volume')
    return out


def seg2d_label_planes(views, flips, planes, s0, relabel=False):
    """planes[s][s0 + r] = the label plane of sample r of set s (include/mrdis.h mrdis_seg2d_label_planes), in place; returns planes.  views: 1 .. 16
    sets (one per missing-contrast pattern), each a list of 1 .. 2 view tensors: fp32 (B, C, H, W) dense channels-last logits, 2 <= C <= 4, of B
    samples with consecutive centres s0, s0 + 1, ...; flips: one code per view, 0 | 1 (H) | 2 (W): the view is the prediction of an input flipped
    along that axis.  One view: argmax of the logits; two: argmax of the mean of the two softmaxes; the lowest class on a tie; relabel: 3 -> 4.
    planes (n_sets, D, H, W) uint8 contiguous on the same device: only planes s0 .. s0 + B - 1 are written.  This package's own convention (the
    reference assembles no volume).  Any other layout raises MrdisError: nothing is copied."""
    lib = load()
    views = [list(v) for v in views]
    flips = [int(f) for f in flips]
    if not 1 <= len(views) <= SEG2D_MAX_SETS:
        raise MrdisError(f'seg2d_label_planes: 1 to {SEG2D_MAX_SETS} sets, got {len(views)}')
    n_views = len(views[0])
    if not 1 <= n_views <= SEG2D_MAX_VIEWS or any(len(v) != n_views for v in views) or len(flips) != n_views:
        raise MrdisError(f'seg2d_label_planes: 1 to {SEG2D_MAX_VIEWS} views per set and one flip code per view, got {[len(v) for v in views]} views, '
                         f'{len(flips)} codes')
    if any(f not in (0, 1, 2) for f in flips):
        raise MrdisError(f'seg2d_label_planes: flip codes 0 (none), 1 (H) or 2 (W), got {flips}')
    B, C, H, W = _want(views[0][0], 'seg2d_label_planes: every view', torch.float32, ('B', 'C', 'H', 'W'), planes.device, cl=True)
    if not 2 <= C <= 4:
        raise MrdisError(f'seg2d_label_planes: (B, C, H, W) logits with 2 <= C <= 4 wanted, got {(B, C, H, W)}')
    for x in (x for v in views for x in v):
        _want(x, 'seg2d_label_planes: every view', torch.float32, (B, C, H, W), planes.device, cl=True)
    D, s0 = _want(planes, 'seg2d_label_planes: planes', torch.uint8, (len(views), 'D', H, W))[1], int(s0)
    if s0 < 0 or s0 + B > D:
        raise MrdisError(f'seg2d_label_planes: planes {s0} .. {s0 + B - 1} are outside a volume of {D}')
    ptrs = (_c.c_void_p * (len(views) * n_views))(*[x.data_ptr() for v in views for x in v])
    codes = (_c.c_int * n_views)(*flips)
    _chk(lib.mrdis_seg2d_label_planes(ptrs, len(views), n_views, codes, _ptr(planes), B, C, H, W, D, s0, int(bool(relabel)), _stream()),
         'seg2d_label_planes')
    return planes


def seg2d_finish(planes):
    """(n_sets, D, H, W) uint8 label planes -> the same volumes as a new contiguous (n_sets, H, W, D) tensor, the volume store's layout
    (include/mrdis.h mrdis_seg2d_finish).  planes contiguous uint8, else MrdisError.  This package's own convention, like the label planes: the
    reference assembles no volume."""
    lib = load()
    S, D, H, W = _want(planes, 'seg2d_finish: planes', torch.uint8, ('n_sets', 'D', 'H', 'W'))
    if planes.numel() == 0: _refuse('seg2d_finish', 'arg', planes)
    out = torch.empty((S, H, W, D), dtype=torch.uint8, device=planes.device)
    _chk(lib.mrdis_seg2d_finish(_ptr(planes), _ptr(out), S, D, H, W, _stream()), 'seg2d_finish')
    return out


def _nhwc_on(t, device, shape, what, out=False):
    """(view, ld) of an fp32 operand of a cold wrapper, of that (B, C, H, W) on that device: NHWC memory or a channel slice of it (else an input is copied, an output refused)"""
    if not isinstance(t, torch.Tensor) or t.dtype is not torch.float32 or t.dim() != 4 or t.device != device or tuple(t.shape) != shape: _refuse(f'{what} on {device}', 'like dtype', t, shape)
    return _out_view(t) if out else nhwc(t)


def _fuse_args(what, srcs, mask, method):
    """the checks mrdis_fuse_present_fwd / _bwd share: -> (views, pixel strides, mask, method code, B, C, H, W).  Raises before the library is touched."""
    srcs = list(srcs)
    if method not in FUSE_METHODS:
        raise MrdisError(f'{what}: method {method!r} is not one of {FUSE_METHODS}')
    if not 1 <= len(srcs) <= FUSE_MAX_SRC:
        raise MrdisError(f'{what}: 1 to {FUSE_MAX_SRC} maps, got {len(srcs)}')
    x0 = srcs[0]
    views = [_nhwc_on(x, x0.device, tuple(x0.shape), f'{what}: every map') for x in srcs]
    B, C, H, W = x0.shape
    _want(mask, f'{what}: mask', torch.float32, (B, len(srcs)), x0.device)
    return [v for v, _ in views], [ld for _, ld in views], mask, FUSE_METHODS.index(method), B, C, H, W


def _view_table(ts, lds):
    return (_c.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), (_c.c_int * len(ts))(*lds)


def fuse_present_fwd(srcs, mask, method, out=None):
    """the K fp32 NHWC maps `srcs` (B, C, H, W) fused per sample over the contrasts with mask[b, k] == 1 (include/mrdis.h mrdis_fuse_present_fwd):
    'mean' | 'max' -> (B, C, H, W); 'mean-max-min' -> (B, 3 C, H, W) = [mean | max | min].  mask: (B, K) fp32 on the device; the kernel reads it
    there.  out: an NHWC view to write into (a channel slice of a wider buffer qualifies); default a new channels-last tensor.  One launch."""
    xs, lds, mask, code, B, C, H, W = _fuse_args('fuse_present_fwd', srcs, mask, method)
    F = 3 if code == 2 else 1
    y, ldy = _nhwc_on(empty_nhwc(B, F * C, H, W, xs[0].device) if out is None else out, xs[0].device, (B, F * C, H, W), 'fuse_present_fwd: out', out=True)
    ptrs, ldarr = _view_table(xs, lds)
    _chk(load().mrdis_fuse_present_fwd(ptrs, ldarr, len(xs), _ptr(mask), code, _ptr(y), ldy, B, H * W, C, _stream()), 'fuse_present_fwd')
    return y


def fuse_present_bwd(dout, srcs, mask, method, outs=None):
    """-> the K gradients of fuse_present_fwd's maps (include/mrdis.h mrdis_fuse_present_bwd): zeros for an absent contrast, g / n_b for the mean,
    g to the lowest present index that attains the max / the min (recomputed from the maps).  outs: K NHWC views to write into.  One launch."""
    xs, lds, mask, code, B, C, H, W = _fuse_args('fuse_present_bwd', srcs, mask, method)
    F = 3 if code == 2 else 1
    dout, lddo = _nhwc_on(dout, xs[0].device, (B, F * C, H, W), 'fuse_present_bwd: dout')
    if outs is None:
        outs = [empty_nhwc(B, C, H, W, dout.device) for _ in xs]
    if len(outs) != len(xs):
        raise MrdisError(f'fuse_present_bwd: {len(xs)} maps, {len(outs)} gradient views')
    dviews = [_nhwc_on(t, dout.device, (B, C, H, W), 'fuse_present_bwd: every gradient view', out=True) for t in outs]
    ptrs, ldarr = _view_table(xs, lds)
    dptrs, dldarr = _view_table([d for d, _ in dviews], [ld for _, ld in dviews])
    _chk(load().mrdis_fuse_present_bwd(_ptr(dout), lddo, ptrs, ldarr, len(xs), _ptr(mask), code, dptrs, dldarr, B, H * W, C, _stream()),
         'fuse_present_bwd')
    return [d for d, _ in dviews]


def recon_err_bwd(gt, x, w, p):
    lib = load()
    gt, ldgt = nhwc(gt); x, ldx = nhwc(x)
    N, C, H, W = x.shape
    if gt.shape != x.shape or not (gt.dtype is x.dtype is w.dtype is torch.float32) or w.numel() != N: _refuse('recon_err_bwd', 'like dtype', gt, x, w)
    dx = empty_nhwc(N, C, H, W, x.device)
    w = w.contiguous()
    _chk(lib.mrdis_recon_err_bwd(_ptr(gt), ldgt, _ptr(x), ldx, _ptr(w), _ptr(dx), C, N, H * W, C, p, _stream()), 'recon_err_bwd')
    return dx


def maxpool_fwd(x, k):
    lib = load()
    x, ldx = nhwc(x)
    N, C, H, W = x.shape
    if x.dtype is not torch.float32 or k < 1: _refuse('maxpool_fwd', 'dtype arg', x)
    y = empty_nhwc(N, C, H // k, W // k, x.device)
    arg = torch.empty((N, H // k, W // k, C), dtype=torch.int32, device=x.device)
    _chk(lib.mrdis_maxpool_fwd(_ptr(x), ldx, _ptr(y), _ptr(arg), N, H, W, C, k, _stream()), 'maxpool_fwd')
    return y, arg


def maxpool_bwd(dy, arg, in_shape, k):
    lib = load()
    N, C, H, W = in_shape
    dy, lddy = nhwc(dy)
    if (dy.dtype is not torch.float32 or k < 1 or tuple(dy.shape) != (N, C, H // k, W // k)
            or arg.dtype is not torch.int32 or arg.numel() != dy.numel() or not arg.is_contiguous()): _refuse('maxpool_bwd', 'like dtype dense arg', dy, arg)
    if lddy != C:
        dy = dy.contiguous(memory_format=torch.channels_last)
    dx = empty_nhwc(N, C, H, W, dy.device)
    _chk(lib.mrdis_maxpool_bwd(_ptr(dy), _ptr(arg), _ptr(dx), C, N, H, W, C, k, _stream()), 'maxpool_bwd')
    return dx


# ---------------------------------------------------------------- optimizer arena
def sumsq_finite(g, out):
    lib = load()
    if not (g.dtype is out.dtype is torch.float32) or out.numel() < 2 or not (g.is_contiguous() and out.is_contiguous()): _refuse('sumsq_finite', 'vec dtype dense', g, out)
    nb = _ws_bytes(lib.mrdis_sumsq_workspace)
    ws = _ws(nb, g.device)
    _chk(lib.mrdis_sumsq_finite(_ptr(g), g.numel(), _ptr(out), _ptr(ws), nb, _stream()), 'sumsq_finite')


def adam_amsgrad_step(p, g, m, v, vmax, lr, beta1, beta2, eps, weight_decay, step, norm_finite, max_norm, grad_scale=1.0,
                      step_state=None, gates=None, gate_steps=None):
    """step: 1-based host count, ignored when `step_state` (device float[2]: applied, skipped) is given.
    gates: (ranges [(lo, hi), ...], flag_index [...], flags device tensor) or None.
    gate_steps: device float[3 * n_flags] per-flag step counters (+ scratch), see include/mrdis.h."""
    lib = load()
    n = p.numel()
    ranges, fidx, flags = gates if gates is not None and len(gates[0]) else ((), (), None)
    n_g = len(ranges)
    if not (n_g and gate_steps is not None):
        gate_steps = None
    n_flags = 0 if gate_steps is None else gate_steps.numel() // 3
    for t, size in ((p, n), (g, n), (m, n), (v, n), (vmax, n), (step_state, 2), (norm_finite, 2), (flags, max(fidx, default=-1) + 1), (gate_steps, 3 * n_flags)):
        if t is not None and (t.dtype is not torch.float32 or t.numel() < size or (size == n and t.numel() != n) or not t.is_contiguous()): _refuse('adam_amsgrad_step', 'vec dtype dense', t)
    if (len(fidx) != n_g or any(not 0 <= int(lo) <= int(hi) <= n for lo, hi in ranges) or min(fidx, default=0) < 0
            or (gate_steps is not None and (step_state is None or max(fidx) >= n_flags))): _refuse('adam_amsgrad_step', 'arg', list(ranges), list(fidx), step_state, gate_steps)
    ra = (_c.c_longlong * (2 * n_g))(*[int(x) for r in ranges for x in r]) if n_g else None
    fa = (_c.c_int * n_g)(*[int(i) for i in fidx]) if n_g else None
    fl = flags.data_ptr() if n_g else None
    _chk(lib.mrdis_adam_amsgrad_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(vmax), p.numel(), lr, beta1, beta2, eps, weight_decay,
                                     int(step), _ptr(step_state), _ptr(norm_finite), max_norm, grad_scale, ra, fa, n_g, fl, _ptr(gate_steps), n_flags, _stream()),
         'adam_amsgrad_step')


# ================================================================ 3-D path (NDHWC, torch.channels_last_3d)
def ndhwc_ld(t):
    """pixel stride (elements) of a logical (N,C,D,H,W) tensor whose memory is NDHWC -- dense or a channel slice of a wider buffer -- else None"""
    N, C, D, H, W = t.shape
    s = t.stride()
    ld = s[4] if W > 1 else (s[3] if H > 1 else (s[2] if D > 1 else (s[0] if N > 1 else C)))
    ok = (ld >= C and (C == 1 or s[1] == 1) and (W == 1 or s[4] == ld) and (H == 1 or s[3] == W * ld) and
          (D == 1 or s[2] == H * W * ld) and (N == 1 or s[0] == D * H * W * ld))
    return ld if ok else None


def ndhwc(t, keep_slice=False):
    """(tensor, ld) of a logical (N,C,D,H,W) fp32 tensor stored NDHWC (channels_last_3d); copies if it is not.
    keep_slice: a channel slice of a wider NDHWC buffer goes through as it is, with its pixel stride as ld (no copy)."""
    if t.dim() != 5 or t.dtype is not torch.float32: _refuse('ndhwc', 'dtype', t)
    N, C, D, H, W = t.shape
    if keep_slice:
        ld = ndhwc_ld(t)
        if ld is not None:
            return t, ld
    want = (D * H * W * C, 1, H * W * C, W * C, C)
    if any(t.shape[i] > 1 and t.stride()[i] != want[i] for i in range(5)):
        t = t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    return t, C


def empty_ndhwc(N, C, D, H, W, device):
    return torch.empty((N, D, H, W, C), dtype=torch.float32, device=device).permute(0, 4, 1, 2, 3)


def _out3(D, H, W, k, stride, pad):
    return tuple((v + 2 * pad - k) // stride + 1 for v in (D, H, W))


def _out_view3(out, shape, what):
    """(out, ld) of a caller's output view: NDHWC, dense or a channel slice of a wider buffer (written in place, never copied)"""
    ld = ndhwc_ld(out) if out.dtype is torch.float32 and tuple(out.shape) == shape else None
    if ld is None: _refuse(what, 'out dtype', out)
    return out, ld


def conv3d_fwd(x, w_tck, bias, k, stride, pad, residual=None, out=None, keep_slices=False):
    """out: an NDHWC view to write (e.g. a channel slice of a wider buffer, passed with its ld); keep_slices: x / residual channel slices go
    in with their ld instead of as dense copies"""
    x, ldx = ndhwc(x, keep_slices)
    N, Ci, D, H, W = x.shape
    Co = w_tck.shape[-1]
    if (tuple(w_tck.shape) != (k * k * k, Ci, Co) or w_tck.dtype is not torch.float32
            or not w_tck.is_contiguous() or (bias is not None and bias.numel() != Co)): _refuse('conv3d_fwd', 'filter vec dtype dense', w_tck, bias)
    Do, Ho, Wo = _out3(D, H, W, k, stride, pad)
    if out is None:
        y, ldy = empty_ndhwc(N, Co, Do, Ho, Wo, x.device), Co
    else:
        y, ldy = _out_view3(out, (N, Co, Do, Ho, Wo), 'conv3d_fwd')
    ldr = 0
    if residual is not None:
        residual, ldr = ndhwc(residual, keep_slices)
        if residual.shape != y.shape: _refuse('conv3d_fwd', 'like', residual)
    _chk(load().mrdis_conv3d_fwd(x.data_ptr(), ldx, w_tck.data_ptr(), _ptr(bias), _ptr(residual), ldr, y.data_ptr(), ldy,
                                 N, D, H, W, Ci, Co, k, stride, pad, _stream()), 'conv3d_fwd')
    return y


def conv3d_bwd_data(dy, w_tkc, in_shape, k, stride, pad, out=None, keep_slices=False):
    """out / keep_slices: as conv3d_fwd (dx into a caller's NDHWC view; a dy channel slice with its ld)"""
    dy, lddy = ndhwc(dy, keep_slices)
    N, Ci, D, H, W = in_shape
    Co = dy.shape[1]
    if (tuple(w_tkc.shape) != (k * k * k, Co, Ci) or w_tkc.dtype is not torch.float32 or not w_tkc.is_contiguous()
            or (dy.shape[0],) + tuple(dy.shape[2:]) != (N,) + _out3(D, H, W, k, stride, pad)): _refuse('conv3d_bwd_data', 'layer filter dtype dense', w_tkc, dy)
    if out is None:
        dx, lddx = empty_ndhwc(N, Ci, D, H, W, dy.device), Ci
    else:
        dx, lddx = _out_view3(out, (N, Ci, D, H, W), 'conv3d_bwd_data')
    _chk(load().mrdis_conv3d_bwd_data(dy.data_ptr(), lddy, w_tkc.data_ptr(), dx.data_ptr(), lddx,
                                      N, D, H, W, Ci, Co, k, stride, pad, _stream()), 'conv3d_bwd_data')
    return dx


def conv3d_bwd_weight(x, dy, k, stride, pad, want_bias, out=None, keep_slices=False):
    """out: caller-owned (dw [k^3][Ci][Co] contiguous, db [Co] or None) to write; keep_slices: x / dy channel slices with their ld"""
    x, ldx = ndhwc(x, keep_slices)
    dy, lddy = ndhwc(dy, keep_slices)
    N, Ci, D, H, W = x.shape
    Co = dy.shape[1]
    if (dy.shape[0],) + tuple(dy.shape[2:]) != (N,) + _out3(D, H, W, k, stride, pad): _refuse('conv3d_bwd_weight', 'layer', x, dy)
    lib = load()
    need = lib.mrdis_conv3d_bwd_weight_workspace(N, D, H, W, Ci, Co, k, stride, pad)
    if need == 0:
        raise MrdisError('conv3d_bwd_weight: unsupported geometry')
    ws = _ws(need, x.device)
    if out is None:
        dw = torch.empty((k * k * k, Ci, Co), dtype=torch.float32, device=x.device)
        db = torch.empty((Co,), dtype=torch.float32, device=x.device) if want_bias else None
    else:
        dw, db = out
        if (tuple(dw.shape) != (k * k * k, Ci, Co) or (db is not None) != bool(want_bias) or dw.dtype is not torch.float32 or not dw.is_contiguous()
                or (db is not None and (db.dtype is not torch.float32 or db.numel() != Co or not db.is_contiguous()))): _refuse('conv3d_bwd_weight', 'out dtype dense', dw, db)
    _chk(lib.mrdis_conv3d_bwd_weight(x.data_ptr(), ldx, dy.data_ptr(), lddy, dw.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel(),
                                     N, D, H, W, Ci, Co, k, stride, pad, _stream()), 'conv3d_bwd_weight')
    return dw, db


def groupnorm_relu_fwd(x, gamma, beta, G, eps, relu):
    x, ld = ndhwc(x)
    N, C, D, H, W = x.shape
    if G < 1 or C % G != 0 or gamma.numel() != C or beta.numel() != C or not (gamma.dtype is beta.dtype is torch.float32): _refuse('groupnorm_relu_fwd', 'vec dtype arg', gamma, beta)
    P = D * H * W
    y = empty_ndhwc(N, C, D, H, W, x.device)
    mean = torch.empty((N, G), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    lib = load()
    ws = _ws(lib.mrdis_groupnorm_workspace(N, P, C, G), x.device)
    _chk(lib.mrdis_groupnorm_relu_fwd(x.data_ptr(), ld, y.data_ptr(), C, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), ws.data_ptr(), ws.numel(), N, P, C, G, eps, int(relu), _stream()), 'groupnorm_relu_fwd')
    return y, mean, rstd


def groupnorm_relu_bwd(dy, x, gamma, beta, mean, rstd, G, relu, add=None):
    """add: a second gradient of x (same shape), summed into dx by the same pass (include/mrdis.h mrdis_groupnorm_relu_bwd_add)"""
    x, ld = ndhwc(x)
    dy, lddy = ndhwc(dy)
    ldadd = 0
    if add is not None:
        add, ldadd = ndhwc(add)
    N, C, D, H, W = x.shape
    if (dy.shape != x.shape or (add is not None and add.shape != x.shape) or G < 1 or C % G != 0 or not (gamma.dtype is beta.dtype is mean.dtype is rstd.dtype is torch.float32)
            or gamma.numel() != C or beta.numel() != C or mean.numel() != N * G or rstd.numel() != N * G): _refuse('groupnorm_relu_bwd', 'like vec dtype arg', dy, x, add, gamma, beta, mean, rstd)
    P = D * H * W
    dx = empty_ndhwc(N, C, D, H, W, x.device)
    dgamma = torch.empty((C,), dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    lib = load()
    ws = _ws(lib.mrdis_groupnorm_workspace(N, P, C, G), x.device)
    _chk(lib.mrdis_groupnorm_relu_bwd_add(dy.data_ptr(), lddy, x.data_ptr(), ld, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                          rstd.data_ptr(), dx.data_ptr(), C, dgamma.data_ptr(), dbeta.data_ptr(), _ptr(add), ldadd, ws.data_ptr(), ws.numel(),
                                          N, P, C, G, int(relu), _stream()), 'groupnorm_relu_bwd')
    return dx, dgamma, dbeta


def upsample2x_add_fwd(x, skip):
    x, _ = ndhwc(x)
    N, C, D, H, W = x.shape
    if skip is not None:
        skip, _ = ndhwc(skip)
        if tuple(skip.shape) != (N, C, 2 * D, 2 * H, 2 * W): _refuse('upsample2x_add_fwd', 'arg', skip)
    y = empty_ndhwc(N, C, 2 * D, 2 * H, 2 * W, x.device)
    _chk(load().mrdis_upsample2x_add_fwd(x.data_ptr(), _ptr(skip), y.data_ptr(), N, D, H, W, C, _stream()), 'upsample2x_add_fwd')
    return y


def upsample2x_bwd(dy):
    dy, _ = ndhwc(dy)
    N, C, D2, H2, W2 = dy.shape
    if D2 % 2 or H2 % 2 or W2 % 2: _refuse('upsample2x_bwd', 'arg', dy)
    dx = empty_ndhwc(N, C, D2 // 2, H2 // 2, W2 // 2, dy.device)
    _chk(load().mrdis_upsample2x_bwd(dy.data_ptr(), dx.data_ptr(), N, D2 // 2, H2 // 2, W2 // 2, C, _stream()), 'upsample2x_bwd')
    return dx


# ---------------------------------------------------------------- nearest-neighbour modality-code search
_ZS_WS = {}       # (device, raw stream) -> zero-initialised workspace of mrdis_cosine_top1 (its arrival counter must start at 0; every launch leaves it 0)


def cosine_top1(gallery, gallery_label, query, query_label):
    """For each query row: the gallery row of highest cosine (reference compute_cosine, model.py:3407-3415) among the rows whose label differs
    from the query's; equal cosines -> the smaller index.  gallery (N, D) fp32 with unit column stride (row stride >= D), query (Q <= 64, D),
    labels int32 on the device.  Returns (idx (Q,) int32, cos (Q,) fp32); a query with every row excluded gets -1 / -inf (include/mrdis.h)."""
    if not isinstance(gallery, torch.Tensor) or gallery.dtype is not torch.float32 or gallery.dim() != 2: _refuse('cosine_top1', 'dtype', gallery)
    N, D = gallery.shape
    if gallery.stride(1) != 1 or gallery.stride(0) < D:
        gallery = gallery.contiguous()
    dev = gallery.device
    Q = _want(query, 'cosine_top1: query', torch.float32, ('Q', D), dev, dense=False)[0]
    _want(gallery_label, 'cosine_top1: gallery_label', torch.int32, (N,), dev, dense=False)
    _want(query_label, 'cosine_top1: query_label', torch.int32, (Q,), dev, dense=False)
    if not 1 <= Q <= 64: _refuse('cosine_top1: 1 .. 64 queries', 'arg', query)
    query, query_label, gallery_label = query.contiguous(), query_label.contiguous(), gallery_label.contiguous()
    lib = load()
    nb = _ws_bytes(lib.mrdis_cosine_top1_workspace, N, D, Q)
    if nb == 0:
        raise MrdisError(f'cosine_top1: unsupported geometry N={N} D={D} Q={Q}')
    key = (dev, _stream())
    ws = _ZS_WS.get(key)
    if ws is None or ws.numel() < nb:
        ws = _ZS_WS[key] = torch.zeros(max(nb, 1 << 16), dtype=torch.uint8, device=dev)
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    cos = torch.empty(Q, dtype=torch.float32, device=dev)
    _chk(lib.mrdis_cosine_top1(gallery.data_ptr(), gallery.stride(0), gallery_label.data_ptr(), N, D, query.data_ptr(), query_label.data_ptr(), Q,
                               idx.data_ptr(), cos.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'cosine_top1')
    return idx, cos


# ---------------------------------------------------------------- the `others` variants (csrc/mrdis_encs.hip)
def _f32_nhwc(t, what):
    if t.dtype is not torch.float32: _refuse(what, 'dtype', t)
    return nhwc(t)


def conv2d_2src_fwd(x, s, w_tck, bias, kh, kw, stride, pad, lrelu=False, out=None):
    """the layer of filter w_tck [T][Cx+Cs][Co] on cat([x, s], 1) without the concatenation: x (N,Cx,H,W), s (N,Cs,H,W) NHWC views.
    out: an NHWC view (N,Co,Ho,Wo) to write into (a channel slice of a wider buffer qualifies); default a new tensor."""
    x, ldx = _f32_nhwc(x, 'conv2d_2src_fwd x'); s, lds = _f32_nhwc(s, 'conv2d_2src_fwd s')
    N, Cx, H, W = x.shape
    Cs = s.shape[1]
    Co = w_tck.shape[-1]
    if ((s.shape[0], s.shape[2], s.shape[3]) != (N, H, W) or tuple(w_tck.shape) != (kh * kw, Cx + Cs, Co) or w_tck.dtype is not torch.float32
            or not w_tck.is_contiguous() or (bias is not None and bias.numel() != Co)): _refuse('conv2d_2src_fwd', 'filter vec dtype dense', x, s, w_tck, bias)
    Ho, Wo = conv_out_hw(H, W, kh, kw, stride, pad)
    y, ldy = _out_view(empty_nhwc(N, Co, Ho, Wo, x.device) if out is None else out, (N, Co, Ho, Wo))
    _chk(load().mrdis_conv2d_2src_fwd(_ptr(x), ldx, Cx, _ptr(s), lds, Cs, _ptr(w_tck), _ptr(bias), _ptr(y), ldy, N, H, W, Co, kh, kw, stride, pad,
                                      1 if lrelu else 0, _stream()), 'conv2d_2src_fwd')
    return y


def conv2d_2src_bwd_data(dy, w_tkc, Cx, Cs, in_hw, kh, kw, stride, pad, need_dx=True, dx_out=None, ds_out=None):
    """-> (dx or None, ds): the data gradients of the two sources of conv2d_2src_fwd (dy: gradient of the pre-activation output)"""
    dy, lddy = _f32_nhwc(dy, 'conv2d_2src_bwd_data dy')
    N, Co = dy.shape[:2]
    H, W = in_hw
    if (tuple(w_tkc.shape) != (kh * kw, Co, Cx + Cs) or w_tkc.dtype is not torch.float32 or not w_tkc.is_contiguous()
            or conv_out_hw(H, W, kh, kw, stride, pad) != (dy.shape[2], dy.shape[3])): _refuse('conv2d_2src_bwd_data', 'layer filter dtype dense', w_tkc, dy)
    ds, ldds = _out_view(empty_nhwc(N, Cs, H, W, dy.device) if ds_out is None else ds_out, (N, Cs, H, W))
    dx, lddx = (None, Cx)
    if need_dx:
        dx, lddx = _out_view(empty_nhwc(N, Cx, H, W, dy.device) if dx_out is None else dx_out, (N, Cx, H, W))
    _chk(load().mrdis_conv2d_2src_bwd_data(_ptr(dy), lddy, _ptr(w_tkc), _ptr(dx), lddx, Cx, _ptr(ds), ldds, Cs, N, H, W, Co, kh, kw, stride, pad,
                                           _stream()), 'conv2d_2src_bwd_data')
    return dx, ds


def conv2d_2src_bwd_weight(x, s, dy, kh, kw, stride, pad, need_bias=True, bias_sink=None, dw_out=None):
    """-> (dw_tck [T][Cx+Cs][Co], dbias or None).  bias_sink: a (Co,) buffer the bias gradient is ADDED to (then dbias is None)."""
    x, ldx = _f32_nhwc(x, 'conv2d_2src_bwd_weight x'); s, lds = _f32_nhwc(s, 'conv2d_2src_bwd_weight s')
    dy, lddy = _f32_nhwc(dy, 'conv2d_2src_bwd_weight dy')
    N, Cx, H, W = x.shape
    Cs, Co = s.shape[1], dy.shape[1]
    if ((s.shape[0], s.shape[2], s.shape[3]) != (N, H, W)
            or (dy.shape[0], dy.shape[2], dy.shape[3]) != (N,) + conv_out_hw(H, W, kh, kw, stride, pad)): _refuse('conv2d_2src_bwd_weight', 'layer', x, s, dy)
    lib = load()
    nb = _ws_bytes(lib.mrdis_conv2d_2src_bwd_weight_workspace, N, H, W, Cx, Cs, Co, kh, kw, stride, pad)
    if nb == 0:
        raise MrdisError(f'conv2d_2src_bwd_weight: unsupported geometry Cx={Cx} Cs={Cs} Co={Co} k={kh}x{kw} stride={stride}')
    ws = _ws(nb, x.device)
    dw = torch.empty((kh * kw, Cx + Cs, Co), dtype=torch.float32, device=x.device) if dw_out is None else dw_out
    sink = bias_sink if need_bias else None
    if (dw.dtype is not torch.float32 or dw.numel() != kh * kw * (Cx + Cs) * Co or not dw.is_contiguous()
            or (sink is not None and sink.numel() != Co)): _refuse('conv2d_2src_bwd_weight', 'vec dtype dense', dw, sink)
    db = torch.empty(Co, dtype=torch.float32, device=x.device) if (need_bias and sink is None) else None
    _chk(lib.mrdis_conv2d_2src_bwd_weight(_ptr(x), ldx, Cx, _ptr(s), lds, Cs, _ptr(dy), lddy, _ptr(dw), _ptr(sink if sink is not None else db),
                                          1 if sink is not None else 0, _ptr(ws), nb, N, H, W, Co, kh, kw, stride, pad, _stream()),
         'conv2d_2src_bwd_weight')
    return dw, db


def _out_view(t, shape=None):
    """(t, ld) for an fp32 output NHWC view (of that shape, where given) that the kernel writes in place (never a silent copy)"""
    v, ld = nhwc(t)
    if v is not t or (shape is not None and (tuple(t.shape) != shape or t.dtype is not torch.float32)): _refuse('output', 'out vec dtype', t)
    return v, ld


def _act_views(what, *ts):
    """[(view, ld)] of fp32 NHWC activations that share one shape"""
    if any(t.shape != ts[0].shape for t in ts): _refuse(what, 'like', *ts)
    return [_f32_nhwc(t, what) for t in ts]


def _elementwise(entry, what, ts, out, nhw=False):
    """one element-wise pass over fp32 NHWC views of one shape -> the output view (out: an NHWC view to write into).  nhw: the entry point takes (B, H, W, C), not (pixels, C)"""
    views = _act_views(what, *ts)
    N, C, H, W = ts[0].shape
    y, ldy = _out_view(empty_nhwc(N, C, H, W, ts[0].device) if out is None else out, (N, C, H, W))
    _chk(entry(*[a for v, ld in views for a in (_ptr(v), ld)], _ptr(y), ldy, *((N, H, W, C) if nhw else (N * H * W, C)), _stream()), what)
    return y


def softplus_fwd(x, out=None):
    """F.softplus(x) (beta 1, threshold 20) over an NHWC view"""
    return _elementwise(load().mrdis_softplus_fwd, 'softplus_fwd', (x,), out)


def softplus_bwd(dy, x, out=None):
    return _elementwise(load().mrdis_softplus_bwd, 'softplus_bwd', (dy, x), out)


def softmax_fwd(s, out=None):
    """F.softmax(s, 1) over the channels of an NHWC view (C <= 8)"""
    return _elementwise(load().mrdis_softmax_fwd, 'softmax_fwd', (s,), out)


def softmax_bwd(dout, out_fwd, out=None):
    return _elementwise(load().mrdis_softmax_bwd, 'softmax_bwd', (dout, out_fwd), out)


# ---------------------------------------------------------------- the latent-code options (csrc/mrdis_latent.hip)
KL_MAXM = 8


def _rows_view(t, what):
    """(t, row stride) of a (B, Z) fp32 device view whose rows are dense"""
    if t.dtype is not torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1): _refuse(what + ' (B, Z) rows', 'dtype dense', t)
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _blocks(ts, what):
    """M (B, Z) blocks of one shape sharing one row stride -> (views, ld)"""
    views = [_rows_view(t, what) for t in ts]
    if any(t.shape != ts[0].shape for t in ts): _refuse(what, 'like', *ts)
    lds = {ld for _, ld in views}
    if len(lds) != 1:
        ts = [t.contiguous() for t in ts]
        views = [(t, t.shape[1]) for t in ts]
    return [v for v, _ in views], views[0][1]


def _prior_view(pmu, plv, M, B, Z):
    """the prior as (pmu, plv, ldp_m, ldp_b): (M, Z) tensors (one row per contrast, broadcast over the batch) or (M, B, Z) (one row per sample)"""
    if pmu is None:
        return None, None, 0, 0
    if (plv is None or pmu.shape != plv.shape or not (pmu.dtype is plv.dtype is torch.float32)
            or tuple(pmu.shape) not in ((M, Z), (M, B, Z))): _refuse('kl', 'dtype', pmu, plv)
    if pmu.dim() == 2:
        if pmu.stride() != plv.stride() or pmu.stride(1) != 1:
            pmu, plv = pmu.contiguous(), plv.contiguous()
        return pmu, plv, pmu.stride(0), 0
    if pmu.stride() != plv.stride() or pmu.stride(2) != 1 or pmu.stride(0) == 0 or pmu.stride(1) == 0:
        pmu, plv = pmu.contiguous(), plv.contiguous()
    return pmu, plv, pmu.stride(0), pmu.stride(1)


def _kl_views(what, mu_list, lv_list, weight):
    """the operands kl_fwd / kl_bwd share: -> (mu views, ldmu, log-variance views, ldlv, the (M, B) weight table, B, Z)"""
    M = len(mu_list)
    if not 1 <= M <= KL_MAXM or len(lv_list) != M:
        raise MrdisError(f'{what}: 1 .. {KL_MAXM} contrasts (got {M} mu, {len(lv_list)} log-variance blocks)')
    mus, ldmu = _blocks(mu_list, f'{what} mu')
    lvs, ldlv = _blocks(lv_list, f'{what} log-variance')
    B, Z = mus[0].shape
    if lvs[0].shape != mus[0].shape or weight.dtype is not torch.float32 or tuple(weight.shape) != (M, B): _refuse(what, 'like vec dtype', lvs[0], weight)
    return mus, ldmu, lvs, ldlv, weight.contiguous(), B, Z


def kl_fwd(mu_list, lv_list, weight, pmu=None, plv=None):
    """-> 0-dim loss: sum_{i,b} weight[i, b] sum_z kl(mu_list[i][b], lv_list[i][b] | prior) (include/mrdis.h mrdis_kl_fwd).
    mu_list / lv_list: M (B, Z) fp32 views; weight: (M, B); pmu / plv: None (standard), (M, Z) or (M, B, Z) (two-Gaussian)."""
    M = len(mu_list)
    mus, ldmu, lvs, ldlv, w, B, Z = _kl_views('kl_fwd', mu_list, lv_list, weight)
    pmu, plv, ldp_m, ldp_b = _prior_view(pmu, plv, M, B, Z)
    loss = torch.empty((), dtype=torch.float32, device=mus[0].device)
    _chk(load().mrdis_kl_fwd(_ptr_array(mus), _ptr_array(lvs), ldmu, ldlv, _ptr(pmu), _ptr(plv), ldp_m, ldp_b, _ptr(w), _ptr(loss), M, B, Z,
                             _stream()), 'kl_fwd')
    return loss


def kl_bwd(dloss, mu_list, lv_list, weight, pmu=None, plv=None, need_prior=True):
    """-> (dmu (M, B, Z), dlv (M, B, Z), dpmu, dplv): the gradients of kl_fwd for the upstream gradient dloss (a 0-dim DEVICE tensor).
    dpmu / dplv have the prior's shape ((M, Z): summed over the batch), None without a prior or when need_prior is False."""
    M = len(mu_list)
    mus, ldmu, lvs, ldlv, w, B, Z = _kl_views('kl_bwd', mu_list, lv_list, weight)
    pmu, plv, ldp_m, ldp_b = _prior_view(pmu, plv, M, B, Z)
    dev = mus[0].device
    if dloss.numel() != 1 or not dloss.is_floating_point(): _refuse('kl_bwd', 'arg', dloss)
    dmu = torch.empty((M, B, Z), dtype=torch.float32, device=dev)
    dlv = torch.empty((M, B, Z), dtype=torch.float32, device=dev)
    dpmu = dplv = None
    if pmu is not None and need_prior:
        shape = (M, Z) if ldp_b == 0 else (M, B, Z)
        dpmu = torch.empty(shape, dtype=torch.float32, device=dev)
        dplv = torch.empty(shape, dtype=torch.float32, device=dev)
    g = dloss.reshape(()).float()
    _chk(load().mrdis_kl_bwd(_ptr(g), _ptr_array(mus), _ptr_array(lvs), ldmu, ldlv, _ptr(pmu), _ptr(plv), ldp_m, ldp_b, _ptr(w),
                             _ptr_array(list(dmu)), _ptr_array(list(dlv)), Z, Z, _ptr(dpmu), _ptr(dplv), M, B, Z, _stream()), 'kl_bwd')
    return dmu, dlv, dpmu, dplv


def avgpool_fwd(x, k):
    """F.avg_pool2d(x, k).view(N, -1) of an NHWC fp32 view: the dense (N, C * (H // k) * (W // k)) compact vector"""
    if x.dtype is not torch.float32 or k < 1: _refuse('avgpool_fwd', 'dtype arg', x)
    x, ldx = nhwc(x)
    N, C, H, W = x.shape
    y = torch.empty((N, C * (H // k) * (W // k)), dtype=torch.float32, device=x.device)
    _chk(load().mrdis_avgpool_fwd(_ptr(x), ldx, _ptr(y), N, H, W, C, k, _stream()), 'avgpool_fwd')
    return y


def avgpool_bwd(dy, in_shape, k, out=None):
    """dx (N, C, H, W) NHWC of avgpool_fwd for dy (N, D); out: an NHWC view to write into"""
    N, C, H, W = in_shape
    dy = dy.contiguous()
    if k < 1 or tuple(dy.shape) != (N, C * (H // k) * (W // k)) or dy.dtype is not torch.float32: _refuse('avgpool_bwd', 'dtype arg', dy)
    dx, lddx = _out_view(empty_nhwc(N, C, H, W, dy.device) if out is None else out, (N, C, H, W))
    _chk(load().mrdis_avgpool_bwd(_ptr(dy), _ptr(dx), lddx, N, H, W, C, k, _stream()), 'avgpool_bwd')
    return dx


# ---------------------------------------------------------------- the attention output decoders (csrc/mrdis_outdec.hip)
def _dense_f32(t, shape, what):
    if t.dtype is not torch.float32 or tuple(t.shape) != tuple(shape): _refuse(f'{what} {tuple(shape)}', 'vec dtype', t)
    return t.contiguous()


def chatt_fwd(x, s, wd, bd, wu, bu, out=None):
    """channel attention + skip sum: a = sigmoid(wu relu(wd mean_hw(x) + bd) + bu), out = (1 + a[b, c]) x + s (include/mrdis.h mrdis_chatt_fwd).
    x, s: (B, C, H, W) NHWC views; out: an NHWC view to write into (a channel slice of a wider buffer qualifies).
    -> (out, pool (B, C), hid (B, Hd), a (B, C)): the last three are what chatt_bwd reads."""
    (x, ldx), (s, lds) = _act_views('chatt_fwd', x, s)
    B, C, H, W = x.shape
    Hd = wd.shape[0]
    wd, bd = _dense_f32(wd, (Hd, C), 'chatt_fwd W_down'), _dense_f32(bd, (Hd,), 'chatt_fwd b_down')
    wu, bu = _dense_f32(wu, (C, Hd), 'chatt_fwd W_up'), _dense_f32(bu, (C,), 'chatt_fwd b_up')
    o, ldo = _out_view(empty_nhwc(B, C, H, W, x.device) if out is None else out, (B, C, H, W))
    dev = x.device
    pool = torch.empty((B, C), dtype=torch.float32, device=dev)
    hid = torch.empty((B, Hd), dtype=torch.float32, device=dev)
    a = torch.empty((B, C), dtype=torch.float32, device=dev)
    lib = load()
    nb = _ws_bytes(lib.mrdis_chatt_workspace, B, H * W, C, Hd)
    ws = _ws(nb, dev)
    _chk(lib.mrdis_chatt_fwd(_ptr(x), ldx, _ptr(s), lds, _ptr(wd), _ptr(bd), _ptr(wu), _ptr(bu), _ptr(o), ldo, _ptr(pool), _ptr(hid), _ptr(a),
                             _ptr(ws), nb, B, H * W, C, Hd, _stream()), 'chatt_fwd')
    return o, pool, hid, a


def chatt_bwd(dy, x, a, hid, pool, wd, wu):
    """-> (dx, dwd, dbd, dwu, dbu) of chatt_fwd for the upstream gradient dy (an NHWC view); the gradient of s is dy itself"""
    (dy, lddy), (x, ldx) = _act_views('chatt_bwd', dy, x)
    B, C, H, W = x.shape
    Hd = hid.shape[-1]
    wd, wu = _dense_f32(wd, (Hd, C), 'chatt_bwd W_down'), _dense_f32(wu, (C, Hd), 'chatt_bwd W_up')
    a, hid, pool = _dense_f32(a, (B, C), 'chatt_bwd a'), _dense_f32(hid, (B, Hd), 'chatt_bwd hid'), _dense_f32(pool, (B, C), 'chatt_bwd pool')
    dev = x.device
    dx = empty_nhwc(B, C, H, W, dev)
    dwd = torch.empty((Hd, C), dtype=torch.float32, device=dev)
    dbd = torch.empty((Hd,), dtype=torch.float32, device=dev)
    dwu = torch.empty((C, Hd), dtype=torch.float32, device=dev)
    dbu = torch.empty((C,), dtype=torch.float32, device=dev)
    lib = load()
    nb = _ws_bytes(lib.mrdis_chatt_workspace, B, H * W, C, Hd)
    ws = _ws(nb, dev)
    _chk(lib.mrdis_chatt_bwd(_ptr(dy), lddy, _ptr(x), ldx, _ptr(a), _ptr(hid), _ptr(pool), _ptr(wd), _ptr(wu), _ptr(dx), C, _ptr(dwd), _ptr(dbd),
                             _ptr(dwu), _ptr(dbu), _ptr(ws), nb, B, H * W, C, Hd, _stream()), 'chatt_bwd')
    return dx, dwd, dbd, dwu, dbu


def symdiff_fwd(g, out=None):
    """|g - g.flip(2)| of an NHWC view (include/mrdis.h mrdis_symdiff_fwd)"""
    return _elementwise(load().mrdis_symdiff_fwd, 'symdiff_fwd', (g,), out, nhw=True)


def symdiff_bwd(dgd, g, out=None):
    return _elementwise(load().mrdis_symdiff_bwd, 'symdiff_bwd', (dgd, g), out, nhw=True)


def rgate_fwd(x, alpha, out=None):
    """(1 + up2(alpha)) * x: x (B, C, H, W) NHWC view with even H, W; alpha (B, 1, H/2, W/2); up2 = bilinear x2, align_corners=False"""
    (x, ldx), = _act_views('rgate_fwd', x)
    B, C, H, W = x.shape
    al = _dense_f32(alpha, (B, 1, H // 2, W // 2), 'rgate_fwd alpha')
    o, ldo = _out_view(empty_nhwc(B, C, H, W, x.device) if out is None else out, (B, C, H, W))
    _chk(load().mrdis_rgate_fwd(_ptr(x), ldx, _ptr(al), _ptr(o), ldo, B, H, W, C, _stream()), 'rgate_fwd')
    return o


def rgate_bwd(dy, x, alpha):
    """-> (dx, dalpha (B, 1, H/2, W/2)) of rgate_fwd: dx element-wise, dalpha = the bilinear backward of sum_c dy * x"""
    (dy, lddy), (x, ldx) = _act_views('rgate_bwd', dy, x)
    B, C, H, W = x.shape
    al = _dense_f32(alpha, (B, 1, H // 2, W // 2), 'rgate_bwd alpha')
    dx = empty_nhwc(B, C, H, W, x.device)
    r = empty_nhwc(B, 1, H, W, x.device)
    _chk(load().mrdis_rgate_bwd(_ptr(dy), lddy, _ptr(x), ldx, _ptr(al), _ptr(dx), C, _ptr(r), B, H, W, C, _stream()), 'rgate_bwd')
    return dx, bilinear_bwd(r, (H // 2, W // 2), False)
