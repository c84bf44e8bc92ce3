// Shared helpers for libmrdis_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mrdis.h"
#include "mrdis_device.h"                                        // the device-side primitives every kernel shares
#include "mrdis_launchers.h"                                     // every launcher that crosses a file boundary, declared once

#define MRDIS_CHECK_LAUNCH()                                     \
    do {                                                         \
        hipError_t e_ = hipGetLastError();                       \
        if (e_ != hipSuccess) return MRDIS_ELAUNCH;              \
    } while (0)

// Process-wide switches.  Each is read from its environment variable ONCE (first use) and afterwards only changes through
// mrdis_set_option(): no getenv() on the launch path.  Boolean debug switches: variable present = 1.  Value switches: -1 = unset.
// ONE list: X(enum id, name, environment variable, is_flag, default) makes both MRDIS_OPT_* and the table of mrdis_runtime.hip, in this order.
#define MRDIS_OPTIONS(X) \
    X(WINO, "wino", "MRDIS_WINO", 0, 1) /* 0 direct kernels only | 1 measured policy | 2 Winograd wherever it applies */ \
    X(NT_MB, "nt_mb", "MRDIS_NT_MB", 0, 128) /* outputs of at least this many MB leave the Winograd kernel with non-temporal stores */ \
    X(WINO_PIPE, "wino_pipe", "MRDIS_WINO_PIPE", 0, 1) /* 1: the software-pipelined Winograd kernel (mrdis_wino2.hip) where it applies | 0: the phase-by-phase one */ \
    X(WINO_U, "wino_u", "MRDIS_WINO_U", 0, 1) /* 1: the pipelined kernel reads a pre-transformed filter image when the caller passes one | 0: always transforms the taps itself */ \
    X(WINO4, "wino4", "MRDIS_WINO4", 0, 1) /* 1: F(4x4, 3x3) (mrdis_wino4.hip) for the filters mrdis_wino_u_format() names, where the grid fills the chip | 0: never | 2: wherever the kernel applies */ \
    X(WINO4R, "wino4r", "MRDIS_WINO4R", 0, 1) /* <= 32 couts: 1: the register-fed F(4x4, 3x3) form (mrdis_wino4r.hip) for <= 64 reduction channels and inputs beyond the Infinity Cache | 0: the shared-transform form | 2 / 3: always its 64-tile / channel-split form */ \
    X(BCONV4, "bconv4", "MRDIS_BCONV4", 0, 1) /* bf16 3x3 stride-1 layers: 1: the LDS-DMA kernel (mrdis_bf16q.hip) where the launch fills the chip | 0: bconv3_kernel (mrdis_bf16p.hip) | 2: wherever it applies */ \
    X(SPLIT6, "split6", "MRDIS_SPLIT6", 0, 1) /* thin fp32 3x3 stride-1 layers on the bf16 matrix pipe: both fp32 operands as three bf16 terms, the six products of order <= 2 summed in fp32 (2^-23 relative per product).  1: the 4 -> C kernel for <= 32 couts, the C -> 4 kernel, sp6.out forward + weight gradient (32 -> 16) | 0: fp32 MFMA | 2 .. 7: one 2-D kernel at a time, see run_c4conv | 8 / 9: only the 3-D 16 -> 16 forward + data gradient / weight gradient kernel (mrdis_conv3d_s6.hip; both also under 1) | 10: only the tap-table kernel for launches that bring a filter image (mrdis_s6conv.hip; also under 1) */ \
    X(NO16, "debug_no16", "MRDIS_DEBUG_NO16", 1, 0) \
    X(NOTHIN, "debug_nothin", "MRDIS_DEBUG_NOTHIN", 1, 0) \
    X(NOC4, "debug_noc4", "MRDIS_DEBUG_NOC4", 1, 0) \
    X(NODMA, "debug_nodma", "MRDIS_DEBUG_NODMA", 1, 0) \
    X(NO16_3D, "debug_no16_3d", "MRDIS_DEBUG_NO16_3D", 1, 0) \
    X(BILGEN, "debug_bilgen", "MRDIS_DEBUG_BILGEN", 1, 0) \
    X(NOW16, "debug_now16", "MRDIS_DEBUG_NOW16", 1, 0) \
    X(NOPACK, "debug_nopack", "MRDIS_DEBUG_NOPACK", 1, 0) /* 1: the four parity classes of a stride-2 data gradient as four launches */ \
    X(MODE, "debug_mode", "MRDIS_DEBUG_MODE", 0, -1) \
    X(BN, "debug_bn", "MRDIS_DEBUG_BN", 0, -1) \
    X(KC, "debug_kc", "MRDIS_DEBUG_KC", 0, -1) \
    X(BM, "debug_bm", "MRDIS_DEBUG_BM", 0, -1) \
    X(C4_TW, "debug_c4_tw", "MRDIS_DEBUG_C4_TW", 0, -1) \
    X(WGSPLIT, "debug_wgsplit", "MRDIS_DEBUG_WGSPLIT", 0, -1) \
    X(BN3, "debug_bn3", "MRDIS_DEBUG_BN3", 0, -1) \
    X(KC3, "debug_kc3", "MRDIS_DEBUG_KC3", 0, -1) \
    X(C4_GRID, "c4_grid", "MRDIS_C4_GRID", 0, 0) /* persistent grid of the Cin = 4 kernels (run_c4conv): 0 = workgroups per CU from the occupancy query of the launched instantiation | k > 0: k workgroups per CU */ \
    X(C4_BLOCKS, "debug_c4_blocks", "MRDIS_DEBUG_C4_BLOCKS", 0, -1) /* read-only diagnostic: grid.x of the last run_c4conv launch */ \
    X(ZS_GRID, "zsearch_grid", "MRDIS_ZSEARCH_GRID", 0, 0) /* workgroups of mrdis_cosine_top1 (mrdis_zsearch.hip): 0 = min(tiles, 1024) | k > 0: min(k, tiles, 2048) */ \
    X(VOLGEN, "debug_volgen", "MRDIS_DEBUG_VOLGEN", 1, 0) /* 1: mrdis_volume_gather and mrdis_patch_gather always run their element kernel (mrdis_volgather.hip, mrdis_patch.hip), never the LDS-tile form */
#define MRDIS_X_OPT_ID(id, name, env, is_flag, dflt) MRDIS_OPT_##id,
enum { MRDIS_OPTIONS(MRDIS_X_OPT_ID) MRDIS_OPT_COUNT };
long long mrdis_opt(int id);      // mrdis_runtime.hip
void mrdis_opt_note(int id, long long value);      // diagnostics a launcher leaves behind (read with mrdis_get_option)

// Launch counters of the Winograd / bf16 / six-product (split6) kernel families (host side, one increment per launch): what a test asks to know which form actually ran
// (mrdis_launch_count("wino4") ...; mrdis_runtime.hip).  ONE list as above: X(enum id, name).
#define MRDIS_COUNTERS(X) \
    X(WINO, "wino") X(WINO_SPADE, "wino_spade") X(WINO2, "wino2") X(WINO2_SPADE, "wino2_spade") X(WINO4, "wino4") X(WINO4_SPADE, "wino4_spade") X(WINO4N, "wino4n") \
    X(WINO4R, "wino4r") X(WINO_WGRAD, "wino_wgrad") X(WINO_WGRAD2, "wino_wgrad2") X(WINO4_WGRAD, "wino4_wgrad") X(BCONV3, "bconv3") X(BCONV3_SPADE, "bconv3_spade") \
    X(BCONV4, "bconv4") X(BCONV4_SPADE, "bconv4_spade") X(BWGRAD, "bwgrad") X(BWGRAD2, "bwgrad2") X(BWGRAD3, "bwgrad3") X(BWGRAD_S2, "bwgrad_s2") /* mrdis_bf16.hip: bwgrad_kernel, bwgrad2_kernel, bwgrad3_kernel, bwgrad_pack_kernel; their reduce launch is not counted */ \
    X(SPLIT6_C4, "split6_c4") X(SPLIT6_C16, "split6_c16") X(SPLIT6_WGRAD16, "split6_wgrad16") X(SPLIT6_CO4, "split6_co4") \
    X(SPLIT6_C3D, "split6_c3d") X(SPLIT6_W3D, "split6_w3d") X(SPLIT6_TAP, "split6_tap") X(ZSEARCH, "zsearch") \
    X(CONV2SRC, "conv2src") X(ANA_ACT, "ana_act") /* mrdis_encs.hip: the others-variant kernels */ \
    X(KL, "kl") X(AVGPOOL, "avgpool") /* mrdis_latent.hip: the KL term and mean compaction */ \
    X(CHATT, "chatt") X(SYMDIFF, "symdiff") X(RGATE, "rgate") /* mrdis_outdec.hip: the attention output decoders */ \
    X(DIRECT3D, "direct3d") X(C3D16, "c3d16") X(WGRAD3D, "wgrad3d") X(WGRAD3D16, "wgrad3d16") X(WINO_WGRAD3D, "wino_wgrad3d") /* mrdis_conv3d.hip / mrdis_wino.hip: the 3-D kernels */ \
    X(VOLGATHER, "volgather") /* mrdis_volgather.hip: the 3-D batch gather, one count per mrdis_volume_gather call */ \
    X(FGCOUNT, "fgcount") X(PATCHORIGIN, "patchorigin") X(PATCHGATHER, "patchgather") /* mrdis_patch.hip: one count per mrdis_fg_block_counts / mrdis_patch_origins / mrdis_patch_gather call */ \
    X(PATCHWARP, "patchwarp") /* mrdis_warp.hip: one count (and one launch) per mrdis_patch_warp call */ \
    X(PATCHBLUR, "patchblur") X(PATCHSTATS, "patchstats") X(PATCHTONE, "patchtone") /* mrdis_tone.hip: one count per mrdis_patch_blur / mrdis_patch_stats / mrdis_patch_tone call */ \
    X(LOSS3D, "loss3d") X(SEGCOUNTS, "segcounts") /* mrdis_loss3d.hip: one count per mrdis_nvnet_loss_fwd / _bwd call; one per mrdis_seg_counts call */ \
    X(SEGACCUM, "segaccum") X(SEGLABELS, "seglabels") /* mrdis_segvol.hip: one count per mrdis_seg_accum / mrdis_seg_label_volume call */ \
    X(TILEACCUM, "tileaccum") X(TILELABELS, "tilelabels") /* mrdis_segvol.hip, tile-wise prediction: one count per mrdis_tile_accum / mrdis_tile_label_volume call */ \
    X(SYNTHACCUM, "synthaccum") X(SYNTHFINISH, "synthfinish") /* mrdis_synth.hip: one count per mrdis_synth_accum / mrdis_synth_finish call */ \
    X(SEG2DLABELS, "seg2dlabels") X(SEG2DFINISH, "seg2dfinish") /* mrdis_seg2d.hip: one count per mrdis_seg2d_label_planes / mrdis_seg2d_finish call */ \
    X(FUSE, "fuse") /* mrdis_fuse.hip: one count per mrdis_fuse_present_fwd / _bwd call */ \
    X(REGSURF, "regsurf") X(EDT, "edt") X(SURFHIST, "surfhist") /* mrdis_surfdist.hip: one count per mrdis_region_surfaces call; one per launch of a distance-transform pass; one per histogram pass (one per mrdis_surface_hist call) */ \
    X(CCLABEL, "cclabel") X(CCCLEAN, "ccclean") /* mrdis_cc.hip: one count per launch of a labelling pass (three per mrdis_cc_label call); one per mrdis_cc_clean call */ \
    X(PREPSTATS, "prepstats") X(PREPWRITE, "prepwrite") /* mrdis_prep.hip: one count per mrdis_prep_stats / mrdis_prep_write call */ \
    X(EXPORT, "export") /* mrdis_export.hip: one count (and one launch) per mrdis_export_volume call */ \
    X(DILATE, "dilate") X(LESMATCH, "lesmatch") X(LESEXPAND, "lesexpand") /* mrdis_lesion.hip: one count per launch of mrdis_region_planes / mrdis_dilate (one per iteration); one per mrdis_lesion_match call; one per mrdis_lesion_expand call */ \
    X(STAT_VEC, "stat_vec") X(STAT_SCALAR, "stat_scalar") X(STAT_INTERP, "stat_interp") /* mrdis_elem.hip launch_stats: which partial-sum kernel took the pass */ \
    X(SPADE_UP2_ONEPASS, "spade_up2_onepass") X(SPADE_UP2_TWOPASS, "spade_up2_twopass") /* mrdis_instnorm_spade_bwd_up2: one count per call, by route */ \
    X(BIL_FWD_X2, "bil_fwd_x2") X(BIL_FWD_GENERAL, "bil_fwd_general") /* mrdis_bilinear_fwd */ \
    X(BIL_BWD_X2, "bil_bwd_x2") X(BIL_BWD_TIGHT3, "bil_bwd_tight3") X(BIL_BWD_TIGHT5, "bil_bwd_tight5") X(BIL_BWD_GENERAL, "bil_bwd_general") /* mrdis_bilinear_bwd */ \
    X(ELEM_V1, "elem_v1") /* mrdis_elem.hip: an element-wise pass took its one-channel-per-thread (V = 1) instantiation (views not 16-byte aligned or C % 4 != 0); also, once per call, the chatt / symdiff / rgate entry points of mrdis_outdec.hip when chatt_vec chose their scalar forms (a stride % 4 != 0 counts too) */ \
    X(ALL, "all") /* every launch of the library */
#define MRDIS_X_CNT_ID(id, name) MRDIS_CNT_##id,
enum { MRDIS_COUNTERS(MRDIS_X_CNT_ID) MRDIS_CNT_COUNT };
void mrdis_count(int id);

// Every kernel launch of the library goes through MRDIS_LAUNCH: it records, per kernel expression, the largest DYNAMIC LDS size it was launched with
// (rocprofv3's kernel trace reports only the static group segment: 0 for the `extern __shared__` kernels, e.g. the 155 KB of wino4_kernel).
// mrdis_dynamic_lds_table (mrdis_runtime.hip) hands the table out; bench.py puts it into its JSON line, tools/prof_summary.py into the per-kernel tables.
void mrdis_note_lds(const char* kernel_expr, size_t bytes);
#define MRDIS_LAUNCH(kernel, grid, block, lds, s, ...) do { mrdis_count(MRDIS_CNT_ALL); if ((size_t)(lds) != 0) mrdis_note_lds(#kernel, (size_t)(lds)); hipLaunchKernelGGL(kernel, grid, block, lds, s, __VA_ARGS__); } while (0)

// Host setup before a launch (mrdis_runtime.hip), cached per kernel ADDRESS (every template instantiation is its own entry) and safe from any
// thread; the hit path is pointer compares, no lock, no runtime call.  A failed opt-in or query is not cached: the next call asks again.
int mrdis_cu_count();                                            // CUs of the device (256 if the runtime cannot say); queried once
bool mrdis_lds_optin(const void* kernel, int bytes);             // the kernel may launch with up to `bytes` of dynamic LDS; false: the runtime refused
int mrdis_occupancy(const void* kernel, int block, size_t lds);  // workgroups per CU at (block, lds), 0 if the runtime gives no answer;
                                                                 // lds above 64 KB needs the kernel's opt-in first

static inline int mrdis_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Bijective XCD-aware remap (cdna_hip_programming.md T1): workgroups b and b+8 share an XCD, so
// give each XCD a contiguous run of logical tile ids -> neighbouring tiles hit the same L2.
__device__ __forceinline__ int mrdis_xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

__device__ __forceinline__ float mrdis_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double mrdis_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
