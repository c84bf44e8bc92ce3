/* mrdis.h -- C ABI of libmrdis_hip.so: the MI355X (gfx950) hot path of the
 * multi-modal MR representation-disentanglement training step.
 *
 * The reference (ouyangjiahong/representation-disentanglement) is pure
 * Python/PyTorch and has no FFI; its operator seam is the class factory
 * `Conv2d(is_cond)` / `CondConv2d.forward` (src/model.py:2075-2120) and the
 * ATen ops its blocks dispatch.  Each entry point below
 * names the reference call site it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller; nothing is
 *    allocated or freed inside the library, nothing synchronises the host.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it.
 *  - activations are NHWC fp32 "views": element (n,h,w,c) of a tensor lives at
 *    p[((n*H + h)*W + w)*ld + c]; `ld` (>= C, in floats) lets a view address a
 *    channel slice of a wider buffer (concat elision).
 *  - return value: 0 = ok, negative = MRDIS_E* (see mrdis_strerror).  No
 *    entry point throws or aborts.
 *  - thread-safety: re-entrant for distinct streams / distinct buffers.
 */
#ifndef MRDIS_H
#define MRDIS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRDIS_OK            0
#define MRDIS_EINVAL       -1   /* bad shape / argument                       */
#define MRDIS_EUNSUPPORTED -2   /* geometry outside what the kernels cover    */
#define MRDIS_EWORKSPACE   -3   /* workspace too small                        */
#define MRDIS_ELAUNCH      -4   /* hipLaunch reported an error                */
#define MRDIS_EALIGN       -5   /* pointer / ld alignment requirement broken  */

#define MRDIS_MAX_TAPS 16

/* epilogue flags of mrdis_conv2d_fwd */
#define MRDIS_EPI_NONE   0
#define MRDIS_EPI_LRELU  1      /* y = leaky_relu(conv + bias, 0.2): model.py:2227, 2375-2394, 2774 */

const char* mrdis_strerror(int code);
int mrdis_version(void);

/* Process-wide switches.  Each one is initialised from its environment variable when the library is first used and is
 * changed afterwards only through mrdis_set_option (nothing on the launch path calls getenv):
 *   "wino"  (MRDIS_WINO, default 1): 0 = direct convolution kernels only, 1 = fused Winograd F(2x2,3x3) where it measured
 *           faster (csrc/mrdis_conv.hip wino_wanted), 2 = Winograd wherever the kernel applies (tests);
 *   "nt_mb" (MRDIS_NT_MB, default 128): Winograd outputs of at least this many MB are written with non-temporal stores;
 *   "wino_pipe" (MRDIS_WINO_PIPE, default 1): 1 = the software-pipelined Winograd kernels (csrc/mrdis_wino2.hip: forward / data
 *           gradient for Cout > 32, weight gradient for Ci, Co multiples of 64), 0 = the phase-by-phase kernels everywhere
 *           (same arithmetic; results agree to 1e-5);
 *   "wino_u" (MRDIS_WINO_U, default 1): 1 = the pipelined kernels read the pre-transformed filter image a caller passes (w_wino), 0 = they
 *           always transform the taps themselves (F(2x2): bit-identical either way; also keeps the F(4x4) kernel, which has no in-kernel
 *           filter transform, out);
 *   "wino4" (MRDIS_WINO4, default 1): 1 = Winograd F(4x4,3x3) (csrc/mrdis_wino4.hip, mrdis_wino4r.hip: 1.78x fewer multiplies than F(2x2),
 *           results within ~5e-6 of the maximum of the direct kernel's) for the 3x3 stride-1 filters whose image mrdis_wino_u_format() gives
 *           format 4 or 5, where the caller passes that image and the launch fills >= 3/4 of the chip (>= 192 workgroups, maps >= 16 x 32):
 *             format 4 (36-point image + the 16-point one): reduction channels R % 8 == 0, couts S >= 64, S % 4 == 0, and R >= 64 for a plain
 *                       filter, R >= 32 for the fused gamma | beta filter of mrdis_conv2d_fwd_spade (C % 8 == 0, C >= 32);
 *             format 5 (36-point image of the 32-cout forms, wino4r / wino4n kernels): R % 8 == 0, R >= 16, S == 32;
 *             format 2 (16-point F(2x2) image) otherwise;
 *           the same option gates the F(3x3,4x4) weight gradient (csrc/mrdis_wino4w.hip) inside mrdis_conv2d_bwd_weight (Ci % 32 == 0, Co % 64 == 0, H and W
 *           multiples of 8, >= 192 workgroups of >= 24 iterations each); 0 = never (F(2x2) everywhere, every image format 2); 2 = wherever those kernels apply (tests: R >= 16,
 *           format 5 from 4 couts).  The option picks the format when an image is BUILT; a built image keeps its format, which the caller
 *           passes beside the pointer (w_wino_fmt) -- changing the option later never makes a kernel read an image in another layout;
 *   "debug_now16" (MRDIS_DEBUG_NOW16, default 0): 1 = the dedicated narrow-layer kernels off -- Cout <= 16 weight gradient
 *           (mrdis_wgrad16.hip), stride-2 first layers and 4 -> C weight gradient (mrdis_wgrad_s2.hip), 1x1 head (mrdis_pointwise.hip),
 *           16-cout and 4-cout 3x3 layers (mrdis_c16.hip, mrdis_co4.hip): the generic tile kernels run those layers (tests and
 *           tools/ use it for A/B; results agree to fp32 rounding);
 *   "debug_nopack" (MRDIS_DEBUG_NOPACK, default 0): 1 = the four output-parity classes of a stride-2 data gradient as four launches
 *           instead of one (bit-identical results; A/B switch);
 *   other "debug_*": kernel-selection overrides used by tools/ (see csrc/mrdis_common.h MRDIS_OPTIONS);
 *   "zsearch_grid" (MRDIS_ZSEARCH_GRID, default 0): workgroups of mrdis_cosine_top1: 0 = min(gallery tiles, 1024), k > 0 = min(k, tiles, 2048) (results do not depend on it).
 * set: 0 or MRDIS_EINVAL (unknown name); get: the value, or MRDIS_EINVAL for an unknown name.  Safe from any thread: a change
 * applies to launches that start after the call returns (a launch already in progress on another thread may still see the old value). */
int mrdis_set_option(const char* name, long long value);
long long mrdis_get_option(const char* name);
/* Launches since load / the last reset of one kernel family (counted on the host at launch): "wino" | "wino_spade" (phase-by-phase F(2x2)),
 * "wino2" | "wino2_spade" (pipelined F(2x2)), "wino4" | "wino4_spade" (F(4x4) 64-cout forms), "wino4n" | "wino4r" (32-cout forms: shared transform / register-fed),
 * "wino_wgrad" | "wino_wgrad2" (F(2x2) weight gradient), "wino4_wgrad" (F(3x3,4x4)); "bconv3" | "bconv3_spade" | "bconv4" | "bconv4_spade" (bf16 3x3 forms);
 * "bwgrad" | "bwgrad2" | "bwgrad3" | "bwgrad_s2" (the bf16 weight gradients: bwgrad_kernel, its register-staged and LDS-DMA pipelined forms, the stride-2 parity-class launch; the reduce launch is not counted);
 * "split6_c4" | "split6_c16" | "split6_wgrad16" | "split6_co4" | "split6_c3d" | "split6_w3d" | "split6_tap" (option split6: the 4 -> C kernel, the 32 -> 16 forward, its weight gradient, the
 * C -> 4 kernel, the 3-D 16 -> 16 forward / data-gradient and weight-gradient kernels, the tap-table kernel fed by mrdis_s6_filter_image, as six bf16 products per fp32 product); "zsearch" (mrdis_cosine_top1); "conv2src" | "ana_act" (the others variants); "kl" | "avgpool" (the latent-code options); "chatt" | "symdiff" | "rgate" (the attention output decoders);
 * "direct3d" | "c3d16" | "wgrad3d" | "wgrad3d16" | "wino_wgrad3d" (the 3-D tap-table, 16-cout, generic and narrow weight-gradient kernels and the hybrid
 * Winograd weight gradient, one count per depth-tap launch; the hybrid 3-D forward / data gradient counts as "wino_spade"); "volgather"; "loss3d" | "segcounts" (the fused 3-D objective, one count per forward and per backward call, and the segmentation counts); "segaccum" | "seglabels" (whole-volume prediction of the 3-D nets); "synthaccum" | "synthfinish" (whole-subject synthesis of the 2-D model, one count per call); "seg2dlabels" | "seg2dfinish" (whole-subject segmentation by the 2-D model, one count per call); "fuse" (mrdis_fuse_present_fwd / _bwd, one count per call); "export" (mrdis_export_volume, one count and one launch per call);
 * "stat_vec" | "stat_scalar" | "stat_interp" (the partial-sum kernel of a statistics pass), "spade_up2_onepass" | "spade_up2_twopass" (the route of
 * mrdis_instnorm_spade_bwd_up2, one per call), "bil_fwd_x2" | "bil_fwd_general", "bil_bwd_x2" | "bil_bwd_tight3" | "bil_bwd_tight5" | "bil_bwd_general"
 * (mrdis_bilinear_fwd / _bwd, one per call), "elem_v1" (an element-wise pass in its one-channel-per-thread form; also, once per call, mrdis_chatt_* / mrdis_symdiff_* /
 * mrdis_rgate_* in their scalar forms: C % 4 != 0, a view not 16-byte aligned or a pixel stride % 4 != 0): dispatch choices, not launches;
 * "all" (every kernel launch of the library).  MRDIS_EINVAL for an unknown name.  Diagnostics: the parity tests
 * use it to prove that the form under test is the one that ran. */
long long mrdis_launch_count(const char* family);
void mrdis_launch_count_reset(void);
/* The largest DYNAMIC LDS size each kernel was launched with so far, as "kernel expression=bytes" lines (at most cap - 1 characters, whole lines only); returns the number of
 * lines written.  rocprofv3's kernel trace only shows the static group segment (0 for the kernels that size their LDS at launch). */
int mrdis_dynamic_lds_table(char* buf, int cap);

/* ---- expert mixing: model.py:2111-2113 --------------------------------------
 * W   : (E, Co, Ci, kh, kw) checkpoint layout (OIHW with leading expert dim)
 * r   : (E) routing weights sigmoid(fc(type)) -- one row; the reference's
 *       inputs_type is constant over the batch at every call site
 *       (model.py:3138, 3169, 3190, 3211), so one mixed kernel serves a call.
 * w_tck : out, [T][Ci][Co]   (T = kh*kw)  forward / wgrad layout
 * w_tkc : out, [T][Co][Ci]                data-gradient layout
 * E = 1 with r = {1} turns a plain nn.Conv2d weight into the two layouts.    */
int mrdis_mix_experts_fwd(const float* W, const float* r, float* w_tck, float* w_tkc,
                          int E, int Co, int Ci, int T, void* stream);

/* backward of the above.  dw_tck: [T][Ci][Co] gradient of the mixed kernel.
 * dW (E,Co,Ci,T) = r[e] * dWm ;  dr[e] += <dWm, W[e]>  (two-level ordered
 * reduction through `workspace`, bit-reproducible; caller zeroes dr).        */
size_t mrdis_mix_experts_bwd_workspace(int E, int Co, int Ci, int T);
int mrdis_mix_experts_bwd(const float* dw_tck, const float* W, const float* r,
                          float* dW, float* dr, void* workspace, size_t workspace_bytes,
                          int E, int Co, int Ci, int T, void* stream);

/* Routed forms: the routing r = sigmoid(fc_w @ type_row + fc_b) of `_routing.forward` (model.py:2071-2073) is
 * evaluated inside the mix kernel (r_out (E) is kept for the backward), and the backward returns the
 * gradients of the routing Linear directly: dfc_w (E,emb), dfc_b (E).  type_row: (emb) device floats. */
int mrdis_mix_experts_routed_fwd(const float* W, const float* fc_w, const float* fc_b, const float* type_row, int emb,
                                 float* r_out, float* w_tck, float* w_tkc, int E, int Co, int Ci, int T, void* stream);
int mrdis_mix_experts_routed_bwd(const float* dw_tck, const float* W, const float* r, const float* type_row, int emb,
                                 float* dW, float* dfc_w, float* dfc_b, void* workspace, size_t workspace_bytes,
                                 int E, int Co, int Ci, int T, void* stream);

/* All M type rows of a layer at once (types (M, emb); a step calls every CondConv2d with each modality
 * label, model.py:3138).  w_tck / w_tkc / dw_tck are HOST arrays of M device pointers; a NULL dw_tck[m]
 * means "type m received no gradient".  r_out (M, E).  dW, dfc_w, dfc_b are the sums over the types.     */
int mrdis_mix_experts_routed_multi_fwd(const float* W, const float* fc_w, const float* fc_b, const float* types, int emb, int M,
                                       float* r_out, float* const* w_tck, float* const* w_tkc,
                                       void* const* w_bf16_tck, void* const* w_bf16_tkc,   /* both NULL, or M bf16 buffers each: bf16 copies of
                                                                                              the two layouts (what mrdis_cast_bf16 would give) */
                                       int ld_tck, long long tap_tkc,   /* 0 = dense.  Otherwise the row pitch of the [T][Ci][.] outputs and the tap
                                                                           pitch of the [T][.][Ci] outputs: the pointers address a column / row block of a
                                                                           wider filter (the halves of a fused gamma | beta filter, model.py:2443-2444) */
                                       int E, int Co, int Ci, int T, void* stream);
size_t mrdis_mix_experts_routed_multi_bwd_workspace(int M, int E, int Co, int Ci, int T);
int mrdis_mix_experts_routed_multi_bwd(const float* const* dw_tck, const float* W, const float* r, const float* types,
                                       int emb, int M, float* dW, float* dfc_w, float* dfc_b,
                                       int accumulate,      /* 1: the three results are ADDED to dW / dfc_w / dfc_b (gradient sinks) */
                                       int ld_dw,           /* 0 = dense; otherwise the row pitch of the dw_tck tensors (a column block of a wider gradient) */
                                       void* workspace, size_t workspace_bytes, int E, int Co, int Ci, int T, void* stream);


/* Every CondConv2d layer of the model in one launch (forward) and one launch pair (backward): the per-layer launches above over a
 * table of jobs in device memory.  A job = one layer, or one half of a fused gamma | beta filter pair; its fields (pointers to the
 * expert weights, routing parameters, the per-label outputs, the gradient sinks, its block range) are laid out as `MixJob` in
 * csrc/mrdis_conv.hip (mrdis_mix_job_bytes() = its size, 368; the Python binding mirrors it with ctypes).  Block-to-element mapping and
 * summation order are those of the per-layer launches (mrdis_mix_job_blocks blocks per job): bit-identical results.
 * dw_table: [njobs][8] device pointers to this step's filter gradients [T][Ci][ld_dw], null where a label's filter got none.
 * Replaces ~90 x routing.forward + sum(r * W) (model.py:2071-2073, 2113) per step and their backward. */
size_t mrdis_mix_job_bytes(void);
int mrdis_mix_job_blocks(int Co, int Ci, int T);
int mrdis_mix_jobs_fwd(const void* jobs, int njobs, int total_blocks, const float* types, int emb, int M, void* stream);
int mrdis_mix_jobs_bwd(const void* jobs, int njobs, int total_blocks, const void* dw_table, const float* types, int emb, int M, void* stream);

/* ---- convolution: F.conv2d at model.py:2104 (CondConv2d._conv_forward) and
 * nn.Conv2d of the discriminator model.py:2773-2789 ---------------------------
 * x : NHWC view (N,H,W,Ci) ld=ldx ; y : NHWC view (N,Ho,Wo,Co) ld=ldy
 * w_tck from mrdis_mix_experts_fwd ; bias (Co) or NULL.
 * kernel (kh,kw) in {1x1,3x3,4x4}; stride in {1,2}; zero padding `pad`.
 *
 * dtype (BASELINE.json configs[2], SURVEY.md 8b "dtype"):
 *   MRDIS_DT_F32       fp32 activations, fp32 MFMA (v_mfma_f32_32x32x2_f32 / Winograd) -- the parity path;
 *   MRDIS_DT_F32_BF16M fp32 activations in HBM, bf16 MFMA operands (v_mfma_f32_32x32x16_bf16, inputs rounded RNE on the
 *                      way into LDS), fp32 accumulate / bias / epilogue.  Needs the bf16 copy of the filter with the
 *                      REDUCTION axis contiguous (mrdis_cast_bf16 of the other layout): forward w_bf16_tkc = bf16
 *                      [T][Co][Ci], data gradient w_bf16_tck = bf16 [T][Ci][Co].  Geometries the bf16 kernel does not
 *                      cover (reduction axis not a multiple of 16, fewer than 16 output channels) and a NULL bf16 filter
 *                      run the fp32 kernels: the result is then exact fp32;
 *   MRDIS_DT_BF16      bf16 activations in HBM (x, y, dy, dx are bf16 views, ld in bf16 elements), bf16 MFMA operands, fp32
 *                      accumulate; bias, filters' master copy, weight / bias gradients and all statistics stay fp32.
 *                      Convolutions: the geometries of the bf16 kernels only (reduction axis % 16 == 0, at least 16 output
 *                      channels, % 4) -- others return MRDIS_EUNSUPPORTED and the caller casts the view (mrdis_cast_view)
 *                      around the fp32 kernel.  The norm / resize / activation entry points take either storage type
 *                      through their own `dtype` argument (arithmetic is fp32 inside).                               */
#define MRDIS_DT_F32        0
#define MRDIS_DT_F32_BF16M  1
#define MRDIS_DT_BF16       2
/* mixed storage at the two ends of a bf16 stretch (`compute_dtype: bf16` keeps tensors with < 16 channels in fp32): named after the
 * LAYER's input x (= dx) and output y (= dy), the same code goes to its forward, data-gradient and weight-gradient entry points.
 *   MRDIS_DT_XBF16_YF32  x / dx bf16 views, y / dy fp32: the 1x1 decoder head 16 -> <= 8 (forward, data gradient, weight gradient); the 3x3
 *                        C -> 4 layer (ana_dec.output): forward (x bf16, C = 32 / 64, y (N, H, W, 4) fp32; w_tck is then [9][C][16], columns >= 4
 *                        zero), data gradient (dy fp32 -> dx bf16; w_tkc is then [9][16][Ci], rows >= 4 zero) and weight gradient (x bf16 with
 *                        C = 32 / 64, dy (N, H, W, 4) fp32 -> dw_tck (9, C, 4) + the 4 bias sums; maps 64 / 128 / 256 wide, else MRDIS_EUNSUPPORTED)
 *   MRDIS_DT_XF32_YBF16  x / dx fp32, y / dy bf16: the 3x3 4 -> C si_layers -- forward (w_tck is then the [9][16][Co] layout, rows >= 4 zero),
 *                        weight gradient (dw_tck (9, 4, Co); maps 64 / 128 / 256 wide, Co 32 / 64 / 128, else MRDIS_EUNSUPPORTED) and data
 *                        gradient (dy bf16, Co = 32 / 64 -> dx (N, H, W, 4) fp32; w_tkc is then [9][Co][16], columns >= 4 zero)
 *                        (the 16-row / 16-column filter layouts are those the mixing launch writes for narrow layers under bf16 storage)
 * These kernels multiply on the bf16 matrix pipe with the fp32 side carried as two (bf16-output forms) or three (fp32-output forms: exact
 * products) bf16 terms; MRDIS_EUNSUPPORTED outside the shapes named.
 * Under MRDIS_DT_BF16 mrdis_conv2d_bwd_weight also takes the stride-2 layers (3x3 / 4x4, pad 1, even H and W, Ci 16 or a multiple of 32, Co % 8 == 0):
 * four input-parity classes in one launch.                                                                                          */
#define MRDIS_DT_XBF16_YF32 3
#define MRDIS_DT_XF32_YBF16 4
/* mrdis_conv2d_bwd_weight only, OR-ed onto one of the two mixed-storage types: dw_tck has the STORED shape of a filter that the mixing launch keeps
 * zero-padded to 16 -- [T][16][Co] for a 4 -> C layer (MRDIS_DT_XF32_YBF16), [T][Ci][16] for a C -> 4 layer (MRDIS_DT_XBF16_YF32) -- and the rows /
 * columns beyond the layer's own are written as zeros (no pad of the result afterwards).  MRDIS_EUNSUPPORTED where the four-channel kernels decline. */
#define MRDIS_DT_DW_PAD16   0x100
/* w_wino (fp32 paths, may be NULL): the filter already in the Winograd domain, the image mrdis_wino_u_jobs builds from w_tck (role:
 * forward) -- used where a software-pipelined Winograd kernel takes the layer, ignored elsewhere.  w_wino_fmt: the format that image was
 * BUILT in (the job's fmt: 2 | 4 | 5; ignored when w_wino is NULL); MRDIS_EINVAL if no image of this filter shape can have it.  Format 2
 * (F(2x2,3x3)): same results bit for bit with or without the image; formats 4 / 5: select the F(4x4,3x3) kernels, which exist only on the
 * image (with the option "wino4" at 0 a format-4 image is read through its trailing 16-point part, a format-5 image is ignored). */
int mrdis_conv2d_fwd(const void* x, int ldx, const float* w_tck, const void* w_bf16_tkc, const float* bias,
                     void* y, int ldy, int N, int H, int W, int Ci, int Co,
                     int kh, int kw, int stride, int pad, int epilogue, int dtype, const float* w_wino, int w_wino_fmt, void* stream);

/* ---- filter images for the software-pipelined Winograd kernels (csrc/mrdis_wino2.hip).  U = G g G^T of a 3x3 filter does not depend
 * on the activations; a training step uses each mixed filter 8-16 times, so the transform is taken out of the convolution kernels:
 * one launch over a job table builds, per (filter, role), the 16-point image in the order the kernel's (input-channel chunk, 64-cout
 * tile) walk consumes it: [cout tile][chunk of 8][8][4][64][4] floats, zero-padded (format 2); format 4 is the 36-point image of the
 * F(4x4,3x3) kernel, [cout tile][chunk of 4][18 point pairs][4][128] floats (csrc/mrdis_wino4.h), FOLLOWED by the format-2 image of the same filter
 * (what a call runs on whose grid the F(4x4) kernel declines: small maps); format 5 is the 36-point image of the 32-cout F(4x4) forms alone.
 * mrdis_wino_u_format(R, S, spadeC) says which one a filter gets NOW (a function of the filter's shape and the current value of the option
 * "wino4"); the job records it, mrdis_wino_u_image_floats_fmt sizes an image of a given format (-1: that shape never has it), and the
 * convolution entry points take it beside the image pointer (w_wino_fmt).
 * Job (`WinoUJob`, mrdis_wino_u_job_bytes() = 48):
 *   { const float* w; float* img; int R, S, flip, spadeC, block0, nblk, fmt, pad; }        fmt = mrdis_wino_u_format(R, S, spadeC) when built
 * w = [9][R][S]: role forward: w_tck, R = Ci, S = Co, flip = 0; role data gradient: w_tkc, R = Co, S = Ci, flip = 1; role SPADE (the fused
 * gamma | beta filter of mrdis_conv2d_fwd_spade): w_tck, R = Ci, S = 2 C, spadeC = C.  img: mrdis_wino_u_image_floats(R, S, spadeC) floats,
 * 16-byte aligned.  block0 / nblk: the job's block range (mrdis_wino_u_job_blocks each), total_blocks = their sum.                     */
size_t mrdis_wino_u_job_bytes(void);
int mrdis_wino_u_format(int R, int S, int spadeC);
long long mrdis_wino_u_image_floats(int R, int S, int spadeC);                 /* = _fmt(..., mrdis_wino_u_format(R, S, spadeC)) */
long long mrdis_wino_u_image_floats_fmt(int R, int S, int spadeC, int fmt);
int mrdis_wino_u_job_blocks(int R, int S, int spadeC);
int mrdis_wino_u_jobs(const void* jobs, int njobs, int total_blocks, void* stream);

/* Six-product filter image (option split6; mrdis_s6conv.hip): the layers without a Winograd form -- the 4x4 / 3x3 stride-2 convolutions of the encoders,
 * F.conv2d at model.py:2104 -- multiply on the bf16 matrix pipe with both fp32 operands split into three bf16 terms (the six products of order <= 2,
 * fp32 accumulation: fp32-equivalent results).  The filter is split ONCE into this image; the convolution entry points take it through their w_wino
 * argument with w_wino_fmt = 6 (fp32 views only; without it, or where the geometry does not fit, the fp32 MFMA kernels run).
 * w = [taps][Cred][Cout] fp32: role forward: w_tck (Cred = Ci, Cout = Co); role data gradient: w_tkc (Cred = Co, Cout = Ci).
 * image: mrdis_s6_filter_image_bytes(taps, Cred, Cout) bytes, 16-byte aligned (0: Cred is not a multiple of 8).                                  */
size_t mrdis_s6_filter_image_bytes(int taps, int Cred, int Cout);
int mrdis_s6_filter_image(const float* w, int taps, int Cred, int Cout, void* image, size_t image_bytes, void* stream);

/* data gradient (autograd convolution_backward, input part).
 * dy view (N,Ho,Wo,Co) ld=lddy -> dx view (N,H,W,Ci) ld=lddx ; w_tkc layout. */
int mrdis_conv2d_bwd_data(const void* dy, int lddy, const float* w_tkc, const void* w_bf16_tck,
                          void* dx, int lddx, int N, int H, int W, int Ci, int Co,
                          int kh, int kw, int stride, int pad, int dtype, const float* w_wino /* role data gradient, or NULL */, int w_wino_fmt, void* stream);

/* fp32 -> bf16, round to nearest even (the bf16 filter copies above); src 16-byte, dst 8-byte aligned. */
int mrdis_cast_bf16(const float* src, void* dst_bf16, long long n, void* stream);
/* NHWC view cast (P rows; ld in ELEMENTS of the respective type) between the storage types, optionally changing the channel
 * count: the first min(C_src, C_dst) channels are copied, the rest of a wider destination is zero.  The boundary between bf16
 * activations and the fp32-only tensors: e.g. the 4-channel anatomy map -> a 16-channel bf16 view the bf16 MFMA kernels accept,
 * and a 16-channel bf16 head output -> its first 7 channels in fp32.  Any combination of MRDIS_DT_F32 / MRDIS_DT_BF16.          */
int mrdis_cast_view(const void* src, int ld_src, int src_dtype, int C_src, void* dst, int ld_dst, int dst_dtype, int C_dst,
                    long long P, void* stream);

/* Word-wise copy src -> dst by a kernel (nbytes % 4 == 0, 4-byte aligned).  src may be pinned host memory: the way small
 * host -> device transfers inside a step avoid the copy engine's host round trip (the reference's CPU-drawn eps, model.py:3159-3162). */
int mrdis_copy_bytes(const void* src, void* dst, long long nbytes, void* stream);
/* Measurement probe: fills n_floats (multiple of 4, 16-byte aligned) with `value` by non-temporal 16-byte stores and reads nothing: the rate a store-only kernel
 * reaches on this device (bench.py reports it beside the north-star convolution, whose traffic is 89 % stores). */
int mrdis_stream_fill(float* dst, long long n_floats, float value, void* stream);

/* A SPADE block's  InstanceNorm(z) * (1 + gamma(s)) + beta(s)  (model.py:2440-2446) with the gamma | beta convolution and the modulation in
 * ONE launch: x = the si_layers output (N, H, W, Ci), w_tck = the fused [9][Ci][2 C] filter (gamma couts first), bias (2 C), z (N, H, W, C)
 * and its instance statistics (mrdis_instnorm_stats).  Writes mix and gamma (the backward, mrdis_instnorm_spade_bwd, needs gamma).
 * dtype MRDIS_DT_F32 (x, z, mix, gamma fp32; w_tck) or MRDIS_DT_BF16 (bf16 views; w_bf16_tkc = the bf16 [9][2 C][Ci] filter).
 * MRDIS_EUNSUPPORTED where the pipelined kernels are not the kernels of choice: run mrdis_conv2d_fwd + mrdis_instnorm_spade_fwd instead. */
int mrdis_instnorm_stats(const void* z, int ldz, float* save_mean, float* save_rstd, void* workspace, size_t workspace_bytes,
                         int N, long long HW, int C, float eps, int dtype, void* stream);
int mrdis_conv2d_fwd_spade(const void* x, int ldx, const float* w_tck, const void* w_bf16_tkc, const float* bias, const void* z, int ldz,
                           const float* mean, const float* rstd, void* mix, int ldmix, void* gamma, int ldg,
                           int N, int H, int W, int Ci, int C, int dtype, const float* w_wino /* role SPADE, or NULL */, int w_wino_fmt /* 2 | 4 */, void* stream);

/* weight gradient.  Two-pass, bit-reproducible: partial slabs in `workspace`
 * (size from mrdis_conv2d_bwd_weight_workspace) then an ordered reduction.
 * dw_tck: [T][Ci][Co] ; dbias (Co) or NULL.                                   */
size_t mrdis_conv2d_bwd_weight_workspace(int N, int H, int W, int Ci, int Co,
                                         int kh, int kw, int stride, int pad);
/* accumulate_bias != 0: dbias += column sums of dy (instead of =), e.g. straight into the parameter's gradient.
 * dtype MRDIS_DT_F32_BF16M: x and dy are rounded to bf16 on their way into LDS and multiplied on bf16 MFMA with fp32
 * accumulation (stride-1 "same" layers with Ci % 32 == 0; others run the fp32 kernels); dbias stays an fp32 sum.       */
int mrdis_conv2d_bwd_weight(const void* x, int ldx, const void* dy, int lddy,
                            float* dw_tck, float* dbias, void* workspace, size_t workspace_bytes,
                            int N, int H, int W, int Ci, int Co,
                            int kh, int kw, int stride, int pad, int accumulate_bias, int dtype, void* stream);

/* ---- LeakyReLU backward (model.py:2227/2240, 2375-2394): dx = dy * (y>0 ? 1 : slope),
 * y being the activation OUTPUT (sign-preserving for slope > 0).              */
int mrdis_lrelu_bwd(const void* dy, int lddy, const void* y, int ldy, void* dx, int lddx,
                    long long P, int C, float slope, int dtype, void* stream);

/* ---- BatchNorm2d, training mode: model.py:2132/2151, 2179/2191, 2776-2785 --
 * x view (P = N*H*W rows, C) ; writes y view, save_mean/save_rstd (C) and
 * updates running_mean/var (momentum 0.1, unbiased var) when non-NULL.
 * groups = G > 1: the view holds G batches of P rows that the reference normalises in G separate calls of the SAME layer (the
 * modalities of one encoder pass, model.py:3135-3157): statistics per group (save_mean / save_rstd, and dgamma / dbeta of the
 * backward, hold G * C entries), the running statistics are updated group by group in order, rounded to fp32 in between.
 * workspace: groups * mrdis_norm_workspace(1, P, C) bytes (each group is chunked as a call of its own: bit-identical statistics). */
size_t mrdis_norm_workspace(int groups, long long P, int C);
int mrdis_bn_train_fwd(const void* x, int ldx, void* y, int ldy, const float* gamma,
                       const float* beta, float* running_mean, float* running_var,
                       float* save_mean, float* save_rstd, void* workspace, size_t workspace_bytes,
                       long long P, int C, float eps, float momentum, int groups, int dtype, void* stream);
/* inference mode (model.eval(), main_missing.py:338): y = (x - running_mean) * rsqrt(running_var + eps) * gamma + beta */
int mrdis_bn_eval_fwd(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var, long long P, int C, float eps, int dtype, void* stream);
/* acc_dgamma / acc_dbeta (both or neither): running parameter-gradient sums this call's dgamma / dbeta are
 * added to in the same launch (a module called several times per step needs no separate accumulation).   */
int mrdis_bn_train_bwd(const void* dy, int lddy, const void* x, int ldx, const float* gamma,
                       const float* save_mean, const float* save_rstd, void* dx, int lddx,
                       float* dgamma, float* dbeta, float* acc_dgamma, float* acc_dbeta,
                       void* workspace, size_t workspace_bytes, long long P, int C, int groups, int dtype, void* stream);

/* ---- InstanceNorm2d(affine=False) fused with the SPADE modulation:
 * model.py:2431/2440 + 2446:  out = IN(z) * (1 + gamma) + beta ---------------
 * z, gamma, beta, out : (N, HW, C) views ; save_mean/save_rstd : (N*C), written -- or, with workspace = NULL, READ: the
 * statistics of z are then taken from them (mrdis_bilinear_up2_stats_fwd computed them when z was produced).            */
int mrdis_instnorm_spade_fwd(const void* z, int ldz, const void* gamma, int ldg,
                             const void* beta, int ldb, void* out, int ldo,
                             float* save_mean, float* save_rstd, void* workspace, size_t workspace_bytes,
                             int N, long long HW, int C, float eps, int dtype, void* stream);
size_t mrdis_instnorm_spade_bwd_workspace(int N, long long HW, int C);
int mrdis_instnorm_spade_bwd(const void* dout, int lddo, const void* z, int ldz,
                             const void* gamma, int ldg, const float* save_mean, const float* save_rstd,
                             void* dz, int lddz, void* dgamma, int lddg, void* dbeta, int lddb,
                             void* workspace, size_t workspace_bytes,
                             int N, long long HW, int C, int dtype, void* stream);
/* The same backward when z = nn.Upsample(scale_factor=2, bilinear)(x) (model.py:2551-2573 in front of a SPADE block): z, dout, gamma, dgamma, dbeta
 * are (N, 2 Hi, 2 Wi, C); dx (N, Hi, Wi, C) receives the gradient of x -- the apply pass and the resize's adjoint in one kernel, the full-resolution
 * d z is neither written nor read back.  xlo != NULL: x itself (N, Hi, Wi, C); z may then be NULL -- both passes interpolate z from x exactly as
 * mrdis_bilinear_fwd stored it, so the up-sampled map need not be kept for the backward.  Workspace: ALWAYS size it with
 * mrdis_instnorm_spade_bwd_up2_workspace (>= mrdis_instnorm_spade_bwd_workspace(N, 4 Hi Wi, C), which is all the two-pass form needs: with the
 * smaller size the entry point takes the two-pass form).  MRDIS_EUNSUPPORTED: views that are not 16-byte aligned / C % 4 != 0 / a last 32-channel chunk
 * whose width is not 4, 8, 16 or 32 (the caller runs mrdis_instnorm_spade_bwd + mrdis_bilinear_bwd).
 * With xlo and a workspace of mrdis_instnorm_spade_bwd_up2_workspace(N, Hi, Wi, C, dtype) bytes: ONE pass over the full-resolution tensors -- d z is linear
 * in (dzh, 1, zh) and so is the resize's adjoint, so the kernel writes U^T dzh and the partial sums, and a kernel over the LOW-resolution map finishes
 * d x = rstd (U^T dzh - 4 s0 / HW - (s1 / HW) rstd (U^T U x - 4 mean)): dout and gamma are read once, z never (bf16 maps: U^T dzh travels in fp32
 * through the workspace). */
size_t mrdis_instnorm_spade_bwd_up2_workspace(int N, int Hi, int Wi, int C, int dtype);
int mrdis_instnorm_spade_bwd_up2(const void* dout, int lddo, const void* z, int ldz,
                                 const void* gamma, int ldg, const float* save_mean, const float* save_rstd,
                                 void* dx, int lddx, void* dgamma, int lddg, void* dbeta, int lddb,
                                 void* workspace, size_t workspace_bytes,
                                 int N, int Hi, int Wi, int C, const void* xlo, int ldxlo, int dtype, void* stream);

/* ---- bilinear resize: nn.Upsample at model.py:2175 (align_corners=True),
 * 2432 / 2501-2509 (align_corners=False, arbitrary output size) --------------*/
int mrdis_bilinear_fwd(const void* x, int ldx, void* y, int ldy, int N, int Hi, int Wi,
                       int Ho, int Wo, int C, int align_corners, int dtype, void* stream);
/* nn.Upsample(scale_factor=(2,2), bilinear) between two SPADE blocks (model.py:2551-2573, 2622-2627) together with the InstanceNorm
 * statistics of its result (model.py:2440): y (N, 2 Hi, 2 Wi, C) as mrdis_bilinear_fwd(align_corners = 0) writes it, save_mean /
 * save_rstd (N*C) as mrdis_instnorm_stats would compute them from y -- taken from the values while they are stored, so the 4x tensor
 * is not read back for a statistics pass.  C % 4 == 0, 16-byte aligned views; MRDIS_EUNSUPPORTED otherwise.  The consumer passes the
 * statistics on: mrdis_conv2d_fwd_spade takes them as arguments, mrdis_instnorm_spade_fwd with workspace = NULL uses the ones in
 * save_mean / save_rstd instead of computing them.                                                                                */
size_t mrdis_bilinear_up2_stats_workspace(int N, int Hi, int C);
/* 1 where mrdis_bilinear_up2_stats_fwd takes (N, Wi, C) on dense aligned views, 0 where it would return MRDIS_EUNSUPPORTED (callers choose their path beforehand) */
int mrdis_bilinear_up2_stats_applies(int N, int Wi, int C);
int mrdis_bilinear_up2_stats_fwd(const void* x, int ldx, void* y, int ldy, int N, int Hi, int Wi, int C,
                                 int out_block, long long out_block_stride,
                                 float* save_mean, float* save_rstd, float eps, void* workspace, size_t workspace_bytes,
                                 int dtype, void* stream);
/* out_block = 0 (or >= N): y is the dense (N, 2 Hi, 2 Wi, ldy) view.  0 < out_block < N (N % out_block == 0): the N images leave as
 * N / out_block blocks of out_block images, block k at y + k * out_block_stride elements (dense inside a block) -- the shared SPADE decoder
 * writes its result for modality label j straight into the [decoder i][label j] arrangement the per-modality decoders read (model.py:3200-3224),
 * which was a concatenation copy of 268 MB per decoder call.                                                                            */
int mrdis_bilinear_bwd(const void* dy, int lddy, void* dx, int lddx, int N, int Hi, int Wi,
                       int Ho, int Wo, int C, int align_corners, int dtype, void* stream);

/* ---- softmax over [100*mask_img, s] with channel 0 dropped: model.py:3150-3153
 * s view (P, C) ; mask_img (P) ; out view (P, C).                             */
int mrdis_softmax_mask_drop_fwd(const float* s, int lds, const float* mask_img, float* out, int ldo,
                                long long P, int C, float mask_scale, void* stream);
int mrdis_softmax_mask_drop_bwd(const float* dout, int lddo, const float* out, int ldo,
                                float* ds, int ldds, long long P, int C, void* stream);

/* ---- per-sample mean |gt - x| (p=1) or (gt-x)^2 (p=2) over (C,H,W):
 * model.py:3260-3266.  out (N).  bwd: dx = w[n] * d|.|/dx / (C*HW).           */
size_t mrdis_recon_err_workspace(int N, long long HW, int C);
int mrdis_recon_err_fwd(const float* gt, int ldgt, const float* x, int ldx, float* out,
                        void* workspace, size_t workspace_bytes,
                        int N, long long HW, int C, int p, void* stream);
int mrdis_recon_err_bwd(const float* gt, int ldgt, const float* x, int ldx, const float* w,
                        float* dx, int lddx, int N, long long HW, int C, int p, void* stream);

/* ---- evaluate() reconstruction metrics on the device: util.py:935-978
 * (compute_reconstruction_metrics[_single], called at main_missing.py:528).
 * n_img images of H x W: image i, pixel p at target[(i*H*W + p) * ldt] (i.e. channel 0
 * of an NHWC view).  Both images are shifted by their own minimum, data range = max of
 * the shifted target.  out (n_img, 3) = { MSE (the reference's 'rmse' key), PSNR, SSIM }.
 * SSIM follows skimage.metrics.structural_similarity defaults (7x7 uniform window,
 * sample covariance, K1 0.01, K2 0.03, mean over the window-valid region).            */
size_t mrdis_recon_metrics_workspace(int n_img, int H);
int mrdis_recon_metrics(const float* target, int ldt, const float* pred, int ldp, float* out,
                        void* workspace, size_t workspace_bytes, int n_img, int H, int W, void* stream);

/* ---- batch assembly from HBM-resident volumes: ZeroDoseDataset.__getitem__ + default collate
 * (util.py:471-566).  vol_ptrs (B, M): device pointers (as 64-bit integers, 0 = contrast missing for that subject)
 * to volumes stored as [D][H][W] planes; slice_idx (B): centre slice, already clamped to [block, D-1-block];
 * drop (B): contrast zeroed by the drop-off augmentation or -1.  All three live in device memory.
 * inputs: NHWC view (B,H,W,ld_in), channel m*(2*block+1)+k = slice slice_idx-block+k of contrast m;
 * mask (B, M); mask_img (B,H,W) = (inputs[:,0] == 0).                                              */
int mrdis_slice_gather(const void* vol_ptrs, const int* slice_idx, const int* drop, float* inputs, int ld_in,
                       float* mask, float* mask_img, int B, int M, int H, int W, int D, int block, void* stream);

/* ---- batch assembly for the 3-D nets: ZeroDoseDataset3D.__getitem__ + default collate (util.py:723-810) in one launch.
 * Volumes are stored as the reference's h5 file has them, (H, W, D) fp32 with D fastest.  table (B, ld_table) 64-bit words in
 * device memory, ld_table >= 2 M + 3, per sample: [0, M) volume pointers (0 = contrast missing or dropped), [M, 2M) pointers
 * to those volumes' fp32 minima inside the depth crop, [2M] target volume pointer (0 = none), [2M+1] bit 0 = flip the H axis,
 * bit 1 = augment, [2M+2] fp32 bits of scale (low word) and shift (high word).
 * mode 0: out (B, H, W, Dz, M) (channels-last-3d view of (B, M, H, W, Dz)) = crop [z0, z0 + Dz) of every contrast, zeros where
 *   absent; with the augment bit v = x * scale + shift (fp32, two roundings) and -10 where the raw value equals the item's raw
 *   minimum (= `inputs[inputs == inputs.min()] = -10`, see mrdis_volgather.hip); mask (B, M) or NULL = pointer present.  K = 0.
 * mode 1: targets from the [2M] volume, same crop and flip, zeros if absent, label 4 -> 3 if `relabel`; K = 0: out (B, H, W, Dz);
 *   K >= 1: out (B, H, W, Dz, K), channel c = (label == c + 1).
 * M, K <= 64, any H, W, Dz >= 1 (H W D < 2^31).  One kernel launch per call, counted as "volgather".                           */
int mrdis_volume_gather(const void* table, int ld_table, float* out, float* mask, int B, int M, int H, int W, int D, int z0,
                        int Dz, int mode, int K, int relabel, void* stream);

/* ---- patch training for the 3-D nets (csrc/mrdis_patch.hip): random (PH, PW, PD) sub-volumes of the whole stored (H, W, D) volume, a share
 * of them centred on a voxel of a foreground class.  This package's conventions (the reference trains on one fixed depth crop).
 * classes: K host integers in 1 .. 255, distinct (BraTS: 1, 2, 4); K <= MRDIS_PATCH_MAX_CLASSES.  nblk = ceil(H W D / 1024).
 * mrdis_fg_block_counts: counts (nblk, K) int32, counts[j][c] = the voxels with seg == classes[c] among the flat indices
 *   (h W + w) D + d in [1024 j, 1024 j + 1024).  K >= 1.  The caller makes the exclusive prefix (nblk + 1, K) of it, once per subject.
 * table (B, ld_table) 64-bit words in device memory, ld_table >= 2 M + 7: the 2 M + 3 words of mrdis_volume_gather (the minima are those of
 *   the WHOLE volumes), then [2M+3] pointer to the subject's int32 prefix table (0 = none), [2M+4] u_class | u_voxel << 32,
 *   [2M+5] u_h | u_w << 32, [2M+6] u_d (uint32 draws); flag word [2M+1]: bit 0 flip H, bit 1 augment, bit 2 flip W, bit 3 flip D,
 *   bit 4 foreground sample, bit 5 centre patch.
 * mrdis_patch_origins: origins (B, 4) int32 = h0, w0, d0, index of the chosen class (-1 = none), with pick(u, n) = (u n) >> 32:
 *   centre bit: h0 = (H - PH) / 2, likewise w0, d0.  Otherwise uniform: h0 = pick(u_h, H - PH + 1), likewise w0, d0; a foreground sample with a
 *   label volume, a prefix table and a class of non-zero total instead takes class = present[pick(u_class, |present|)] (present classes in
 *   list order), the r-th voxel (r = pick(u_voxel, n_class), 0-based, increasing flat index) of that class as centre (hc, wc, dc) and
 *   h0 = clamp(hc - PH / 2, 0, H - PH), likewise w0, d0.  K = 0 (classes may be NULL): always uniform.  One workgroup per sample.
 * mrdis_patch_gather: mode, K, relabel, out and mask as mrdis_volume_gather with (PH, PW, PD) for (H, W, Dz), read at the sample's origin
 *   (clamped into the volume) and mirrored inside the patch on every axis whose flip bit is set.
 * A patch larger than the volume on any axis: MRDIS_EINVAL (no padding).  One launch per call, counted as "fgcount" / "patchorigin" /
 * "patchgather"; no host read, no atomics: the same bits on every run.                                                        */
#define MRDIS_PATCH_MAX_CLASSES 8
int mrdis_fg_block_counts(const float* seg, const int* classes, int K, int* counts, int H, int W, int D, void* stream);
int mrdis_patch_origins(const void* table, int ld_table, int* origins, const int* classes, int K, int B, int M, int H, int W, int D, int PH,
                        int PW, int PD, void* stream);
int mrdis_patch_gather(const void* table, int ld_table, const int* origins, float* out, float* mask, int B, int M, int H, int W, int D,
                       int PH, int PW, int PD, int mode, int K, int relabel, void* stream);

/* ---- rotated and zoomed training patches (csrc/mrdis_warp.hip): mrdis_patch_gather with an affine resampling of the samples whose warp bit
 * is set.  This package's conventions.  Parameters, out, mask, mode, K, relabel and the return codes are mrdis_patch_gather's, except
 * ld_table >= 2 M + 12 (else MRDIS_EINVAL): the 2 M + 7 words above, flag word [2M+1] bit 6 = warp, and [2M+7 .. 2M+11] the nine entries
 * a[r][c] of a 3 x 3 matrix in Q16 (int32, row-major, two per word, the low half first; the last high half is 0).
 * Source coordinate of output voxel o (after the flip rule: o' = P - 1 - o on a flipped axis), integers in units of 2^-17 voxel, 64-bit:
 *   s[r] = ((2 origin[r] + P[r] - 1) << 16) + sum_c a[r][c] (2 o'[c] - (P[c] - 1))
 *   floor index i0 = s >> 17, fraction f = s & (2^17 - 1), nearest index = (s + 2^16) >> 17
 * (a rotation about the centre of the unwarped patch).  Every corner index i0, i0 + 1 and the nearest index are clamped per axis into the
 * volume (edge replication); the entries are clamped to +-2^18 first, so no table can send a read outside a volume.
 * mode 1: the raw label at the nearest index, then relabel and the region channels as mrdis_patch_gather.
 * mode 0, per contrast (absent: every voxel reads 0), m0 the item's whole-volume minimum: with the augment bit, -10 exactly where the voxel
 *   at the nearest index equals m0; elsewhere every one of the eight corners that equals m0 takes the nearest voxel's value, the corners
 *   are interpolated along d, then w, then h as a + (f / 2^17) (b - a) in fp32 (three roundings each, no fused multiply-add), and
 *   x * scale + shift follows (two roundings).  Without the augment bit: the interpolated raw corners.
 * A sample with the warp bit clear is mrdis_patch_gather's, bit for bit.  One launch per call, counted as "patchwarp"; no atomics.     */
#define MRDIS_PATCH_WARP_FLAG 64
int mrdis_patch_warp(const void* table, int ld_table, const int* origins, float* out, float* mask, int B, int M, int H, int W, int D,
                     int PH, int PW, int PD, int mode, int K, int relabel, void* stream);

/* ---- intensity augmentation of the gathered training patches (csrc/mrdis_tone.hip): Gaussian blur, contrast, gamma and additive noise.  This
 * package's conventions (the reference has none).  x, y: (B, PH, PW, PD, M) dense fp32, the layout mrdis_patch_gather / mrdis_patch_warp write;
 * scale, shift and the marker rule are already applied.  A voxel is BACKGROUND iff its value equals -10.0f exactly, every other one is
 * tissue; background voxels leave every call as -10 exactly and enter no sum.  An item or contrast without a flag leaves all three calls bit
 * for bit as it went in.  Any M in 1 .. 64, any extents >= 1 with PH PW PD < 2^31, B in 1 .. 65535.
 * table (B, ld_table) 64-bit words in device memory; the calls read the block of 1 + 5 M words at word `col` of a row (after the 2 M + 7 or
 *   2 M + 12 words of the gathers): word 0 = seed_lo | seed_hi << 32, then five words per contrast as ten 32-bit halves, the low half first:
 *   flags, g0, g1, g2, g3, g4, f, gamma, std, 0 (fp32 bits but for the flags).  Flag bits: MRDIS_TONE_BLUR 1, MRDIS_TONE_CONTRAST 2,
 *   MRDIS_TONE_GAMMA 4, MRDIS_TONE_INVERT 8 (the inverted gamma curve), MRDIS_TONE_NOISE 16.  The taps are
 *   g[t] = exp(-t^2 / (2 sigma^2)) / (g'0 + 2 sum_{t=1..4} g'[t]) (g' the unnormalised ones), float64 on the host, rounded once to fp32.
 * mrdis_patch_blur, out of place (x == y: MRDIS_EINVAL).  A contrast with the blur flag clear: y = x bit for bit.  A flagged one: the
 *   normalised convolution over tissue, m = (x != -10), xm = m ? x : 0.  Three passes along d, then w, then h, starting from N = xm, D = m:
 *   N'[p] = sum_t g[|t|] N[p + t e] and D'[p] = sum_t g[|t|] D[p + t e], e the pass's axis, t = -4 .. 4 in increasing order, each sum an fp32
 *   fmaf chain from 0 over the t with p + t e inside the patch (nothing is padded: the patch border renormalises as the background does).
 *   After the third pass y = m ? N / D : -10 (D > 0 wherever m holds: g0 > 0).  Launches: 2 where M == 4 and x and y are 16-byte aligned
 *   (a voxel's four contrasts as one 16-byte access), else 3; 3 always under the debug_volgen switch.  Both forms give the same bits.
 * mrdis_patch_stats: stats (B, M, 4) 32-bit words = fp32 lo (minimum over tissue), fp32 hi (maximum), fp32 mean = (float)(sum / n) with the
 *   sum in float64 in a fixed order, int32 n (tissue count); n = 0: the first three are 0.  2 launches; no atomics: two runs give the same bits.
 * mrdis_patch_tone, in place on tissue voxels, per contrast, each step only where its flag is set, in this order:
 *   contrast  v = min(max(fmaf(v - mean, f, mean), lo), hi)
 *   gamma     only if hi > lo: rg = hi - lo, t = min(max((v - lo) / rg, 0), 1); inverted: t = 1 - t; t = powf(t, gamma); inverted: t = 1 - t;
 *             v = fmaf(t, rg, lo)
 *   noise     v = fmaf(std, z, v), z = (float)(2 S - 4080) * C, S the integer sum of the 16 bytes of Philox4x32-10 (multipliers 0xD2511F53,
 *             0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) on the counter (p, m, 0, 0), p = (i PW + j) PD + k the voxel's flat index in
 *             the patch, under the key (seed_lo, seed_hi); C = 0x3addb446, the fp32 nearest to 349520^-1/2: mean 0, variance 1, |z| < 6.91.
 *   1 launch.
 * Refused before any launch: a NULL pointer, x == y, col < 0, ld_table < col + 1 + 5 M, B < 1, M outside 1 .. 64, an extent < 1 (MRDIS_EINVAL);
 * B > 65535 or PH PW PD >= 2^31 (MRDIS_EUNSUPPORTED); x, y or stats not 4-byte, table not 8-byte, workspace not 16-byte aligned (MRDIS_EALIGN);
 * a workspace below the query's size (MRDIS_EWORKSPACE).  Counted once per call as "patchblur" / "patchstats" / "patchtone".               */
#define MRDIS_TONE_BLUR 1
#define MRDIS_TONE_CONTRAST 2
#define MRDIS_TONE_GAMMA 4
#define MRDIS_TONE_INVERT 8
#define MRDIS_TONE_NOISE 16
size_t mrdis_patch_blur_workspace(int B, int M, int PH, int PW, int PD);
int mrdis_patch_blur(const float* x, float* y, const void* table, int ld_table, int col, int B, int M, int PH, int PW, int PD,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t mrdis_patch_stats_workspace(int B, int M, int PH, int PW, int PD);
int mrdis_patch_stats(const float* x, void* stats, int B, int M, int PH, int PW, int PD, void* workspace, size_t workspace_bytes, void* stream);
int mrdis_patch_tone(float* x, const void* stats, const void* table, int ld_table, int col, int B, int M, int PH, int PW, int PD, void* stream);

/* ---- objective of the 3-D nets (model3d.nvnet_loss) fused: soft Dice of sigmoid(uout) against `target`, GLOBAL over the batch, plus
 * w_l2 times the mean squared error of vout against x (csrc/mrdis_loss3d.hip).  uout / target: fp32 of one shape (shape_ut, nd_ut <= 8
 * extents) and ONE dense memory layout, given by their element strides; vout / x likewise with shape_vx, or both NULL for the Dice-only
 * form (UNet3D).  Strides that differ inside a pair return MRDIS_EINVAL, a layout with holes MRDIS_EUNSUPPORTED, a base that is not
 * 16-byte aligned MRDIS_EALIGN: nothing is ever copied.  Any element count (a tail of n % 4 floats is handled).
 * fwd: ONE pass over the four tensors + a one-workgroup finish.  sums (device, 4 doubles) = { sum p t, sum p^2, sum t^2, sum (v - x)^2 },
 *   p = sigmoid(uout); terms (device, 3 floats) = { dice = 1 - 2 sums[0] / (sums[1] + sums[2] + 1e-6), l2 = sums[3] / n_vx (0 without vout),
 *   dice + w_l2 l2 }, evaluated in fp64 and rounded once.  Fixed reduction order through `workspace` (16-byte aligned), no floating-point
 *   atomics: bit-identical from run to run.
 * bwd: ONE pass.  du = g [(-2 t / den + 4 sums[0] p / den^2) p (1 - p)], dv = g w_l2 2 (v - x) / n_vx, den = sums[1] + sums[2] + 1e-6,
 *   written in the layout of uout / vout; g (one float, the gradient of terms[2]) and sums are DEVICE pointers: no host sync.  du or dv
 *   may be NULL (not wanted).  Each call counts once as "loss3d".                                                                 */
size_t mrdis_nvnet_loss_workspace(long long n_ut, long long n_vx);
int mrdis_nvnet_loss_fwd(const float* uout, const long long* stride_u, const float* target, const long long* stride_t,
                         const long long* shape_ut, int nd_ut, const float* vout, const long long* stride_v, const float* x,
                         const long long* stride_x, const long long* shape_vx, int nd_vx, double w_l2, double* sums, float* terms,
                         void* workspace, size_t workspace_bytes, void* stream);
int mrdis_nvnet_loss_bwd(const float* uout, const long long* stride_u, const float* target, const long long* stride_t,
                         const long long* shape_ut, int nd_ut, const float* vout, const long long* stride_v, const float* x,
                         const long long* stride_x, const long long* shape_vx, int nd_vx, double w_l2, const double* sums,
                         const float* g, float* du, float* dv, void* stream);

/* ---- the integer counts behind the reference's Dice / IoU (compute_segmentation_metrics_single, util.py:980-992).  pred, target:
 * (B, P, C) fp32, channel fastest (channels-last-3d of (B, C, H, W, D)), target channel c = (label == c + 1).
 * out (B, C, 3) int32 += { |pred > 0.5 and target == 1|, |pred > 0.5|, |target == 1| } (strictly above 0.5); the caller zeroes `out`.
 * apply_sigmoid != 0: pred holds logits, the kernel compares sigmoid(pred).  C <= 4, P C < 2^31.  One launch, counted as "segcounts". */
int mrdis_seg_counts(const float* pred, const float* target, int* out, int B, long long P, int C, int apply_sigmoid, void* stream);

/* ---- whole-volume sliding-window prediction of the 3-D nets (csrc/mrdis_segvol.hip).  The overlap rule and the label rule are this
 * package's own convention, like the objective: the reference ships no 3-D inference.
 * mrdis_seg_accum: logits (B, H, W, Dz, C) fp32 (channels-last-3d view of the net's (B, C, H, W, Dz) output), acc (B, H, W, D, C) fp32,
 *   16-byte aligned: acc[b][h][w][z0 + k][c] += sigmoid(logits[b][h'][w][k][c]), h' = H - 1 - h if flip_h (the prediction of an H-flipped
 *   input, un-flipped), else h.  The sigmoid is the one of mrdis_seg_counts (accurate expf, IEEE division).  One thread owns an acc element
 *   within a launch and there are no atomics: windows add in launch order, bit-identical from run to run.  1 <= C <= 4, any H, W, Dz >= 1,
 *   0 <= z0 <= D - Dz (else MRDIS_EINVAL); B H W (Dz C + 6) / 4 < 2^31.  One launch, counted as "segaccum".
 * mrdis_seg_label_volume: acc as above; cover (D) int32, device: how many accumulations touched each depth (windows times flips);
 *   targets: B 64-bit device pointers (device memory) to raw (H, W, D) fp32 label volumes, 0 = none, or NULL = none for any sample.
 *   Per voxel pbar_c = acc_c / (float)cover[z] (IEEE fp32 division; cover 1: the sigmoid itself; cover 0: nothing is predicted there);
 *   counts (B, C, 3) int32 += { |pbar_c > 0.5 and t == c + 1|, |pbar_c > 0.5|, |t == c + 1| } (strictly above, t relabelled 4 -> 3 if
 *   `relabel`: the semantics of mrdis_seg_counts); the caller zeroes `counts`.  labels (B, H, W, D) uint8, 4-byte aligned: 0 if
 *   max_c pbar_c <= 0.5, else 1 + argmax_c pbar_c (lowest c on a tie), a 3 written as 4 if `relabel` (BraTS labels 0 / 1 / 2 / 4).
 *   1 <= C <= 4, H W D < 2^31.  One launch, counted as "seglabels".                                                                 */
int mrdis_seg_accum(const float* logits, float* acc, int B, int H, int W, int Dz, int D, int C, int z0, int flip_h, void* stream);
int mrdis_seg_label_volume(const float* acc, const int* cover, const void* targets, unsigned char* labels, int* counts, int B, int H,
                           int W, int D, int C, int relabel, void* stream);

/* ---- tile-wise prediction of the 3-D nets (csrc/mrdis_segvol.hip; model3d.predict_tiles).  The rule is this package's own convention: the
 * reference ships no 3-D inference.  Volume (H, W, D), tile (TH, TW, TD) <= the volume, nothing is padded.  Per axis the tile origins are
 * 0, S, 2 S, ... below n - T, then n - T; the tiles are the Cartesian product, visited with h0 outermost and d0 innermost.  The views of a
 * tile are the subsets of the mirrored axes, flag bits 1 (h) | 4 (w) | 8 (d) as in the gather table, in increasing binary count with the first
 * named axis (in h, w, d order) as the lowest bit; view 0 is the identity.  Weights are separable, one fp32 vector per axis (uniform: ones;
 * gaussian: exp(-0.5 ((x - (T - 1) / 2) / (sigma T))^2) evaluated in double, rounded once, clamped from below to 2^-20); the weight of tile
 * position (i, j, k) is (wh[i] * ww[j]) * wd[k] in fp32: two roundings, in that order.
 * mrdis_tile_accum: logits (B, TH, TW, TD, C) fp32 (channels-last-3d view of the net's output for one tile and view), acc (B, H, W, D, C) fp32,
 *   16-byte aligned, wh (TH) / ww (TW) / wd (TD) fp32 on the device:
 *     acc[b][h0 + i][w0 + j][d0 + k][c] = fmaf((wh[i] * ww[j]) * wd[k], sigmoid(logits[b][i'][j'][k'][c]), acc[b][h0 + i][w0 + j][d0 + k][c])
 *   with i' = TH - 1 - i if flips & 1, else i; j' by flips & 4 and k' by flips & 8 likewise: the prediction of a mirrored input, put back.  The
 *   weight is indexed by the position in the volume (i, j, k), not by the position in the net's output.  The sigmoid is mrdis_seg_accum's.
 *   One thread owns an acc element within a launch and there are no atomics: calls add in launch order, bit-identical from run to run.
 *   MRDIS_EINVAL: C outside 1 .. 4, a tile larger than the volume, an origin outside [0, n - T], flip bits other than 1 | 4 | 8, a null
 *   pointer; MRDIS_EALIGN: acc not 16-byte aligned; MRDIS_EUNSUPPORTED: B TH TW (TD C + 6) / 4 >= 2^31.  One launch, counted as "tileaccum".
 * mrdis_tile_label_volume: mrdis_seg_label_volume with the denominator den = (nh[h] * nw[w]) * nd[d] in fp32 in place of (float)cover[d] and
 *   pbar_c = den > 0 ? acc_c / den : 0.  nh (H) / nw (W) / nd (D) fp32 on the device: the tiles are a Cartesian product, so the summed weight of
 *   a voxel factorises; n_axis[x] = the sum over the axis' origins o of w_axis[x - o], summed in double from the fp32 weights and rounded once,
 *   the number of views multiplied into nd before that rounding.  With nh = nw = 1 and nd = cover it gives mrdis_seg_label_volume's bits.
 *   Labels, counts, targets, limits and alignment as there.  One launch, counted as "tilelabels".                                      */
int mrdis_tile_accum(const float* logits, float* acc, const float* wh, const float* ww, const float* wd, int B, int H, int W, int D, int TH,
                     int TW, int TD, int C, int h0, int w0, int d0, int flips, void* stream);
int mrdis_tile_label_volume(const float* acc, const float* nh, const float* nw, const float* nd, const void* targets, unsigned char* labels,
                            int* counts, int B, int H, int W, int D, int C, int relabel, void* stream);

/* ---- whole-subject synthesis of missing contrasts by the 2-D model (csrc/mrdis_synth.hip): slice blocks -> volume.  The block rule is this
 * package's own convention: the reference ships no such path.
 * mrdis_synth_accum: srcs: HOST array of n_src (1 .. MRDIS_SYNTH_MAX_SRC) device pointers, handed to the kernel by value; each a dense
 *   channels-last (B, C, H, W) fp32 reconstruction (memory [B][H][W][C]) of B samples with CONSECUTIVE centres s0, s0 + 1, ... (the caller
 *   checks that), C = 2b + 1.  Channel c of sample r predicts plane k = s0 + r + c - b.  For every plane k the batch predicts with a channel in
 *   [c_lo, c_hi] (b..b: the centre slice only; 0..2b: every prediction) and 0 <= k < D:
 *     acc[k][h][w] += the values src_j[r][c][h][w], added one by one in the order (r ascending -- c = k - s0 - r + b follows --, j ascending);
 *     cnt[k] += their number.
 *   acc (D, H, W) fp32, cnt (D) int32, both read and written.  A gather: one thread owns an acc element within a launch and there are no atomics,
 *   so batches add in launch order, bit-identical from run to run.  C odd, 0 <= c_lo <= c_hi < C (else MRDIS_EINVAL); H W < 2^31.  acc planes are
 *   accessed 16 bytes per lane when H W % 4 == 0 and acc is 16-byte aligned, else 4.  One launch, counted as "synthaccum".
 * mrdis_synth_finish: acc[d][h][w] = cnt[d] > 0 ? acc[d][h][w] / (float)cnt[d] : fill (IEEE fp32 division), in place, and the same values in the
 *   volume store's (H, W, D) layout: out[h][w][d].  The transpose goes through LDS (both sides coalesced for any D).  One launch, counted as
 *   "synthfinish".                                                                                                                          */
#define MRDIS_SYNTH_MAX_SRC 8
int mrdis_synth_accum(const float* const* srcs, int n_src, float* acc, int* cnt, int B, int C, int H, int W, int D, int s0, int c_lo, int c_hi,
                      void* stream);
int mrdis_synth_finish(float* acc, const int* cnt, float* out, int D, int H, int W, float fill, void* stream);

/* ---- whole-subject tumour segmentation by the 2-D model (csrc/mrdis_seg2d.hip; segment.segment_volumes): logits of a batch of consecutive
 * centre slices -> label planes of one volume per missing-contrast pattern ("set") -> the store's (H, W, D) volumes.  The label rule is this
 * package's own convention: the reference assembles no volume and never fuses for M > 1.
 * mrdis_seg2d_label_planes: views: HOST array of n_sets * n_views device pointers, set-major, handed to the kernel by value; each a dense
 *   channels-last (B, C, H, W) fp32 logit tensor (memory [B][H][W][C]) of B samples with CONSECUTIVE centres s0, s0 + 1, ...  flips: HOST array
 *   of n_views codes, 0 none | 1 H | 2 W: view v is the prediction of an input flipped along that axis and is read at the mirrored pixel.
 *   planes (n_sets, D, H, W) uint8: planes[s][s0 + r][h][w] = the label of pixel (h, w) of sample r of set s; exactly the bytes of planes
 *   s0 .. s0 + B - 1 of every set are written, nothing else.
 *     one view:  argmax_c y_c over the logits themselves (no exp), the lowest c on a tie;
 *     two views: p_c = 0.5 (softmax(y^0)_c + softmax(y^1)_c), each softmax exp(y_c - max) / sum in fp32 (accurate expf, IEEE division, the sum
 *                in increasing c); argmax_c p_c, the lowest c on a tie.
 *   Class c is written as label c, a 3 as 4 if `relabel` (BraTS labels 0 / 1 / 2 / 4).  No atomics, one owner per byte: the same bits from run
 *   to run.  2 <= C <= 4, 1 <= n_sets <= MRDIS_SEG2D_MAX_SETS, 1 <= n_views <= MRDIS_SEG2D_MAX_VIEWS, 0 <= s0, s0 + B <= D, H W < 2^31, flip
 *   codes in 0 .. 2: anything else returns MRDIS_EINVAL before any launch.  The logits are read 16 bytes per lane when C == 4 and every view is
 *   16-byte aligned, else 4 (a view that is not 4-byte aligned: MRDIS_EALIGN); the stores are coalesced along w.  ONE launch whatever n_sets,
 *   counted as "seg2dlabels".
 * mrdis_seg2d_finish: out[s][h][w][d] = planes[s][d][h][w], (n_sets, D, H, W) uint8 -> (n_sets, H, W, D) uint8, through LDS (both sides
 *   coalesced for any D).  n_sets >= 1.  One launch whatever n_sets, counted as "seg2dfinish".                                          */
#define MRDIS_SEG2D_MAX_SETS 16
#define MRDIS_SEG2D_MAX_VIEWS 2
int mrdis_seg2d_label_planes(const float* const* views, int n_sets, int n_views, const int* flips, unsigned char* planes, int B, int C, int H,
                             int W, int D, int s0, int relabel, void* stream);
int mrdis_seg2d_finish(const unsigned char* planes, unsigned char* out, int n_sets, int D, int H, int W, void* stream);

/* ---- fusion of the anatomy maps over the contrasts a sample has (csrc/mrdis_fuse.hip; lambda_recon_y_fused).  The rule is this package's own
 * convention: the reference's `si_cat[mask == 1]` (model.py:3239-3258) never fuses and fails for M > 1.
 * srcs / ld_srcs: HOST arrays of K (1 .. MRDIS_FUSE_MAX_SRC) device pointers and pixel strides (floats), handed to the kernel by value; each
 *   source a (B, H, W, C) fp32 NHWC view.  mask: (B, K) fp32 contiguous ON THE DEVICE, present = 1.0f exactly; the kernels derive the present
 *   set and its size n_b from it, nothing per step is baked into the launch.  method: MRDIS_FUSE_MEAN | _MAX | _MEAN_MAX_MIN.
 * mrdis_fuse_present_fwd: out (B, H, W, F C) with pixel stride ldo >= F C, F = 3 for MRDIS_FUSE_MEAN_MAX_MIN ([mean | max | min]) else 1.  Over
 *   the present contrasts of sample b: mean = (the sum in increasing k) / (float)n_b (IEEE fp32 division), max, min.  One launch, every output
 *   element written once.  K = 1: the identity.
 * mrdis_fuse_present_bwd: dout as out; dsrcs / ld_dsrcs: K gradient views like the sources.  Every element of all K gradients is written once:
 *   0 for an absent contrast; mean: g / (float)n_b for every present k; max / min: g for the LOWEST present k that attains the extremum (recomputed
 *   from the maps, no saved index), 0 for the others; mean-max-min: the three contributions added in the order mean, max, min.  One launch.
 * A row of the mask without any present contrast gets zeros both ways (callers refuse it from the host mask).  16 bytes per lane when C % 4 == 0
 * and every pointer and stride allows it, else 4.  B <= 65535, H W < 2^31.  Each call counts once as "fuse".                              */
#define MRDIS_FUSE_MAX_SRC 8
#define MRDIS_FUSE_MEAN 0
#define MRDIS_FUSE_MAX 1
#define MRDIS_FUSE_MEAN_MAX_MIN 2
int mrdis_fuse_present_fwd(const float* const* srcs, const int* ld_srcs, int K, const float* mask, int method, float* out, int ldo, int B,
                           long long HW, int C, void* stream);
int mrdis_fuse_present_bwd(const float* dout, int lddo, const float* const* srcs, const int* ld_srcs, int K, const float* mask, int method,
                           float* const* dsrcs, const int* ld_dsrcs, int B, long long HW, int C, void* stream);

/* ---- region scoring of label volumes (csrc/mrdis_surfdist.hip): region surfaces, the exact squared Euclidean distance transform and the
 * histogram of surface distances behind the 95th-percentile Hausdorff distance (HD95).  Integer arithmetic throughout: exact, and the same
 * bits from run to run.  Volumes are (B, H, W, D), D contiguous; voxel spacing is isotropic, squared distances are integers in voxel units.
 * mrdis_region_surfaces: labels (B, H, W, D) uint8 as mrdis_seg_label_volume writes them, 4-byte aligned; targets: B 64-bit device pointers
 *   (device memory) to raw (H, W, D) fp32 label volumes, 0 = none, or NULL = none for any sample (the convention of mrdis_seg_label_volume);
 *   region_masks: HOST array of R (1 .. MRDIS_SURF_MAX_REGIONS) integers in 0 .. 255: a label value l in 0 .. 7 belongs to region r iff bit l
 *   of region_masks[r] is set; a value above 7, negative, or non-integral after the cast belongs to no region.  flags (B, H, W, D) uint8,
 *   4-byte aligned, every byte written: bit r = the voxel is a surface voxel of predicted region r, bit 4 + r = of ground-truth region r.  A
 *   surface voxel lies in the region and has at least one of its six face neighbours outside it; the volume border counts as outside.
 *   counts (B, R, 5) int32 += { |P and T|, |P|, |T|, surface voxels of P, surface voxels of T }; the caller zeroes `counts`.  A sample without
 *   ground truth keeps its ground-truth bits and T counts at 0.  H W D < 2^31, B <= 65535.  One launch, counted as "regsurf".
 * mrdis_edt_sq: src (B, H, W, D) uint8; src_masks: HOST array of S (1 .. MRDIS_EDT_MAX_SRC) bytes: a voxel is a feature of source s iff
 *   (src & src_masks[s]) != 0 (0xFF: a plain mask; 1 << k: bit k of the flags above).  out (S, B, H, W, D) int32, 16-byte aligned: the squared
 *   Euclidean distance to the nearest feature of the same source and batch item, 0 on a feature, MRDIS_EDT_FAR everywhere in an item without
 *   one.  Separable: a nearest-feature scan along D, then min_j (g[j] + (i - j)^2) along W and along H, brute force over an LDS-resident line.
 *   Each of H, W, D in 1 .. 1024 and (H-1)^2 + (W-1)^2 + (D-1)^2 < MRDIS_EDT_FAR, B <= 65535: anything else returns MRDIS_EINVAL.
 *   workspace: mrdis_edt_workspace bytes (0: unsupported geometry), 16-byte aligned.  Three launches whatever B and S, each counted as "edt".
 * mrdis_surface_hist: flags as mrdis_region_surfaces wrote them for R regions.  For region r, at every surface voxel of T adds 1 into
 *   hist[b][r][0][d2], d2 = the squared distance to the nearest surface voxel of P, and at every surface voxel of P into hist[b][r][1][d2],
 *   d2 to the nearest surface voxel of T; a direction whose source surface is empty adds nothing.  hist (B, R, 2, bins) int32,
 *   bins = (H-1)^2 + (W-1)^2 + (D-1)^2 + 1 (anything else: MRDIS_EINVAL); the caller zeroes it.  The distances are never stored: the histogram
 *   is the last pass of the transform of the 2 R surfaces.  workspace: mrdis_edt_workspace(2 R, ...) bytes.  Geometry as mrdis_edt_sq.  Three
 *   launches: two counted as "edt", the last as "surfhist".
 * The scores formed from counts and histograms on the host (surfdist.region_scores) follow THIS PACKAGE'S CONVENTION -- BraTS's region
 * definitions (WT = {1, 2, 4}, TC = {1, 4}, ET = {4}) are standard, the empty-region and percentile rules vary between toolkits.  N = H W D,
 * TN = N - P - T + I:  dice = 2 I / (P + T);  sensitivity = I / T, or 1 if T = 0;  specificity = TN / (N - T), or 1 if N = T.  The directed 95 %
 * distance from A to B is spacing * sqrt(k), k the smallest squared distance with 20 * cum[k] >= 19 * n_A (n_A surface voxels of A, cum the
 * running sum of its histogram row): the nearest rank, decided in integers, no interpolation; hd95 is the larger of the two directed distances.
 * Both regions empty: dice 1, hd95 0.  Exactly one empty: dice 0, hd95 = spacing * sqrt(H^2 + W^2 + D^2) (373.13 for BraTS geometry, the
 * challenge's penalty).  No ground truth for the sample: NaN in all four.                                                             */
#define MRDIS_EDT_FAR (1 << 30)
#define MRDIS_EDT_MAX_SRC 8
#define MRDIS_SURF_MAX_REGIONS 4
int mrdis_region_surfaces(const unsigned char* labels, const void* targets, const int* region_masks, int R, unsigned char* flags, int* counts,
                          int B, int H, int W, int D, void* stream);
size_t mrdis_edt_workspace(int S, int B, int H, int W, int D);
int mrdis_edt_sq(const unsigned char* src, const unsigned char* src_masks, int S, int* out, void* workspace, size_t workspace_bytes, int B,
                 int H, int W, int D, void* stream);
int mrdis_surface_hist(const unsigned char* flags, int R, int* hist, long long bins, void* workspace, size_t workspace_bytes, int B, int H,
                       int W, int D, void* stream);

/* ---- connected components of label volumes and the clean-up rules built on them (csrc/mrdis_cc.hip).  Integer arithmetic throughout: exact,
 * and the same bits from run to run.  Volumes are (B, H, W, D) uint8, D contiguous, as mrdis_seg_label_volume writes them.  A voxel is
 * FOREGROUND iff its label l is at most 7 and bit l of fg_mask is set (bit 0 must be clear, some bit of 1 .. 7 set, else MRDIS_EINVAL); every
 * other voxel, values above 7 included, is background and is never joined to anything.  connectivity: 6 (faces), 18 (faces and edges) or 26
 * (faces, edges and corners), else MRDIS_EINVAL.  Components never cross a sample and never wrap from the end of a D line, a W row or an H
 * plane into the start of the next.  B in 1 .. 65535, each of H, W, D in 1 .. 1024, H W D < 2^31: anything else returns MRDIS_EUNSUPPORTED
 * (checked before every other argument).
 * mrdis_cc_label: comp, size (B, H, W, D) int32, 4-byte aligned, every element written.  comp = -1 on background, on foreground the SMALLEST
 *   in-sample flat index (h W + w) D + d of the voxel's component: a canonical value, independent of scheduling.  size = the component's voxel
 *   count at its root voxel (where comp equals the voxel's own index), 0 everywhere else.  Block-local union-find in LDS over tiles of
 *   4 x 4 x 64 voxels, a lock-free merge of the tile faces (find both roots, atomicMin the larger root's parent; no workgroup waits for
 *   another), a compress-and-count pass: THREE launches whatever B, shape and content, each counted as "cclabel"; no host sync.
 * mrdis_cc_clean: the rules of postproc.clean_labels -- THIS PACKAGE'S CONVENTION -- on labels and the comp / size mrdis_cc_label made of them.
 *   (1) a component is kept iff its size >= min_voxels; with keep_largest = 1 only the largest component of the sample is a candidate (a size
 *   tie goes to the smaller root index) and it is kept iff its size >= min_voxels.  Voxels of components that are not kept become 0,
 *   background voxels pass through unchanged.  (2) n = the voxels of the sample whose label then equals et_label: if et_min_voxels > 0 and
 *   0 < n < et_min_voxels they become et_replace.  out (B, H, W, D) uint8 and stats (B, 6) int32 = { components found, components kept,
 *   foreground voxels, voxels removed, n, replaced (0 | 1) } are written whole (the kernels clear stats).  et_label, et_replace in 0 .. 7,
 *   thresholds >= 0, keep_largest 0 | 1, else MRDIS_EINVAL.  workspace: mrdis_cc_clean_workspace(B) bytes, 8-byte aligned.  Four launches
 *   whatever the arguments; one count of "ccclean" per call.                                                                              */
int mrdis_cc_label(const unsigned char* labels, int fg_mask, int connectivity, int* comp, int* size, int B, int H, int W, int D, void* stream);
size_t mrdis_cc_clean_workspace(int B);
int mrdis_cc_clean(const unsigned char* labels, const int* comp, const int* size, int min_voxels, int keep_largest, int et_label,
                   int et_min_voxels, int et_replace, unsigned char* out, int* stats, void* workspace, size_t workspace_bytes, int B, int H,
                   int W, int D, void* stream);

/* ---- lesion-wise scoring of label volumes (csrc/mrdis_lesion.hip): region membership planes, binary dilation, the matching of predicted
 * components to dilated ground-truth lesions and the per-lesion masks that mrdis_region_surfaces / mrdis_surface_hist then score.  Integer
 * arithmetic and integer atomics only: exact, and the same bits from run to run; no workgroup waits for another; the launches of a call do
 * not depend on the volumes' content.  Volumes are (B, H, W, D), D contiguous.  Geometry as mrdis_cc_label (B in 1 .. 65535, each of H, W, D
 * in 1 .. 1024, H W D < 2^31), anything else returns MRDIS_EUNSUPPORTED (checked before every other argument).
 * mrdis_region_planes: labels, targets, region_masks, R exactly as mrdis_region_surfaces takes them.  planes (B, H, W, D) uint8, 4-byte
 *   aligned, every byte written: bit r = the voxel lies in predicted region r, bit 4 + r = in ground-truth region r -- the membership
 *   mrdis_region_surfaces counts as |P| and |T|, voxel for voxel.  One launch, counted as "dilate".
 * mrdis_dilate: dst (B, H, W, D) uint8 = src dilated `iterations` (1 .. MRDIS_DILATE_MAX_ITERATIONS) times by the structuring element of
 *   `connectivity`: 6 (a voxel and its face neighbours), 18 (faces and edges: scipy's generate_binary_structure(3, 2)) or 26 (the full
 *   3 x 3 x 3 cube), else MRDIS_EINVAL.  Every bit of a byte dilates on its own: an output bit is the OR of that bit over the neighbourhood, so
 *   the eight planes of mrdis_region_planes dilate in one pass (a 0 / 1 or 0 / 255 mask stays one).  Outside the volume is background; nothing
 *   wraps around a border or crosses into another sample.  A workgroup stages a tile of 8 x 8 x 64 voxels and a halo of one voxel in LDS;
 *   ONE LAUNCH PER ITERATION, each counted as "dilate": src -> dst for one iteration, ping-pong between dst and the workspace for more.  src
 *   and dst must not alias.  workspace: mrdis_dilate_workspace bytes (B H W D for iterations >= 2, else 0; NULL allowed when 0).
 * mrdis_lesion_match: items are (sample, region) pairs, item = b R + r, R in 1 .. MRDIS_SURF_MAX_REGIONS, B R <= 65535.  planes (B, H, W, D) as
 *   mrdis_region_planes wrote them (undilated); comp_l, comp_p (B R, H, W, D) int32: what mrdis_cc_label made of the dilated ground-truth plane
 *   and of the predicted plane of every item (-1 on background, else the component's root index); rank_l, rank_p (B R, H, W, D) int32: AT A ROOT
 *   VOXEL the dense number of its component over the whole call, in (item, root index) order -- the caller's scan over size > 0; other voxels
 *   are not read.  first_p (B R) int32: the dense number of the item's first predicted component.  Lesion j = a component of a dilated plane.
 *   For every voxel inside lesion j: a predicted voxel of component k (k = its dense number - first_p[item], below 32 words) sets bit k % 32
 *   of bits[j][k / 32] by atomicOr; a ground-truth voxel adds 1 to tcount[j]; the root voxel stores root[j] = its index and item[j].  bits
 *   (n_lesions, words) and tcount (n_lesions) int32 are zeroed by the caller; root and item (n_lesions) are written whole when n_lesions is
 *   the number of lesions.  A rank outside 0 .. n_lesions - 1, or a k outside the row, touches nothing.  One launch, counted as "lesmatch".
 * mrdis_lesion_expand: the arrays of mrdis_lesion_match after it ran.  For lesions j0 .. j0 + n - 1 (n <= 65535, j0 + n <= n_lesions) writes
 *   stack_t[i] (n, H, W, D) uint8 = 1 on a ground-truth voxel of the lesion's region whose dilated component is lesion j0 + i, stack_s[i] = 1
 *   on a predicted voxel of that region whose component has its bit set in row j0 + i; 0 elsewhere.  Both 4-byte aligned, every byte
 *   written.  One launch, counted as "lesexpand".                                                                                          */
#define MRDIS_DILATE_MAX_ITERATIONS 8
int mrdis_region_planes(const unsigned char* labels, const void* targets, const int* region_masks, int R, unsigned char* planes, int B, int H,
                        int W, int D, void* stream);
size_t mrdis_dilate_workspace(int iterations, int B, int H, int W, int D);
int mrdis_dilate(const unsigned char* src, unsigned char* dst, int connectivity, int iterations, void* workspace, size_t workspace_bytes, int B,
                 int H, int W, int D, void* stream);
int mrdis_lesion_match(const unsigned char* planes, const int* comp_l, const int* rank_l, const int* comp_p, const int* rank_p,
                       const int* first_p, int words, int n_lesions, int* bits, int* tcount, int* root, int* item, int B, int R, int H, int W,
                       int D, void* stream);
int mrdis_lesion_expand(const unsigned char* planes, const int* comp_l, const int* rank_l, const int* comp_p, const int* rank_p,
                        const int* first_p, const int* bits, int words, const int* item, int n_lesions, int j0, int n, unsigned char* stack_s,
                        unsigned char* stack_t, int B, int R, int H, int W, int D, void* stream);

/* ---- max_pool2d(kernel k x k, stride k): model.py:3448-3451 ---------------- */
int mrdis_maxpool_fwd(const float* x, int ldx, float* y, int32_t* argmax, int N, int H, int W, int C,
                      int k, void* stream);
int mrdis_maxpool_bwd(const float* dy, const int32_t* argmax, float* dx, int lddx, int N, int H, int W,
                      int C, int k, void* stream);

/* ---- optimizer side: main_missing.py:272-278 (clip + finite check) and :118/:283
 * (Adam, amsgrad, L2 weight decay) over one flat fp32 parameter arena --------
 * sumsq_finite: out[0] += sum(g^2), out[1] += count(non-finite)  (zero `out` first). */
size_t mrdis_sumsq_workspace(void);
int mrdis_sumsq_finite(const float* g, long long n, float* out, void* workspace, size_t workspace_bytes,
                       void* stream);
/* One fused step.  norm_finite points at the device scalar pair written by mrdis_sumsq_finite (or NULL): with
 * max_norm > 0 the gradient is scaled by coef = min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6)) (clip_grad_norm_,
 * main_missing.py:272); the step is skipped on the device when the non-finite count is > 0 (the reference stops in pdb
 * there, :273-278), with max_norm = 0 the pair only gates.
 * step_count / step_state: bias correction uses the 1-based host `step_count`, or -- when step_state (device float[2]) is
 * given -- a device-side counter: [0] = steps applied (incremented by this call unless it is skipped), [1] = steps skipped
 * as non-finite; a skipped step does not advance the bias correction.  Either way 1 - beta^t is formed on the device: the
 * same count from the host or from step_state gives the same bits.
 * gates (n_gates <= 32): HOST arrays gate_ranges[2k], [2k+1] = index range [lo, hi) of the arena, gate_flag_index[k] = entry
 * of the DEVICE array gate_flags that gates it: a range whose flag is 0 is left untouched (torch's Adam skips parameters
 * whose grad is None: a decoder whose modality is absent from the whole batch).
 * gate_steps (DEVICE float[3 * n_flags], zero-initialised, or NULL; needs step_state): per-flag step counters.  torch's Adam
 * keeps `step` per parameter and does not advance it while the gradient is None, so the ranges of flag k are bias-corrected
 * with [k] = the number of applied steps in which flag k was set (incremented by this call); [n_flags ..) is scratch
 * for the (1 - beta1^t, sqrt(1 - beta2^t)) pairs.  NULL: gated ranges use the arena-wide counter.                  */
int mrdis_adam_amsgrad_step(float* p, const float* g, float* m, float* v, float* vmax,
                            long long n, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int step_count, float* step_state, const float* norm_finite,
                            float max_norm, float grad_scale, const long long* gate_ranges, const int* gate_flag_index,
                            int n_gates, const float* gate_flags, float* gate_steps, int n_flags, void* stream);

/* ==== 3-D path: the Conv3d / GroupNorm / Upsample layers of BasicBlock, UNet3D, VAEBranch and
 * NVNet3D (src/model.py:1856-2060).  Tensors are NDHWC fp32 views (torch.channels_last_3d); 1x1x1 convolutions go
 * through mrdis_conv2d_* on the (N*D, H, W) view. -------------------------------------------------------------- */

/* nn.Conv3d(k = 3, padding = 1, stride in {1,2}) (model.py:1861, 1864, 1969-1984): x (N,D,H,W,Ci) ld=ldx ->
 * y (N,Do,Ho,Wo,Co) ld=ldy.  w_tck [27][Ci][Co] with tap = (kd*3 + kh)*3 + kw (mrdis_mix_experts_fwd, E = 1, T = 27).
 * residual (same extents as y, ld=ldres) or NULL: y = conv + bias + residual -- BasicBlock's `x + residul`
 * (model.py:1873) in the epilogue.                                                                             */
int mrdis_conv3d_fwd(const float* x, int ldx, const float* w_tck, const float* bias, const float* residual, int ldres,
                     float* y, int ldy, int N, int D, int H, int W, int Ci, int Co,
                     int k, int stride, int pad, void* stream);
/* data gradient: dy (N,Do,Ho,Wo,Co) -> dx (N,D,H,W,Ci); w_tkc [27][Co][Ci] */
int mrdis_conv3d_bwd_data(const float* dy, int lddy, const float* w_tkc, float* dx, int lddx,
                          int N, int D, int H, int W, int Ci, int Co, int k, int stride, int pad, void* stream);
/* weight (+ bias) gradient: split-K slabs in `workspace`, ordered reduction; dw_tck [27][Ci][Co], dbias (Co) or NULL */
size_t mrdis_conv3d_bwd_weight_workspace(int N, int D, int H, int W, int Ci, int Co, int k, int stride, int pad);
int mrdis_conv3d_bwd_weight(const float* x, int ldx, const float* dy, int lddy, float* dw_tck, float* dbias,
                            void* workspace, size_t workspace_bytes,
                            int N, int D, int H, int W, int Ci, int Co, int k, int stride, int pad, void* stream);

/* nn.GroupNorm(G, C) followed by nn.ReLU (model.py:1859-1860, 1862-1863, 1889-1890) on (N, P = D*H*W, C) rows:
 * y = relu?((x - mean[n,g]) * rstd[n,g] * gamma + beta); biased variance, eps inside the sqrt.  save_mean /
 * save_rstd: (N, G).  The backward takes dy w.r.t. the ReLU output and recomputes the ReLU mask from x.          */
size_t mrdis_groupnorm_workspace(int N, long long P, int C, int G);
int mrdis_groupnorm_relu_fwd(const float* x, int ldx, float* y, int ldy, const float* gamma, const float* beta,
                             float* save_mean, float* save_rstd, void* workspace, size_t workspace_bytes,
                             int N, long long P, int C, int G, float eps, int relu, void* stream);
int mrdis_groupnorm_relu_bwd(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* beta,
                             const float* save_mean, const float* save_rstd, float* dx, int lddx,
                             float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                             int N, long long P, int C, int G, int relu, void* stream);
/* the same with a second gradient of x summed in: dx = (GroupNorm+ReLU backward) + add (add: (N, P, C) rows, ld = ldadd; NULL = none).  BasicBlock's input
 * x feeds the normalised branch AND the residual addition (model.py:1873): both gradients of x then leave in one pass instead of autograd's extra add.   */
int mrdis_groupnorm_relu_bwd_add(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* beta,
                                 const float* save_mean, const float* save_rstd, float* dx, int lddx,
                                 float* dgamma, float* dbeta, const float* add, int ldadd, void* workspace, size_t workspace_bytes,
                                 int N, long long P, int C, int G, int relu, void* stream);

/* nn.Upsample(scale_factor=2) (nearest, model.py:1995-2003, 1898-1911) fused with the skip addition of
 * UNet3D.forward (model.py:2029-2040): y (N,2D,2H,2W,C) = x[d/2,h/2,w/2] + skip (skip may be NULL); contiguous NDHWC.
 * Backward: dx = sum of the 8 children of dy (d skip = dy needs no kernel).                                       */
int mrdis_upsample2x_add_fwd(const float* x, const float* skip, float* y, int N, int D, int H, int W, int C, void* stream);
int mrdis_upsample2x_bwd(const float* dy, float* dx, int N, int D, int H, int W, int C, void* stream);

/* Nearest-neighbour search of the missing-modality evaluation (model.py:3396-3415 compute_nearest_neighbour_z_by_s /
 * compute_cosine, called per query from main_missing.py:414-426), csrc/mrdis_zsearch.hip.  For each query q < Q (Q <= 64):
 *   out_idx[q] = argmax over gallery rows n with gallery_label[n] != query_label[q] of
 *                cos(g_n, q) = sum g_n*q / (norm(g_n) * norm(q)),  norm(x) = max(sqrt(sum x^2 + 1e-8), 1e-8),
 *   out_cos[q] = that cosine; equal cosines: the smaller n (torch.argmax's first occurrence); every row excluded: -1 and -inf.
 * gallery (N, D) fp32 with row stride ldg >= D (floats), query (Q, D) dense fp32, labels int32.  One launch reads the gallery
 * once for all queries (fp32 MFMA dot tiles); out_cos is bit-identical across launches and across grid sizes (option
 * "zsearch_grid").  workspace: >= mrdis_cosine_top1_workspace(N, D, Q) bytes, 16-byte aligned, used by this entry point ONLY;
 * its first 4 bytes are an arrival counter that must be zero before the first launch (zero the buffer once when allocating
 * it): every launch leaves it zero again.  Launches sharing one workspace must be stream-ordered.
 * Launch counter family "zsearch".                                                                                       */
size_t mrdis_cosine_top1_workspace(int N, int D, int Q);
int mrdis_cosine_top1(const float* gallery, long long ldg, const int* gallery_label, int N, int D,
                      const float* query, const int* query_label, int Q,
                      int* out_idx, float* out_cos, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the `others` variants of the reference (config.yaml:67-70), csrc/mrdis_encs.hip.
 * mod_enc_s: the modality encoder's first layer reads cat([x, s], 1) (model.py:2374) from its two sources: x (N,H,W,Cx) view with
 * pixel stride ldx, s (N,H,W,Cs) view with pixel stride lds.  Filters are those of the concatenated layer: w_tck [T][Cx+Cs][Co],
 * w_tkc [T][Co][Cx+Cs], input channel ci < Cx from x, ci >= Cx from s (T = kh * kw <= 9, Cx + Cs <= 32, Co <= 16, stride <= 2).
 * fp32 FMA.  Forward with optional fused LeakyReLU(0.2); the data gradient writes ds and, unless dx is NULL, dx (dy is the gradient
 * of the pre-activation output); the weight gradient writes dw_tck and, unless dbias is NULL, the bias gradient (added to dbias when
 * accumulate_bias), via per-workgroup slabs in `workspace` (>= the query's bytes, 16-byte aligned) summed in a fixed order.
 * Launch counter family "conv2src".                                                                                     */
int mrdis_conv2d_2src_fwd(const float* x, int ldx, int Cx, const float* s, int lds, int Cs, const float* w_tck, const float* bias,
                          float* y, int ldy, int N, int H, int W, int Co, int kh, int kw, int stride, int pad, int lrelu, void* stream);
int mrdis_conv2d_2src_bwd_data(const float* dy, int lddy, const float* w_tkc, float* dx, int lddx, int Cx, float* ds, int ldds, int Cs,
                               int N, int H, int W, int Co, int kh, int kw, int stride, int pad, void* stream);
size_t mrdis_conv2d_2src_bwd_weight_workspace(int N, int H, int W, int Cx, int Cs, int Co, int kh, int kw, int stride, int pad);
int mrdis_conv2d_2src_bwd_weight(const float* x, int ldx, int Cx, const float* s, int lds, int Cs, const float* dy, int lddy,
                                 float* dw_tck, float* dbias, int accumulate_bias, void* workspace, size_t workspace_bytes,
                                 int N, int H, int W, int Co, int kh, int kw, int stride, int pad, void* stream);
/* ana_dec_act (model.py:3145-3153) on (P, C) views: softplus = F.softplus (beta 1, threshold 20: y = x where x > 20, log1p(exp(x))
 * otherwise; backward dy * e^x / (e^x + 1), dy where x > 20); softmax = F.softmax(s, 1) with no mask channel (C <= 8), backward
 * ds = out * (dout - sum(dout * out)).  Launch counter family "ana_act".                                                 */
int mrdis_softplus_fwd(const float* x, int ldx, float* y, int ldy, long long P, int C, void* stream);
int mrdis_softplus_bwd(const float* dy, int lddy, const float* x, int ldx, float* dx, int lddx, long long P, int C, void* stream);
int mrdis_softmax_fwd(const float* s, int lds, float* out, int ldo, long long P, int C, void* stream);
int mrdis_softmax_bwd(const float* dout, int lddo, const float* out, int ldo, float* ds, int ldds, long long P, int C, void* stream);

/* ---- the latent-code options of the loss block (config.yaml:36, 54, 60-61), csrc/mrdis_latent.hip.
 * Masked KL of the M per-contrast modality codes (M <= MRDIS_KL_MAXM): mu[i], lv[i] (i < M) are HOST arrays of device pointers to (B, Z)
 * fp32 blocks with row strides ldmu / ldlv.  Prior: pmu = plv = NULL for the standard form 0.5 (exp(lv) + mu^2 - 1 - lv) (model.py:3343-3353);
 * otherwise the two-Gaussian form 0.5 (-1 + (plv - lv) + (exp(lv) + (mu - pmu)^2) / exp(plv)) (model.py:3362-3382) with the prior of
 * contrast i, sample b at pmu[i * ldp_m + b * ldp_b + z] (ldp_b = 0: one row per contrast, broadcast over the batch).  weight: (M, B)
 * dense device table (mask and normalisation, computed on the host).  loss = sum_{i,b} weight[i][b] sum_z kl, written to loss[0] by one
 * workgroup in a fixed order.  Backward: the upstream gradient is read from the device scalar dloss; dmu[i], dlv[i] are host arrays of
 * device pointers to (B, Z) outputs with row strides lddmu / lddlv; dpmu / dplv (both NULL, or both given with a prior): dense (M, Z)
 * sums over the batch when ldp_b = 0, dense (M, B, Z) per-sample gradients otherwise.  One launch each way.  Launch counter family "kl".  */
#define MRDIS_KL_MAXM 8
int mrdis_kl_fwd(const float* const* mu, const float* const* lv, int ldmu, int ldlv, const float* pmu, const float* plv, long long ldp_m,
                 int ldp_b, const float* weight, float* loss, int M, int B, int Z, void* stream);
int mrdis_kl_bwd(const float* dloss, const float* const* mu, const float* const* lv, int ldmu, int ldlv, const float* pmu, const float* plv,
                 long long ldp_m, int ldp_b, const float* weight, float* const* dmu, float* const* dlv, int lddmu, int lddlv,
                 float* dpmu, float* dplv, int M, int B, int Z, void* stream);
/* k x k mean pooling, stride k, floor (F.avg_pool2d(x, k), model.py:3453-3456) of an NHWC (N,H,W,C) fp32 view with pixel stride ldx; y is
 * the dense (N, C * (H/k) * (W/k)) compact vector in the NCHW order of the pooled map (view(B, -1)).  Backward: dx = dy / k^2 broadcast
 * over each window, exactly 0 in the rows / columns the floor leaves out; every element of dx (pixel stride lddx) is written.
 * Launch counter family "avgpool".                                                                                        */
int mrdis_avgpool_fwd(const float* x, int ldx, float* y, int N, int H, int W, int C, int k, void* stream);
int mrdis_avgpool_bwd(const float* dy, float* dx, int lddx, int N, int H, int W, int C, int k, void* stream);

/* ---- the attention output decoders 'U+SA+CA' / 'U+SSA+CA' (model.py:1002-1137, 1389-1433), csrc/mrdis_outdec.hip.  fp32 NHWC views with
 * pixel strides (channel slices allowed); float4 forms when every pointer is 16-byte aligned and every stride and C are multiples of 4.
 * Channel attention + the decoder level's skip sum: a = sigmoid(W_up relu(W_down mean_hw(x) + b_down) + b_up), out = (1 + a[b, c]) x + s.
 * x, s, out: (B, HW, C) views (out: typically channels [0, C) of the level's concatenation buffer); wd (Hd, C), bd (Hd), wu (C, Hd), bu (C):
 * the nn.Linear parameters, dense.  Writes pool (B, C), hid (B, Hd, after the ReLU) and a (B, C), dense: what the backward reads.  Three
 * launches (partial sums over fixed pixel chunks, the mean and the MLP for all rows, the combine).  Backward: dx = (1 + a) dy + dpool / HW
 * with the MLP backward in between; the weight and bias gradients are WRITTEN (sums over the batch in a fixed order); the gradient of s
 * is dy itself.  Workspace: mrdis_chatt_workspace bytes, for either direction.  Launch counter family "chatt" (one count per call). */
size_t mrdis_chatt_workspace(int B, long long HW, int C, int Hd);
int mrdis_chatt_fwd(const float* x, int ldx, const float* s, int lds, const float* wd, const float* bd, const float* wu, const float* bu,
                    float* out, int ldo, float* pool, float* hid, float* a, void* ws, size_t ws_bytes, int B, long long HW, int C, int Hd,
                    void* stream);
int mrdis_chatt_bwd(const float* dy, int lddy, const float* x, int ldx, const float* a, const float* hid, const float* pool,
                    const float* wd, const float* wu, float* dx, int lddx, float* dwd, float* dbd, float* dwu, float* dbu,
                    void* ws, size_t ws_bytes, int B, long long HW, int C, int Hd, void* stream);
/* gd = |g - flip_H(g)| of a (B, H, W, C) view; backward dg[h] = sgn(g[h] - g[H-1-h]) (dgd[h] + dgd[H-1-h]), sgn(0) = 0.  Family "symdiff". */
int mrdis_symdiff_fwd(const float* g, int ldg, float* gd, int ldo, int B, int H, int W, int C, void* stream);
int mrdis_symdiff_bwd(const float* dgd, int lddgd, const float* g, int ldg, float* dg, int lddg, int B, int H, int W, int C, void* stream);
/* out = (1 + up2(alpha)) x: x (B, H, W, C) with H, W even, alpha a dense (B, H/2, W/2) map, up2 the x2 bilinear resize with align_corners=False.
 * Backward: dx = (1 + up2(alpha)) dy and rsum (B, H, W) dense = sum_c dy x (dalpha = the bilinear backward of rsum).  Family "rgate". */
int mrdis_rgate_fwd(const float* x, int ldx, const float* alpha, float* out, int ldo, int B, int H, int W, int C, void* stream);
int mrdis_rgate_bwd(const float* dy, int lddy, const float* x, int ldx, const float* alpha, float* dx, int lddx, float* rsum,
                    int B, int H, int W, int C, void* stream);

/* ---- preprocessing of raw scans into store volumes (data_preprocessing_BraTS.py:79-96, commented out there; the same rule is live in
 * data_preprocessing_ZeroDose.py:124-134), csrc/mrdis_prep.hip.  raw: the voxel array of a NIfTI-1 file in its own dtype (the NIfTI datatype
 * codes below), voxel (h, w, d) at raw[h stride_h + w stride_w + d stride_d] (element strides >= 1; the file's own order is stride_h = 1,
 * stride_w = H, stride_d = H W, and it is the fast path; any other triple is only correct).  v = (double)raw * slope + inter in float64, NaN -> 0.
 * The crop removes h0 / h1 voxels at the low / high end of H and w0 / w1 of W; the depth is kept whole: H' = H - h0 - h1, W' = W - w0 - w1.
 * Each of H, W, D in 1 .. 1024, H W D < 2^31, H' >= 1, W' >= 1; anything else: MRDIS_EUNSUPPORTED before any launch.
 * mrdis_prep_stats: stats (5 float64, device) = { n = #(v > 0), sum = sum v, ssd = sum_{v > 0} (v - sum / (n + 1))^2 } over the cropped volume,
 * { vmax = max v with NaN ignored, nan_inner = #NaN with d in [d_lo, D - d_hi) } over the uncropped one.  Four launches (partial sums and
 * their fixed-order sum, twice: ssd needs n and sum), no atomics: two runs give the same bits.  workspace: >= mrdis_prep_workspace bytes
 * (0 for an unsupported geometry), 8-byte aligned, used by this call only.
 * mrdis_prep_write: reads stats from the device (no host synchronisation in between) and writes fp32, rounded once at the store, as
 * (D, H', W') (MRDIS_PREP_DHW) or (H', W', D) (MRDIS_PREP_HWD), dense.  MRDIS_PREP_ZSCORE: (v - norm) / (std + 1e-8) with norm = sum / (n + 1),
 * std = sqrt(ssd / (n + 1)), and -10 where v <= 0; MRDIS_PREP_MEAN: v / norm; MRDIS_PREP_LABEL: v (stats is not read).  One launch.
 * Launch counter families "prepstats" / "prepwrite": one count per call.                                                                   */
#define MRDIS_PREP_U8 2
#define MRDIS_PREP_I16 4
#define MRDIS_PREP_I32 8
#define MRDIS_PREP_F32 16
#define MRDIS_PREP_F64 64
#define MRDIS_PREP_U16 512
#define MRDIS_PREP_ZSCORE 0
#define MRDIS_PREP_MEAN 1
#define MRDIS_PREP_LABEL 2
#define MRDIS_PREP_DHW 0
#define MRDIS_PREP_HWD 1
size_t mrdis_prep_workspace(int H, int W, int D);
int mrdis_prep_stats(const void* raw, int dtype, long long stride_h, long long stride_w, long long stride_d, int H, int W, int D,
                     int h0, int h1, int w0, int w1, int d_lo, int d_hi, double slope, double inter, double* stats,
                     void* workspace, size_t workspace_bytes, void* stream);
int mrdis_prep_write(const void* raw, int dtype, long long stride_h, long long stride_w, long long stride_d, int H, int W, int D,
                     int h0, int h1, int w0, int w1, double slope, double inter, const double* stats, int kind, int layout,
                     float* out, void* stream);

/* ---- the inverse of mrdis_prep_write: store volumes back to the order and canvas of a NIfTI file, csrc/mrdis_export.hip.  src: B volumes of one
 * geometry, dense and back to back, uint8 (MRDIS_PREP_U8) or fp32 (MRDIS_PREP_F32), each (H', W', D) (MRDIS_PREP_HWD: a VolumeStore3D, label and
 * synthesized volumes) or (D, H', W') (MRDIS_PREP_DHW: a VolumeStore).  dst: (B, D, W, H) dense, h fastest -- the order of the file --, on the full
 * canvas H = H' + h0 + h1, W = W' + w0 + w1; uint8, int16 (MRDIS_PREP_I16) or fp32, aligned to its element only (no 4-byte promise for the narrow types).
 * Per output voxel (b, d, w, h): outside [h0, H - h1) x [w0, W - w1) y = fill; inside, with s = src[b](h - h0, w - w0, d),
 *   MRDIS_EXPORT_COPY      y = s
 *   MRDIS_EXPORT_UNZSCORE  y = 0 where s == -10.0f exactly, else (double)s * (std + 1e-8) + norm, multiply and add rounded separately in float64
 *   MRDIS_EXPORT_UNMEAN    y = (double)s * norm
 * with norm = sum / (n + 1), std = sqrt(ssd / (n + 1)) read on the device from stats + 5 b: B x 5 float64 in the layout mrdis_prep_stats writes (no
 * host read).  Conversion: fp32 by one rounding of y; int16 / uint8 by NaN -> 0, round to nearest with ties to even, clamp to the type's range
 * (+-inf saturate).  A uint8 source takes COPY only (uint8 -> uint8 is a byte copy).  stats may be NULL for COPY.
 * One launch whatever B, on the caller's stream, no atomics: two runs give the same bits.  Launch counter family "export": one count per call.
 * MRDIS_EUNSUPPORTED before any launch: H', W', D, H or W outside 1 .. 1024, H W D >= 2^31, B outside 1 .. 65535, a negative crop, an unknown dtype,
 * layout or kind code, a uint8 source with another kind than COPY, stats NULL with a kind that reads it.  MRDIS_EINVAL: src or dst NULL.
 * MRDIS_EALIGN: src / dst not aligned to their element, stats not to 8 bytes.                                                                    */
#define MRDIS_EXPORT_COPY 0
#define MRDIS_EXPORT_UNZSCORE 1
#define MRDIS_EXPORT_UNMEAN 2
int mrdis_export_volume(const void* src, int src_dtype, int layout, int Hc, int Wc, int D, int h0, int h1, int w0, int w1, int B,
                        int kind, const double* stats, double fill, void* dst, int dst_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRDIS_H */
