// mrdis_launchers.h -- every kernel launcher and workspace query that one translation unit defines and another calls, declared once.
// mrdis_common.h includes this file, so the defining file sees the declaration too: a parameter list that drifts from it fails the link
// (-Wl,--no-undefined), not the dlopen.  Default arguments live here and nowhere else.  Launchers that take a parameter struct sit beside
// the struct instead (mrdis_tapconv.h, mrdis_s6conv.h, mrdis_conv3d.h).  MRDIS_EUNSUPPORTED from a launcher means "outside what this
// kernel covers": the caller runs the next form; a workspace query answers 0 for the same layers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// ---- mrdis_wino.hip ----
// fused Winograd F(2x2, 3x3) kernel; MRDIS_EUNSUPPORTED: the caller falls back to the direct kernel
int mrdis_run_wino(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy,
                   int N, int H, int W, int Ci, int Co, int flip, int lrelu, hipStream_t s);
// hybrid 3-D path: F(2x2, 3x3) in (h, w), direct in depth; x (N, D, H, W, Ci) -> y (N, D, H, W, Co), 27-tap filter [27][Ci][Co]
int mrdis_run_wino3d(const float* x, int ldx, const float* w, const float* bias, const float* res, int ldres, float* y, int ldy,
                     int N, int D, int H, int W, int Ci, int Co, int flip, hipStream_t s);
// Winograd weight gradient: 3x3 s1 p1 layers with Ci, Co multiples of 32 / 64 and enough tiles per split; workspace 0 / MRDIS_EUNSUPPORTED elsewhere
size_t mrdis_wino_wgrad_workspace(int N, int H, int W, int Ci, int Co);
int mrdis_run_wino_wgrad(const float* x, int ldx, const float* dy, int lddy, float* dw_tck, float* dbias, void* workspace,
                         size_t workspace_bytes, int N, int H, int W, int Ci, int Co, int accumulate_bias, hipStream_t s);
// hybrid 3-D weight gradient: dw_tck [27][Ci][Co], three launches of the 2-D kernel (one per depth tap)
size_t mrdis_wino_wgrad3d_workspace(int N, int D, int H, int W, int Ci, int Co);
int mrdis_run_wino_wgrad3d(const float* x, int ldx, const float* dy, int lddy, float* dw_tck, float* dbias, void* workspace,
                           size_t workspace_bytes, int N, int D, int H, int W, int Ci, int Co, hipStream_t s);

// ---- mrdis_wino2.hip ----
// software-pipelined F(2x2, 3x3) variant for Cout > 32; MRDIS_EUNSUPPORTED: the caller takes mrdis_run_wino
int mrdis_run_wino2(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy,
                    int N, int H, int W, int Ci, int Co, int flip, int lrelu, hipStream_t s, const float* u_img);
// its SPADE-fused form: gamma | beta convolution + InstanceNorm modulation in one launch; MRDIS_EUNSUPPORTED: the caller runs the two-step path
int mrdis_run_wino2_spade(const float* x, int ldx, const float* w, const float* bias, const float* z, int ldz, const float* mean, const float* rstd,
                          float* mix, int ldmix, float* gamma, int ldg, int N, int H, int W, int Ci, int C, hipStream_t s, const float* u_img);

// ---- mrdis_wino4.hip ----
// F(4x4, 3x3): takes the layers whose filter image is of format 4 (mrdis_wino_u_format; the image carries the flip, so forward and
// data gradient are the same call); MRDIS_EUNSUPPORTED where its shape limits / grid test decline
int mrdis_run_wino4(const float* x, int ldx, const float* bias, float* y, int ldy, int N, int H, int W, int Ci, int Co, int lrelu,
                    hipStream_t s, const float* u_img);
// the narrow form of the same kernel (image format 5, <= 32 couts); MRDIS_EUNSUPPORTED: the caller takes the F(2x2) kernel
int mrdis_run_wino4n(const float* x, int ldx, const float* bias, float* y, int ldy, int N, int H, int W, int Ci, int Co, int lrelu,
                     hipStream_t s, const float* u_img);
// SPADE-fused form on a format-4 image of the fused gamma | beta filter; MRDIS_EUNSUPPORTED: the caller takes the F(2x2) form / the two-step path
int mrdis_run_wino4_spade(const float* x, int ldx, const float* bias, const float* z, int ldz, const float* mean, const float* rstd,
                          float* mix, int ldmix, float* gamma, int ldg, int N, int H, int W, int Ci, int C, hipStream_t s, const float* u_img);

// ---- mrdis_wino4r.hip ----
// the register-fed form of the <= 32-cout F(4x4) layers (option wino4r); MRDIS_EUNSUPPORTED: the caller takes mrdis_run_wino4n
int mrdis_run_wino4r(const float* x, int ldx, const float* bias, float* y, int ldy, int N, int H, int W, int Ci, int Co, int lrelu,
                     hipStream_t s, const float* u_img);

// ---- mrdis_bf16.hip ----
// weight gradient on bf16 MFMA operands (stride-1 "same" convolutions, Ci % 32 == 0); workspace 0 / MRDIS_EUNSUPPORTED elsewhere
size_t mrdis_bwgrad_workspace(int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad);
int mrdis_run_bwgrad(const void* x, int ldx, const void* dy, int lddy, float* dw_tck, float* dbias, void* workspace, size_t workspace_bytes,
                     int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int accumulate_bias, int dtype, hipStream_t s);

// ---- mrdis_bf16p.hip ----
// SPADE-fused form of the pipelined bf16 kernel on bf16 activations; MRDIS_EUNSUPPORTED: the caller runs the two-step path
int mrdis_run_bconv3_spade(const void* x, int ldx, const void* w_bf16, const float* bias, const void* z, int ldz, const float* mean, const float* rstd,
                           void* mix, int ldmix, void* gamma, int ldg, int N, int H, int W, int Ci, int C, hipStream_t s);

// ---- mrdis_bf16q.hip ----
// the same contract on the LDS-DMA kernel; MRDIS_EUNSUPPORTED: the caller takes mrdis_run_bconv3_spade
int mrdis_run_bconv4_spade(const void* x, int ldx, const void* w_bf16, const float* bias, const void* z, int ldz, const float* mean, const float* rstd,
                           void* mix, int ldmix, void* gamma, int ldg, int N, int H, int W, int Ci, int C, hipStream_t s);

// ---- mrdis_pointwise.hip ----
// the 1x1 decoder head (16 -> <= 8 channels) as streaming kernels; each returns MRDIS_EUNSUPPORTED (workspace: 0) outside what it covers
// (16 channels on the wide side -- fp32 or bf16 views --, <= 8 fp32 channels on the narrow one)
int mrdis_run_pw_fwd(const void* x, int ldx, const float* w_tck, const float* bias, float* y, int ldy, long long npix, int Ci, int Co, int lrelu, int x16_bf16, hipStream_t s);
int mrdis_run_pw_dgrad(const float* dy, int lddy, const float* w_tkc, void* dx, int lddx, long long npix, int Ci, int Co, int x16_bf16, hipStream_t s);
size_t mrdis_pw_wgrad_workspace(long long npix, int Ci, int Co, int x16_bf16);
int mrdis_run_pw_wgrad(const void* x, int ldx, const float* dy, int lddy, float* dw_tck, float* dbias, void* workspace, size_t workspace_bytes,
                       long long npix, int Ci, int Co, int accumulate_bias, int x16_bf16, hipStream_t s);

// ---- mrdis_wgrad_s2.hip ----
// dw[i] = sum_k slab[k * total + i], dbias[co] (+)= sum_k bslab[k * Co + co], fixed order: the slab reduction shared with mrdis_pointwise.hip
int mrdis_launch_slab_reduce(const float* slab, float* dw, int total, int Co, int nslab, const float* bslab, float* dbias, int accumulate_bias,
                             hipStream_t s);
// the stride-2 first layers (Cin <= 7): forward, data gradient (dy (N, H/2, W/2, Co) -> dx (N, H, W, Ci)) and weight gradient;
// MRDIS_EUNSUPPORTED (workspace: 0) outside what the kernels cover
int mrdis_run_conv_s2_fwd(const float* x, int ldx, const float* w_tck, const float* bias, float* y, int ldy, int N, int H, int W, int Ci, int Co,
                          int kh, int kw, int stride, int pad, int lrelu, hipStream_t s);
int mrdis_run_dgrad_s2(const float* dy, int lddy, const float* w_tkc, float* dx, int lddx, int N, int H, int W, int Ci, int Co,
                       int kh, int kw, int stride, int pad, hipStream_t s);
size_t mrdis_wgrad_s2_workspace(int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad);
int mrdis_run_wgrad_s2(const float* x, int ldx, const float* dy, int lddy, float* dw_tck, float* dbias, void* workspace, size_t workspace_bytes,
                       int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int accumulate_bias, hipStream_t s);
// weight gradient of the 4 -> C si_layers (3x3 s1 p1); MRDIS_EUNSUPPORTED (workspace: 0) outside what the kernel covers
size_t mrdis_wgrad_c4_workspace(int N, int H, int W, int Ci, int Co);
int mrdis_run_wgrad_c4(const float* x, int ldx, const void* dy, int lddy, float* dw_tck, float* dbias, void* workspace, size_t workspace_bytes,
                       int N, int H, int W, int Ci, int Co, int accumulate_bias, int dy_bf16, hipStream_t s, int pad16 = 0);
// weight gradient of the C -> 4 layers on a bf16 input; MRDIS_EUNSUPPORTED (workspace: 0) outside what the kernel covers
size_t mrdis_wgrad_co4b_workspace(int N, int H, int W, int Ci, int Co);
int mrdis_run_wgrad_co4b(const void* x_bf16, int ldx, const float* dy, int lddy, float* dw_tck, float* dbias, void* workspace, size_t workspace_bytes,
                         int N, int H, int W, int Ci, int Co, int accumulate_bias, hipStream_t s, int pad16);

// ---- mrdis_wgrad16.hip ----
// weight gradient for Cout <= 16, 3x3 s1 p1; MRDIS_EUNSUPPORTED (workspace: 0) when the layer is outside what the kernel covers
size_t mrdis_wgrad16_workspace(int N, int H, int W, int Ci, int Co);
int mrdis_run_wgrad16(const float* x, int ldx, const float* dy, int lddy, float* dw_tck, float* dbias, void* workspace,
                      size_t workspace_bytes, int N, int H, int W, int Ci, int Co, int accumulate_bias, hipStream_t s);
// bf16 views, 32 -> 16, large maps; MRDIS_EUNSUPPORTED elsewhere (the caller runs the generic bf16 kernel)
int mrdis_run_wgrad16_bf16(const void* x, int ldx, const void* dy, int lddy, float* dw_tck, float* dbias, void* workspace, size_t workspace_bytes,
                           int N, int H, int W, int Ci, int Co, int accumulate_bias, hipStream_t s);

// ---- mrdis_co4.hip ----
// 3x3 s1 p1 with 4 output channels: window-free GEMM + tap gather; MRDIS_EUNSUPPORTED outside what the kernel covers
int mrdis_run_co4(const void* x, int ldx, const float* w, const float* bias, float* y, int ldy, int N, int H, int W, int Ci, int Co, int flip, int lrelu, hipStream_t s,
                  int x_bf16 = 0, int wld = 4);

// ---- mrdis_c16.hip ----
// 3x3 s1 p1 with 16 output channels, filter in registers; MRDIS_EUNSUPPORTED: the caller runs the generic narrow-output kernel
int mrdis_run_c16(const float* x, int ldx, const float* w_tck, const float* bias, float* y, int ldy, int N, int H, int W, int Ci, int Co, int lrelu, hipStream_t s);
// 16 -> 32 on six bf16 products, as a data gradient (taps reversed) or a forward (flip = 0); MRDIS_EUNSUPPORTED outside what the kernel covers
int mrdis_run_c16t_split6(const float* x, int ldx, const float* w_t_ci_co, float* y, int ldy, int N, int H, int W, int flip, hipStream_t s);
