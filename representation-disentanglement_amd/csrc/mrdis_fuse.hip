// Fusion of the anatomy maps over the contrasts a sample HAS (MultimodalModel.reconstruct_output_fused, lambda_recon_y_fused): the input of the
// output decoder when contrasts are missing.  The rule is this package's own convention -- the reference's `si_cat[mask == 1]`
// (model.py:3239-3258) flattens batch and contrast into rows and reduces a singleton axis, so it never fuses and fails for M > 1:
//   for sample b, over the contrasts k with mask[b, k] == 1 (n_b of them), per pixel and channel
//     mean   the sum in increasing k, divided by (float)n_b (IEEE fp32 division)
//     max    the largest, min the smallest value
//     mean-max-min   the channel concatenation [mean | max | min] (3 C channels, the reference's order)
//   With one map (K = 1) every method is the identity.  A row without any present contrast is refused by the caller from its HOST mask
//   (ops.fuse_present); the kernels themselves write zeros for such a row, forward and backward.
//   mrdis_fuse_present_fwd   one pass, every output element written exactly once
//   mrdis_fuse_present_bwd   reads dout and the K maps again (the arg is recomputed: no index tensor is saved) and writes all K gradients, every
//                            element once: zeros for an absent contrast; mean: g / (float)n_b for every present k; max / min: g for the LOWEST
//                            present index that attains the extremum and 0 for the others (ties are common: the background pixels of the softmax
//                            maps are 0 in every contrast; torch leaves the choice on ties unspecified); mean-max-min: the three contributions
//                            added in the order mean, max, min.
// n_b and the present set come from the (B, K) mask ON THE DEVICE: nothing that varies per step is baked into the launch, so a recorded step
// replays for any mask.  A workgroup works on one sample (blockIdx.y), so the mask row, the present set and the skipped loads of an absent
// contrast are wave-uniform.
//
// fp32 NHWC views with pixel strides; float4 forms when every pointer and stride allows them, scalar forms otherwise.  No float atomics, no
// memset / memcpy / host synchronisation (graph capture).  Launch counter family "fuse": one count per _fwd / _bwd call.
#include "mrdis_common.h"

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_MAXK = MRDIS_FUSE_MAX_SRC;

struct FuseSrc { const float* p[FU_MAXK]; int ld[FU_MAXK]; };
struct FuseDst { float* p[FU_MAXK]; int ld[FU_MAXK]; };

// x dimension of a (gx, B) grid over the per-image work items: about 4096 workgroups in all, grid-strided beyond that
inline int fu_image_grid(long long per_image, int B) {
    long long cap = 4096 / B; if (cap < 1) cap = 1;
    long long b = (per_image + FU_THREADS - 1) / FU_THREADS; if (b > cap) b = cap; if (b < 1) b = 1;
    return (int)b;
}

template <int V> __device__ __forceinline__ void ld_arr(const float* p, float (&a)[V]) {
    if constexpr (V == 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(p); a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
    else a[0] = *p;
}
template <int V> __device__ __forceinline__ void st_arr(float* p, const float (&a)[V]) {
    if constexpr (V == 4) { f32x4 v; v.x = a[0]; v.y = a[1]; v.z = a[2]; v.w = a[3]; *reinterpret_cast<f32x4*>(p) = v; }
    else *p = a[0];
}

// bit k: mask[b, k] == 1 (wave-uniform: b is the workgroup's sample)
__device__ __forceinline__ unsigned fu_present(const float* __restrict__ mask, int b, int K) {
    unsigned pres = 0;
#pragma unroll
    for (int k = 0; k < FU_MAXK; ++k)
        if (k < K && mask[(long long)b * K + k] == 1.f) pres |= 1u << k;
    return pres;
}

// METHOD 0 mean | 1 max | 2 mean-max-min
template <int V, int METHOD>
__global__ __launch_bounds__(FU_THREADS) void fuse_fwd_kernel(FuseSrc src, int K, const float* __restrict__ mask, float* __restrict__ out, int ldo,
                                                              long long HW, int C) {
    const int CV = C / V;
    const long long total = HW * CV;                 // per image (blockIdx.y)
    const int b = blockIdx.y;
    const unsigned pres = fu_present(mask, b, K);
    const float fn = (float)__popc(pres);
    for (long long e = blockIdx.x * (long long)FU_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * FU_THREADS) {
        const long long pix = (long long)b * HW + e / CV;
        const int c = (int)(e % CV) * V;
        float sum[V], mx[V], mn[V];
#pragma unroll
        for (int v = 0; v < V; ++v) sum[v] = mx[v] = mn[v] = 0.f;
        bool first = true;
#pragma unroll
        for (int k = 0; k < FU_MAXK; ++k) {
            if ((pres >> k) & 1u) {                                  // wave-uniform
                float x[V];
                ld_arr<V>(src.p[k] + pix * src.ld[k] + c, x);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if (first) { sum[v] = x[v]; mx[v] = x[v]; mn[v] = x[v]; }
                    else { sum[v] += x[v]; mx[v] = x[v] > mx[v] ? x[v] : mx[v]; mn[v] = x[v] < mn[v] ? x[v] : mn[v]; }
                }
                first = false;
            }
        }
        float* o = out + pix * ldo + c;
        if (METHOD != 1) {
            float m[V];
#pragma unroll
            for (int v = 0; v < V; ++v) m[v] = pres ? sum[v] / fn : 0.f;
            st_arr<V>(o, m);
        }
        if (METHOD == 1) st_arr<V>(o, mx);
        if (METHOD == 2) { st_arr<V>(o + C, mx); st_arr<V>(o + 2 * C, mn); }
    }
}

template <int V, int METHOD>
__global__ __launch_bounds__(FU_THREADS) void fuse_bwd_kernel(FuseSrc src, int K, const float* __restrict__ mask, const float* __restrict__ dout,
                                                              int lddo, FuseDst dst, long long HW, int C) {
    const int CV = C / V;
    const long long total = HW * CV;
    const int b = blockIdx.y;
    const unsigned pres = fu_present(mask, b, K);
    const float fn = (float)__popc(pres);
    for (long long e = blockIdx.x * (long long)FU_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * FU_THREADS) {
        const long long pix = (long long)b * HW + e / CV;
        const int c = (int)(e % CV) * V;
        const float* g = dout + pix * lddo + c;
        float gm[V], gx[V], gn[V];                   // gradients of the mean, max and min outputs
        int ax[V], an[V];                            // lowest present index attaining the max / the min
#pragma unroll
        for (int v = 0; v < V; ++v) { gm[v] = gx[v] = gn[v] = 0.f; ax[v] = an[v] = -1; }
        if (METHOD == 0) ld_arr<V>(g, gm);
        if (METHOD == 1) ld_arr<V>(g, gx);
        if (METHOD == 2) { ld_arr<V>(g, gm); ld_arr<V>(g + C, gx); ld_arr<V>(g + 2 * C, gn); }
        if (METHOD != 0) {
            float mx[V], mn[V];
#pragma unroll
            for (int v = 0; v < V; ++v) mx[v] = mn[v] = 0.f;
#pragma unroll
            for (int k = 0; k < FU_MAXK; ++k) {
                if ((pres >> k) & 1u) {
                    float x[V];
                    ld_arr<V>(src.p[k] + pix * src.ld[k] + c, x);
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        if (ax[v] < 0 || x[v] > mx[v]) { mx[v] = x[v]; ax[v] = k; }      // strict: a tie stays with the lower index
                        if (an[v] < 0 || x[v] < mn[v]) { mn[v] = x[v]; an[v] = k; }
                    }
                }
            }
        }
        if (METHOD != 1) {
#pragma unroll
            for (int v = 0; v < V; ++v) gm[v] = gm[v] / fn;          // (no present contrast: unused)
        }
#pragma unroll
        for (int k = 0; k < FU_MAXK; ++k) {
            if (k < K) {
                float d[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    float t = 0.f;
                    if ((pres >> k) & 1u) {
                        if (METHOD == 0) t = gm[v];
                        if (METHOD == 1) t = ax[v] == k ? gx[v] : 0.f;
                        if (METHOD == 2) {
                            t = gm[v];
                            if (ax[v] == k) t += gx[v];
                            if (an[v] == k) t += gn[v];
                        }
                    }
                    d[v] = t;
                }
                st_arr<V>(dst.p[k] + pix * dst.ld[k] + c, d);
            }
        }
    }
}

bool fu_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool fu_al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

template <int V, int METHOD>
void fu_launch_fwd(dim3 grid, hipStream_t st, const FuseSrc& s, int K, const float* mask, float* out, int ldo, long long HW, int C) {
    MRDIS_LAUNCH((fuse_fwd_kernel<V, METHOD>), grid, dim3(FU_THREADS), 0, st, s, K, mask, out, ldo, HW, C);
}
template <int V, int METHOD>
void fu_launch_bwd(dim3 grid, hipStream_t st, const FuseSrc& s, int K, const float* mask, const float* dout, int lddo, const FuseDst& d,
                   long long HW, int C) {
    MRDIS_LAUNCH((fuse_bwd_kernel<V, METHOD>), grid, dim3(FU_THREADS), 0, st, s, K, mask, dout, lddo, d, HW, C);
}

// the checks both directions share; fills the by-value source table (entries K .. 7 repeat entry 0 and are never read)
int fu_check(const float* const* srcs, const int* ld_srcs, int K, const float* mask, int method, int B, long long HW, int C, FuseSrc& s, bool& vec) {
    if (!srcs || !ld_srcs || !mask || K < 1 || K > FU_MAXK || method < 0 || method > 2 || B < 1 || HW < 1 || C < 1) return MRDIS_EINVAL;
    if (B > 65535 || HW >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    if (!fu_al4(mask)) return MRDIS_EALIGN;
    vec = (C % 4) == 0;
    for (int k = 0; k < FU_MAXK; ++k) {
        const int j = k < K ? k : 0;
        s.p[k] = srcs[j]; s.ld[k] = ld_srcs[j];
        if (!s.p[k] || s.ld[k] < C) return MRDIS_EINVAL;
        if (!fu_al4(s.p[k])) return MRDIS_EALIGN;
        vec = vec && fu_al16(s.p[k]) && (s.ld[k] % 4) == 0;
    }
    return MRDIS_OK;
}

}  // namespace

extern "C" int mrdis_fuse_present_fwd(const float* const* srcs, const int* ld_srcs, int K, const float* mask, int method, float* out, int ldo,
                                      int B, long long HW, int C, void* stream) {
    FuseSrc s;
    bool vec = false;
    const int rc = fu_check(srcs, ld_srcs, K, mask, method, B, HW, C, s, vec);
    if (rc != MRDIS_OK) return rc;
    const int F = method == 2 ? 3 : 1;
    if (!out || ldo < F * C) return MRDIS_EINVAL;
    if (!fu_al4(out)) return MRDIS_EALIGN;
    vec = vec && fu_al16(out) && (ldo % 4) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(fu_image_grid(HW * (C / (vec ? 4 : 1)), B), B);
    mrdis_count(MRDIS_CNT_FUSE);
    if (vec) {
        if (method == 0) fu_launch_fwd<4, 0>(grid, st, s, K, mask, out, ldo, HW, C);
        else if (method == 1) fu_launch_fwd<4, 1>(grid, st, s, K, mask, out, ldo, HW, C);
        else fu_launch_fwd<4, 2>(grid, st, s, K, mask, out, ldo, HW, C);
    } else {
        if (method == 0) fu_launch_fwd<1, 0>(grid, st, s, K, mask, out, ldo, HW, C);
        else if (method == 1) fu_launch_fwd<1, 1>(grid, st, s, K, mask, out, ldo, HW, C);
        else fu_launch_fwd<1, 2>(grid, st, s, K, mask, out, ldo, HW, C);
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_fuse_present_bwd(const float* dout, int lddo, const float* const* srcs, const int* ld_srcs, int K, const float* mask, int method,
                                      float* const* dsrcs, const int* ld_dsrcs, int B, long long HW, int C, void* stream) {
    FuseSrc s;
    bool vec = false;
    const int rc = fu_check(srcs, ld_srcs, K, mask, method, B, HW, C, s, vec);
    if (rc != MRDIS_OK) return rc;
    const int F = method == 2 ? 3 : 1;
    if (!dout || lddo < F * C || !dsrcs || !ld_dsrcs) return MRDIS_EINVAL;
    if (!fu_al4(dout)) return MRDIS_EALIGN;
    vec = vec && fu_al16(dout) && (lddo % 4) == 0;
    FuseDst d;
    for (int k = 0; k < FU_MAXK; ++k) {
        const int j = k < K ? k : 0;
        d.p[k] = dsrcs[j]; d.ld[k] = ld_dsrcs[j];
        if (!d.p[k] || d.ld[k] < C) return MRDIS_EINVAL;
        if (!fu_al4(d.p[k])) return MRDIS_EALIGN;
        vec = vec && fu_al16(d.p[k]) && (d.ld[k] % 4) == 0;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(fu_image_grid(HW * (C / (vec ? 4 : 1)), B), B);
    mrdis_count(MRDIS_CNT_FUSE);
    if (vec) {
        if (method == 0) fu_launch_bwd<4, 0>(grid, st, s, K, mask, dout, lddo, d, HW, C);
        else if (method == 1) fu_launch_bwd<4, 1>(grid, st, s, K, mask, dout, lddo, d, HW, C);
        else fu_launch_bwd<4, 2>(grid, st, s, K, mask, dout, lddo, d, HW, C);
    } else {
        if (method == 0) fu_launch_bwd<1, 0>(grid, st, s, K, mask, dout, lddo, d, HW, C);
        else if (method == 1) fu_launch_bwd<1, 1>(grid, st, s, K, mask, dout, lddo, d, HW, C);
        else fu_launch_bwd<1, 2>(grid, st, s, K, mask, dout, lddo, d, HW, C);
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
