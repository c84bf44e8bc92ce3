// Kernels of the reference's attention output decoders 'U+SA+CA' and 'U+SSA+CA' (model.py:1002-1137, 1389-1433):
//
//  * channel attention (ChannelAttentionLayer, squeeze and excitation, :1417-1433) fused with the skip sum of the decoder level:
//      a = sigmoid(W_up relu(W_down mean_hw(x) + b_down) + b_up)      (B, C), hidden width Hd = C / r
//      skip = (1 + a[b, c]) * x + s                                     s: the spatial branch's output
//    Forward: (a) partial per-(b, c) sums of x over fixed pixel chunks, (b) one small launch that finishes the mean in a fixed order and
//    runs the MLP for all B rows, (c) the combine, written straight into the caller's output view (a channel slice of the decoder level's
//    concatenation buffer).  Backward: (a) partial sums of dy * x, (b) one workgroup for the MLP backward (weight / bias gradients summed
//    over the batch in order, dpool), (c) dx = (1 + a) dy + dpool / HW.  The gradient of s is dy itself (no kernel).
//  * symmetric difference (SymmetryGateResidualSpatialAttentionLayer, :1405-1406): gd = |g - flip_H(g)|, and its adjoint
//      dg[h] = sgn(g[h] - g[H-1-h]) * (dgd[h] + dgd[H-1-h])      sgn(0) = 0 (torch's abs backward): the middle row of an odd H gets 0
//  * residual gate (:1409-1412): out = (1 + up2(alpha)) * x, alpha (B, 1, H/2, W/2) dense, up2 = bilinear x2 with align_corners=False
//    interpolated on the fly.  Backward: dx = (1 + up2(alpha)) dy and r = sum_c dy * x per pixel (dalpha = up2^T r: the existing
//    bilinear backward on the 1-channel r).
//
// fp32 NHWC views with pixel strides; float4 forms when every pointer and stride allows them, scalar forms otherwise.  Fixed-order
// reductions, no float atomics, no memset / memcpy / host synchronisation (graph capture).  Launch counter families "chatt",
// "symdiff", "rgate".
#include "mrdis_common.h"

namespace {

constexpr int OD_THREADS = 256;
constexpr int OD_MLP_BWD_THREADS = 1024;

inline int od_grid(long long n, int threads) { long long b = (n + threads - 1) / threads; if (b > 8192) b = 8192; if (b < 1) b = 1; return (int)b; }
// x dimension of a (gx, B) grid over per-image work items: about 4096 workgroups in all, grid-strided beyond that
inline int od_image_grid(long long per_image, int B) {
    long long cap = 4096 / B; if (cap < 1) cap = 1;
    long long b = (per_image + OD_THREADS - 1) / OD_THREADS; if (b > cap) b = cap; if (b < 1) b = 1;
    return (int)b;
}

template <int V> struct vec;
template <> struct vec<1> { typedef float t; };
template <> struct vec<4> { typedef f32x4 t; };

template <int V> __device__ __forceinline__ typename vec<V>::t ldv(const float* p) { return *reinterpret_cast<const typename vec<V>::t*>(p); }
template <int V> __device__ __forceinline__ void stv(float* p, typename vec<V>::t v) { *reinterpret_cast<typename vec<V>::t*>(p) = v; }
__device__ __forceinline__ float hsum(float v) { return v; }
__device__ __forceinline__ float hsum(f32x4 v) { return ((v.x + v.y) + v.z) + v.w; }

// ---------------------------------------------------------------- channel attention
// Partial sums over a fixed pixel chunk of one image: block (b * P + p, cg) sums pixels [p * chunk, (p + 1) * chunk) of image b for the
// channel vectors [cg * 256, cg * 256 + 256) (V channels each).  PROD: the summand is x * y.  part[(b * P + p) * C + c], every element
// written once.  The npl pixel lanes of one channel vector meet in LDS in lane order.
template <int V, bool PROD>
__global__ __launch_bounds__(OD_THREADS) void chatt_partial_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ y, int ldy,
                                                                   float* __restrict__ part, int HW, int C, int P, int chunk) {
    __shared__ float red[OD_THREADS * V];
    const int CV = C / V;
    const int cv0 = blockIdx.y * OD_THREADS;
    const int CVb = min(OD_THREADS, CV - cv0);
    const int npl = OD_THREADS / CVb;
    const int t = threadIdx.x;
    const int cvl = t % CVb, pl = t / CVb;
    const int b = blockIdx.x / P, p = blockIdx.x - b * P;
    const int q0 = p * chunk, q1 = min(HW, q0 + chunk);
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    if (pl < npl) {
        const int c = (cv0 + cvl) * V;
        for (int q = q0 + pl; q < q1; q += npl) {
            const long long pix = (long long)b * HW + q;
            typename vec<V>::t xv = ldv<V>(x + pix * ldx + c);
            if (PROD) xv = xv * ldv<V>(y + pix * ldy + c);
            if constexpr (V == 1) { acc[0] += xv; }
            else { acc[0] += xv.x; acc[1] += xv.y; acc[2] += xv.z; acc[3] += xv.w; }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) red[(pl * CVb + cvl) * V + v] = acc[v];
    }
    __syncthreads();
    if (pl == 0) {
        float s[V];
#pragma unroll
        for (int v = 0; v < V; ++v) s[v] = red[cvl * V + v];
        for (int k = 1; k < npl; ++k)
#pragma unroll
            for (int v = 0; v < V; ++v) s[v] += red[(k * CVb + cvl) * V + v];
        float* o = part + ((long long)b * P + p) * C + (cv0 + cvl) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = s[v];
    }
}

// One workgroup per row b: pool = (sum of the P partials, in order) / HW; h = relu(W_down pool + b_down) (one wave per hidden unit, lanes over
// the channels, a fixed shuffle tree); a = sigmoid(W_up h + b_up).  Writes pool, h (post-ReLU) and a, (B, C) / (B, Hd) dense.
__global__ __launch_bounds__(OD_THREADS) void chatt_mlp_fwd_kernel(const float* __restrict__ part, int P, float inv_hw, const float* __restrict__ wd,
                                                                   const float* __restrict__ bd, const float* __restrict__ wu, const float* __restrict__ bu,
                                                                   float* __restrict__ pool, float* __restrict__ hid, float* __restrict__ a, int C, int Hd) {
    extern __shared__ float lds[];
    float* pool_s = lds;            // C
    float* h_s = lds + C;           // Hd
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int c = t; c < C; c += OD_THREADS) {
        float s = 0.f;
        for (int p = 0; p < P; ++p) s += part[((long long)b * P + p) * C + c];
        const float m = s * inv_hw;
        pool_s[c] = m;
        pool[(long long)b * C + c] = m;
    }
    __syncthreads();
    for (int j = wave; j < Hd; j += OD_THREADS / 64) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += wd[(long long)j * C + c] * pool_s[c];
        s = mrdis_wave_sum(s);
        if (lane == 0) {
            const float v = fmaxf(s + bd[j], 0.f);
            h_s[j] = v;
            hid[(long long)b * Hd + j] = v;
        }
    }
    __syncthreads();
    for (int c = t; c < C; c += OD_THREADS) {
        float z = 0.f;
        for (int j = 0; j < Hd; ++j) z += wu[(long long)c * Hd + j] * h_s[j];
        z += bu[c];
        a[(long long)b * C + c] = 1.f / (1.f + expf(-z));
    }
}

// skip = (1 + a[b, c]) * x + s into the output view
template <int V>
__global__ __launch_bounds__(OD_THREADS) void chatt_combine_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ s, int lds,
                                                                   const float* __restrict__ a, float* __restrict__ out, int ldo, long long HW, int C) {
    const int CV = C / V;
    const long long total = HW * CV;                 // per image (blockIdx.y)
    const int b = blockIdx.y;
    const float* ab = a + (long long)b * C;
    for (long long e = blockIdx.x * (long long)OD_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * OD_THREADS) {
        const long long pix = (long long)b * HW + e / CV;
        const int c = (int)(e % CV) * V;
        typename vec<V>::t av = ldv<V>(ab + c);
        const typename vec<V>::t r = (1.f + av) * ldv<V>(x + pix * ldx + c) + ldv<V>(s + pix * lds + c);
        stv<V>(out + pix * ldo + c, r);
    }
}

// The MLP backward for all rows in ONE workgroup (phases separated by barriers; every sum over the batch runs b = 0 .. B-1 in order):
//   dzu = (da (1 - a)) a, da = sum of the P partials of dy * x            -> ws_dzu (B, C)
//   dW_up[c, j] = sum_b dzu[b, c] h[b, j]; db_up[c] = sum_b dzu[b, c]; dzd[b, j] = [h > 0] sum_c dzu[b, c] W_up[c, j]   -> ws_dzd (B, Hd)
//   dW_down[j, c] = sum_b dzd[b, j] pool[b, c]; db_down[j] = sum_b dzd[b, j]; dpool_hw[b, c] = (sum_j dzd[b, j] W_down[j, c]) / HW
__global__ __launch_bounds__(OD_MLP_BWD_THREADS) void chatt_mlp_bwd_kernel(const float* __restrict__ part, int P, float inv_hw,
                                                                           const float* __restrict__ a, const float* __restrict__ hid,
                                                                           const float* __restrict__ pool, const float* __restrict__ wd,
                                                                           const float* __restrict__ wu, float* __restrict__ dwd, float* __restrict__ dbd,
                                                                           float* __restrict__ dwu, float* __restrict__ dbu, float* dzu, float* dzd,
                                                                           float* __restrict__ dpool_hw, int B, int C, int Hd) {
    const int t = threadIdx.x, T = OD_MLP_BWD_THREADS;
    for (int e = t; e < B * C; e += T) {
        const int b = e / C, c = e - b * C;
        float da = 0.f;
        for (int p = 0; p < P; ++p) da += part[((long long)b * P + p) * C + c];
        const float av = a[e];
        dzu[e] = da * (1.f - av) * av;
    }
    __threadfence_block();
    __syncthreads();
    for (int e = t; e < C * Hd; e += T) {
        const int c = e / Hd, j = e - c * Hd;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dzu[(long long)b * C + c] * hid[(long long)b * Hd + j];
        dwu[e] = s;
    }
    for (int c = t; c < C; c += T) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dzu[(long long)b * C + c];
        dbu[c] = s;
    }
    for (int e = t; e < B * Hd; e += T) {
        const int b = e / Hd, j = e - b * Hd;
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += dzu[(long long)b * C + c] * wu[(long long)c * Hd + j];
        dzd[e] = hid[e] > 0.f ? s : 0.f;
    }
    __threadfence_block();
    __syncthreads();
    for (int e = t; e < Hd * C; e += T) {
        const int j = e / C, c = e - j * C;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dzd[(long long)b * Hd + j] * pool[(long long)b * C + c];
        dwd[e] = s;
    }
    for (int j = t; j < Hd; j += T) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dzd[(long long)b * Hd + j];
        dbd[j] = s;
    }
    for (int e = t; e < B * C; e += T) {
        const int b = e / C, c = e - b * C;
        float s = 0.f;
        for (int j = 0; j < Hd; ++j) s += dzd[(long long)b * Hd + j] * wd[(long long)j * C + c];
        dpool_hw[e] = s * inv_hw;
    }
}

// dx = (1 + a[b, c]) * dy + dpool_hw[b, c]
template <int V>
__global__ __launch_bounds__(OD_THREADS) void chatt_dx_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ a,
                                                              const float* __restrict__ dpool_hw, float* __restrict__ dx, int lddx, long long HW, int C) {
    const int CV = C / V;
    const long long total = HW * CV;
    const int b = blockIdx.y;
    const float* ab = a + (long long)b * C;
    const float* gb = dpool_hw + (long long)b * C;
    for (long long e = blockIdx.x * (long long)OD_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * OD_THREADS) {
        const long long pix = (long long)b * HW + e / CV;
        const int c = (int)(e % CV) * V;
        const typename vec<V>::t r = (1.f + ldv<V>(ab + c)) * ldv<V>(dy + pix * lddy + c) + ldv<V>(gb + c);
        stv<V>(dx + pix * lddx + c, r);
    }
}

// ---------------------------------------------------------------- symmetric difference |g - flip_H(g)|
template <int V>
__global__ __launch_bounds__(OD_THREADS) void symdiff_fwd_kernel(const float* __restrict__ g, int ldg, float* __restrict__ gd, int ldo,
                                                                 int B, int H, int W, int C) {
    const int CV = C / V;
    const long long total = (long long)B * H * W * CV;
    for (long long e = blockIdx.x * (long long)OD_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * OD_THREADS) {
        const int c = (int)(e % CV) * V;
        long long r = e / CV;
        const int w = (int)(r % W); r /= W;
        const int h = (int)(r % H); const long long b = r / H;
        const long long p = (b * H + h) * W + w, pf = (b * H + (H - 1 - h)) * W + w;
        const typename vec<V>::t d = ldv<V>(g + p * ldg + c) - ldv<V>(g + pf * ldg + c);
        typename vec<V>::t o;
        if constexpr (V == 1) o = fabsf(d);
        else o = f32x4{fabsf(d.x), fabsf(d.y), fabsf(d.z), fabsf(d.w)};
        stv<V>(gd + p * ldo + c, o);
    }
}

__device__ __forceinline__ float sgnf(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

template <int V>
__global__ __launch_bounds__(OD_THREADS) void symdiff_bwd_kernel(const float* __restrict__ dgd, int lddgd, const float* __restrict__ g, int ldg,
                                                                 float* __restrict__ dg, int lddg, int B, int H, int W, int C) {
    const int CV = C / V;
    const long long total = (long long)B * H * W * CV;
    for (long long e = blockIdx.x * (long long)OD_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * OD_THREADS) {
        const int c = (int)(e % CV) * V;
        long long r = e / CV;
        const int w = (int)(r % W); r /= W;
        const int h = (int)(r % H); const long long b = r / H;
        const long long p = (b * H + h) * W + w, pf = (b * H + (H - 1 - h)) * W + w;
        const typename vec<V>::t d = ldv<V>(g + p * ldg + c) - ldv<V>(g + pf * ldg + c);
        const typename vec<V>::t s = ldv<V>(dgd + p * lddgd + c) + ldv<V>(dgd + pf * lddgd + c);
        typename vec<V>::t o;
        if constexpr (V == 1) o = sgnf(d) * s;
        else o = f32x4{sgnf(d.x) * s.x, sgnf(d.y) * s.y, sgnf(d.z) * s.z, sgnf(d.w) * s.w};
        stv<V>(dg + p * lddg + c, o);
    }
}

// ---------------------------------------------------------------- residual gate (1 + up2(alpha)) * x
// up2(alpha) at output pixel (y, x) of a (2h, 2w) map, align_corners=False (scale 1/2): ATen's source index, clamp and weights
__device__ __forceinline__ float up2_at(const float* __restrict__ al, int h, int w, int y, int x) {
    float sy = 0.5f * ((float)y + 0.5f) - 0.5f; if (sy < 0.f) sy = 0.f;
    float sx = 0.5f * ((float)x + 0.5f) - 0.5f; if (sx < 0.f) sx = 0.f;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = sy - (float)y0, ly0 = 1.f - ly1, lx1 = sx - (float)x0, lx0 = 1.f - lx1;
    return ly0 * (lx0 * al[y0 * w + x0] + lx1 * al[y0 * w + x1]) + ly1 * (lx0 * al[y1 * w + x0] + lx1 * al[y1 * w + x1]);
}

template <int V>
__global__ __launch_bounds__(OD_THREADS) void rgate_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ alpha,
                                                               float* __restrict__ out, int ldo, int B, int H, int W, int C) {
    const int CV = C / V, h = H / 2, w = W / 2;
    const long long total = (long long)B * H * W * CV;
    for (long long e = blockIdx.x * (long long)OD_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * OD_THREADS) {
        const int c = (int)(e % CV) * V;
        const long long pix = e / CV;
        long long r = pix;
        const int xx = (int)(r % W); r /= W;
        const int yy = (int)(r % H); const long long b = r / H;
        const float u = 1.f + up2_at(alpha + b * h * w, h, w, yy, xx);
        stv<V>(out + pix * ldo + c, u * ldv<V>(x + pix * ldx + c));
    }
}

// 16 lanes per pixel: lane l handles channel vectors l, l + 16, ...; dx element-wise, r[pix] = sum_c dy x (lane partials, then a fixed
// xor-shuffle tree inside the 16-lane group)
constexpr int RG_LANES = 16;
template <int V>
__global__ __launch_bounds__(OD_THREADS) void rgate_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                                               const float* __restrict__ alpha, float* __restrict__ dx, int lddx, float* __restrict__ rsum,
                                                               int B, int H, int W, int C) {
    const int CV = C / V, h = H / 2, w = W / 2;
    const long long npix = (long long)B * H * W;
    const int lane = threadIdx.x % RG_LANES;
    const long long groups_per_grid = (long long)gridDim.x * (OD_THREADS / RG_LANES);
    for (long long pix = blockIdx.x * (long long)(OD_THREADS / RG_LANES) + threadIdx.x / RG_LANES; pix < npix; pix += groups_per_grid) {
        long long r = pix;
        const int xx = (int)(r % W); r /= W;
        const int yy = (int)(r % H); const long long b = r / H;
        const float u = 1.f + up2_at(alpha + b * h * w, h, w, yy, xx);
        float s = 0.f;
        for (int cv = lane; cv < CV; cv += RG_LANES) {
            const typename vec<V>::t g = ldv<V>(dy + pix * lddy + cv * V);
            stv<V>(dx + pix * lddx + cv * V, u * g);
            s += hsum(g * ldv<V>(x + pix * ldx + cv * V));
        }
#pragma unroll
        for (int o = RG_LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, RG_LANES);
        if (lane == 0) rsum[pix] = s;
    }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct ChattGeom { int P, chunk, CG; };
ChattGeom chatt_geom(int B, long long HW, int C, int V) {
    ChattGeom g;
    const int CV = C / V;
    g.CG = (CV + OD_THREADS - 1) / OD_THREADS;
    long long P = 1024 / ((long long)B * g.CG);
    const long long maxP = HW / 64 > 0 ? HW / 64 : 1;       // at least ~64 pixels per chunk
    if (P > maxP) P = maxP;
    if (P < 1) P = 1;
    g.chunk = (int)((HW + P - 1) / P);
    g.P = (int)((HW + g.chunk - 1) / g.chunk);
    return g;
}
int chatt_vec(int C, std::initializer_list<const void*> ptrs, std::initializer_list<int> lds) {
    if (C % 4) return 1;
    for (const void* p : ptrs) if (p && !al16(p)) return 1;
    for (int l : lds) if (l % 4) return 1;
    return 4;
}

}  // namespace

// workspace floats: the partial sums (B * P * C) of either direction, then for the backward dzu (B * C), dzd (B * Hd) and dpool (B * C)
extern "C" size_t mrdis_chatt_workspace(int B, long long HW, int C, int Hd) {
    if (B < 1 || HW < 1 || C < 1 || Hd < 1) return 0;
    const ChattGeom g = chatt_geom(B, HW, C, C % 4 ? 1 : 4);
    const ChattGeom g1 = chatt_geom(B, HW, C, 1);
    const long long P = g.P > g1.P ? g.P : g1.P;
    return (size_t)((long long)B * P * C + 2LL * B * C + (long long)B * Hd) * sizeof(float) + 256;
}

extern "C" int mrdis_chatt_fwd(const float* x, int ldx, const float* s, int lds, const float* wd, const float* bd, const float* wu, const float* bu,
                               float* out, int ldo, float* pool, float* hid, float* a, void* ws, size_t ws_bytes, int B, long long HW, int C, int Hd,
                               void* stream) {
    if (!x || !s || !wd || !bd || !wu || !bu || !out || !pool || !hid || !a || !ws || B < 1 || HW < 1 || C < 1 || Hd < 1 ||
        ldx < C || lds < C || ldo < C)
        return MRDIS_EINVAL;
    if (C > 4096 || Hd > 1024) return MRDIS_EUNSUPPORTED;
    if (ws_bytes < mrdis_chatt_workspace(B, HW, C, Hd)) return MRDIS_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int V = chatt_vec(C, {x, s, out}, {ldx, lds, ldo});
    if (V == 1) mrdis_count(MRDIS_CNT_ELEM_V1);
    const ChattGeom g = chatt_geom(B, HW, C, V);
    float* part = (float*)ws;
    mrdis_count(MRDIS_CNT_CHATT);
    if (V == 4) MRDIS_LAUNCH((chatt_partial_kernel<4, false>), dim3(B * g.P, g.CG), dim3(OD_THREADS), 0, st, x, ldx, nullptr, 0, part, (int)HW, C, g.P, g.chunk);
    else MRDIS_LAUNCH((chatt_partial_kernel<1, false>), dim3(B * g.P, g.CG), dim3(OD_THREADS), 0, st, x, ldx, nullptr, 0, part, (int)HW, C, g.P, g.chunk);
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(chatt_mlp_fwd_kernel, dim3(B), dim3(OD_THREADS), (size_t)(C + Hd) * sizeof(float), st, part, g.P, 1.f / (float)HW, wd, bd, wu, bu,
                 pool, hid, a, C, Hd);
    MRDIS_CHECK_LAUNCH();
    const int gx = od_image_grid(HW * (C / V), B);
    if (V == 4) MRDIS_LAUNCH((chatt_combine_kernel<4>), dim3(gx, B), dim3(OD_THREADS), 0, st, x, ldx, s, lds, a, out, ldo, HW, C);
    else MRDIS_LAUNCH((chatt_combine_kernel<1>), dim3(gx, B), dim3(OD_THREADS), 0, st, x, ldx, s, lds, a, out, ldo, HW, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_chatt_bwd(const float* dy, int lddy, const float* x, int ldx, const float* a, const float* hid, const float* pool,
                               const float* wd, const float* wu, float* dx, int lddx, float* dwd, float* dbd, float* dwu, float* dbu,
                               void* ws, size_t ws_bytes, int B, long long HW, int C, int Hd, void* stream) {
    if (!dy || !x || !a || !hid || !pool || !wd || !wu || !dx || !dwd || !dbd || !dwu || !dbu || !ws || B < 1 || HW < 1 || C < 1 || Hd < 1 ||
        lddy < C || ldx < C || lddx < C)
        return MRDIS_EINVAL;
    if (C > 4096 || Hd > 1024) return MRDIS_EUNSUPPORTED;
    if (ws_bytes < mrdis_chatt_workspace(B, HW, C, Hd)) return MRDIS_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int V = chatt_vec(C, {dy, x, dx}, {lddy, ldx, lddx});
    if (V == 1) mrdis_count(MRDIS_CNT_ELEM_V1);
    const ChattGeom g = chatt_geom(B, HW, C, V);
    float* part = (float*)ws;
    float* dzu = part + (long long)B * g.P * C;
    float* dpool = dzu + (long long)B * C;
    float* dzd = dpool + (long long)B * C;
    mrdis_count(MRDIS_CNT_CHATT);
    if (V == 4) MRDIS_LAUNCH((chatt_partial_kernel<4, true>), dim3(B * g.P, g.CG), dim3(OD_THREADS), 0, st, x, ldx, dy, lddy, part, (int)HW, C, g.P, g.chunk);
    else MRDIS_LAUNCH((chatt_partial_kernel<1, true>), dim3(B * g.P, g.CG), dim3(OD_THREADS), 0, st, x, ldx, dy, lddy, part, (int)HW, C, g.P, g.chunk);
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(chatt_mlp_bwd_kernel, dim3(1), dim3(OD_MLP_BWD_THREADS), 0, st, part, g.P, 1.f / (float)HW, a, hid, pool, wd, wu, dwd, dbd, dwu, dbu,
                 dzu, dzd, dpool, B, C, Hd);
    MRDIS_CHECK_LAUNCH();
    const int gx = od_image_grid(HW * (C / V), B);
    if (V == 4) MRDIS_LAUNCH((chatt_dx_kernel<4>), dim3(gx, B), dim3(OD_THREADS), 0, st, dy, lddy, a, dpool, dx, lddx, HW, C);
    else MRDIS_LAUNCH((chatt_dx_kernel<1>), dim3(gx, B), dim3(OD_THREADS), 0, st, dy, lddy, a, dpool, dx, lddx, HW, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_symdiff_fwd(const float* g, int ldg, float* gd, int ldo, int B, int H, int W, int C, void* stream) {
    if (!g || !gd || B < 1 || H < 1 || W < 1 || C < 1 || ldg < C || ldo < C) return MRDIS_EINVAL;
    const int V = chatt_vec(C, {g, gd}, {ldg, ldo});
    if (V == 1) mrdis_count(MRDIS_CNT_ELEM_V1);
    const long long n = (long long)B * H * W * (C / V);
    mrdis_count(MRDIS_CNT_SYMDIFF);
    if (V == 4) MRDIS_LAUNCH((symdiff_fwd_kernel<4>), dim3(od_grid(n, OD_THREADS)), dim3(OD_THREADS), 0, (hipStream_t)stream, g, ldg, gd, ldo, B, H, W, C);
    else MRDIS_LAUNCH((symdiff_fwd_kernel<1>), dim3(od_grid(n, OD_THREADS)), dim3(OD_THREADS), 0, (hipStream_t)stream, g, ldg, gd, ldo, B, H, W, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_symdiff_bwd(const float* dgd, int lddgd, const float* g, int ldg, float* dg, int lddg, int B, int H, int W, int C, void* stream) {
    if (!dgd || !g || !dg || B < 1 || H < 1 || W < 1 || C < 1 || lddgd < C || ldg < C || lddg < C) return MRDIS_EINVAL;
    const int V = chatt_vec(C, {dgd, g, dg}, {lddgd, ldg, lddg});
    if (V == 1) mrdis_count(MRDIS_CNT_ELEM_V1);
    const long long n = (long long)B * H * W * (C / V);
    mrdis_count(MRDIS_CNT_SYMDIFF);
    if (V == 4) MRDIS_LAUNCH((symdiff_bwd_kernel<4>), dim3(od_grid(n, OD_THREADS)), dim3(OD_THREADS), 0, (hipStream_t)stream, dgd, lddgd, g, ldg, dg, lddg, B, H, W, C);
    else MRDIS_LAUNCH((symdiff_bwd_kernel<1>), dim3(od_grid(n, OD_THREADS)), dim3(OD_THREADS), 0, (hipStream_t)stream, dgd, lddgd, g, ldg, dg, lddg, B, H, W, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_rgate_fwd(const float* x, int ldx, const float* alpha, float* out, int ldo, int B, int H, int W, int C, void* stream) {
    if (!x || !alpha || !out || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1 || ldx < C || ldo < C) return MRDIS_EINVAL;
    const int V = chatt_vec(C, {x, out}, {ldx, ldo});
    if (V == 1) mrdis_count(MRDIS_CNT_ELEM_V1);
    const long long n = (long long)B * H * W * (C / V);
    mrdis_count(MRDIS_CNT_RGATE);
    if (V == 4) MRDIS_LAUNCH((rgate_fwd_kernel<4>), dim3(od_grid(n, OD_THREADS)), dim3(OD_THREADS), 0, (hipStream_t)stream, x, ldx, alpha, out, ldo, B, H, W, C);
    else MRDIS_LAUNCH((rgate_fwd_kernel<1>), dim3(od_grid(n, OD_THREADS)), dim3(OD_THREADS), 0, (hipStream_t)stream, x, ldx, alpha, out, ldo, B, H, W, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_rgate_bwd(const float* dy, int lddy, const float* x, int ldx, const float* alpha, float* dx, int lddx, float* rsum,
                               int B, int H, int W, int C, void* stream) {
    if (!dy || !x || !alpha || !dx || !rsum || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1 || lddy < C || ldx < C || lddx < C)
        return MRDIS_EINVAL;
    const int V = chatt_vec(C, {dy, x, dx}, {lddy, ldx, lddx});
    if (V == 1) mrdis_count(MRDIS_CNT_ELEM_V1);
    const long long npix = (long long)B * H * W;
    const int grid = od_grid(npix, OD_THREADS / RG_LANES);
    mrdis_count(MRDIS_CNT_RGATE);
    if (V == 4) MRDIS_LAUNCH((rgate_bwd_kernel<4>), dim3(grid), dim3(OD_THREADS), 0, (hipStream_t)stream, dy, lddy, x, ldx, alpha, dx, lddx, rsum, B, H, W, C);
    else MRDIS_LAUNCH((rgate_bwd_kernel<1>), dim3(grid), dim3(OD_THREADS), 0, (hipStream_t)stream, dy, lddy, x, ldx, alpha, dx, lddx, rsum, B, H, W, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
