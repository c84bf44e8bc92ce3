// Objective and segmentation counts of the 3-D nets (model3d.nvnet_loss_hip / model3d.seg_metrics).
//
// nvnet_loss (model3d.py) = soft Dice of sigmoid(uout) against the region channels + 0.1 * mean squared error of the VAE reconstruction (+ a KL
// term on (B, 16) rows that stays in torch).  The Dice term is GLOBAL over the batch, so both terms are plain sums over flat buffers:
//   A = sum p t,  P2 = sum p^2,  T2 = sum t^2  (p = sigmoid(u))      SE = sum (v - x)^2
//   dice = 1 - 2 A / (P2 + T2 + 1e-6)          l2 = SE / n_vx          objective = dice + w_l2 * l2
// The torch composition makes about a dozen passes over 100-134 MB tensors at 4 x 128^3 and as many again in autograd; here the forward is ONE
// pass over the four tensors and the backward ONE pass that writes both gradients:
//   du = g [(-2 t / den + 4 A p / den^2) p (1 - p)]        dv = g w_l2 2 (v - x) / n_vx            den = P2 + T2 + 1e-6
//
// Access.  uout / target (and vout / x) must be dense and share one memory layout (the entry points check the strides; a mismatch is an error, never
// a copy), so the element order does not matter and every buffer is read flat: 16 bytes per lane, 1 KB per wave instruction, grid-stride with
// four loads of each tensor in flight per thread; a tail of n % 4 floats goes through 4-byte accesses.  That loop is written once (l3_stream) and
// takes what to do with each pair as a functor.  Bandwidth-bound: ~30 VALU instructions per element (accurate expf + an IEEE division for the
// sigmoid) stay under the memory time.
//
// Numerics.  p is the fp32 sigmoid torch computes (1 / (1 + expf(-u))).  Products and sums are then carried in fp64: p t, p^2, t^2 and (v - x)^2
// of fp32 values are exact in fp64, so the four sums carry the rounding of p and nothing else worth naming; the fp64 arithmetic stays under the
// memory time (measured: the forward reads at 5.45 TB/s at 4 x 128^3, beside 5.5 TB/s for a store-only pass; profiles/loss3d_bench.txt).
// Reduction order is fixed: thread -> wave (shuffles) -> workgroup (LDS) -> one fp64 partial row per workgroup in the caller's workspace -> a
// single-workgroup finish kernel.  No floating-point atomics: the same inputs give the same bits on every run.
//
// mrdis_seg_counts: per (sample, channel) the three integer counts the reference's Dice / IoU are made of (util.py:980-992), exact in int32.
// A thread takes four positions of a channels-last sample (C consecutive 16-byte loads), so the channel of every register is static; counts go
// thread -> wave -> workgroup -> one integer atomicAdd per (workgroup, channel, count), exact in any order.
#include "mrdis_common.h"
#include <math.h>

namespace {
constexpr int L3_THREADS = 256;
constexpr int L3_MAX_BLOCKS = 2048;          // 256 CUs x 8 workgroups: the grid of a memory-bound pass (cdna_hip_programming.md Guideline 11)
constexpr int L3_UNROLL = 4;

struct L3Sums { double a, p2, t2, se; };
struct L3Coef { double c1, c2, cv; };

// per-element operations: two that add to the running sums, two that give a gradient
struct L3AccUT {
    __device__ __forceinline__ void operator()(float u, float t, L3Sums& s) const {
        const double p = (double)mrdis_sigmoid(u), td = (double)t;
        s.a = fma(p, td, s.a); s.p2 = fma(p, p, s.p2); s.t2 = fma(td, td, s.t2);
    }
};
struct L3AccVX {
    __device__ __forceinline__ void operator()(float v, float x, L3Sums& s) const {
        const double d = (double)v - (double)x;
        s.se = fma(d, d, s.se);
    }
};
struct L3GradU {
    L3Coef c;
    __device__ __forceinline__ float operator()(float u, float t) const {
        const double p = (double)mrdis_sigmoid(u);
        return (float)(fma(c.c2, p, c.c1 * (double)t) * (p * (1.0 - p)));
    }
};
struct L3GradV {
    L3Coef c;
    __device__ __forceinline__ float operator()(float v, float x) const { return (float)(c.cv * ((double)v - (double)x)); }
};

// what the streaming loop does with a float4 pair / a tail element: fold it into the sums, or store op(a, b)
template <class Op>
struct L3Reduce {
    Op op; L3Sums& s;
    __device__ __forceinline__ void vec(long long, const f32x4& a, const f32x4& b) { op(a.x, b.x, s); op(a.y, b.y, s); op(a.z, b.z, s); op(a.w, b.w, s); }
    __device__ __forceinline__ void one(long long, float a, float b) { op(a, b, s); }
};
template <class Op>
struct L3Map {
    Op op; float* __restrict__ out;
    __device__ __forceinline__ void vec(long long i, const f32x4& a, const f32x4& b) {
        const f32x4 r = {op(a.x, b.x), op(a.y, b.y), op(a.z, b.z), op(a.w, b.w)};
        reinterpret_cast<f32x4*>(out)[i] = r;
    }
    __device__ __forceinline__ void one(long long i, float a, float b) { out[i] = op(a, b); }
};

// THE streaming loop of this file: both flat buffers of n floats, 16 bytes per lane, grid-stride over the whole launch (tid of T threads), L3_UNROLL
// loads of each buffer in flight per thread, then the remainder, then the n % 4 tail through 4-byte accesses (thread tid takes element 4 (n / 4) + tid)
template <class Sink>
__device__ __forceinline__ void l3_stream(const float* __restrict__ pa, const float* __restrict__ pb, long long n, long long tid, long long T, Sink sink) {
    const long long nv = n >> 2;
    const f32x4* a4 = reinterpret_cast<const f32x4*>(pa);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(pb);
    long long i = tid;
    for (; i + (L3_UNROLL - 1) * T < nv; i += L3_UNROLL * T) {
        f32x4 a[L3_UNROLL], b[L3_UNROLL];
#pragma unroll
        for (int k = 0; k < L3_UNROLL; ++k) { a[k] = a4[i + k * T]; b[k] = b4[i + k * T]; }
#pragma unroll
        for (int k = 0; k < L3_UNROLL; ++k) sink.vec(i + k * T, a[k], b[k]);
    }
    for (; i < nv; i += T) sink.vec(i, a4[i], b4[i]);
    if (tid < n - 4 * nv) sink.one(4 * nv + tid, pa[4 * nv + tid], pb[4 * nv + tid]);
}

// part[blockIdx.x][4] = this workgroup's { A, P2, T2, SE }.  grid <= L3_MAX_BLOCKS, 256 threads.  v == nullptr: no reconstruction term.
__global__ __launch_bounds__(L3_THREADS) void nvnet_loss_fwd_kernel(const float* __restrict__ u, const float* __restrict__ t, long long n1,
                                                                    const float* __restrict__ v, const float* __restrict__ x, long long n2,
                                                                    double* __restrict__ part) {
    __shared__ double red[L3_THREADS / 64][4];
    L3Sums s = {0.0, 0.0, 0.0, 0.0};
    const long long tid = blockIdx.x * (long long)L3_THREADS + threadIdx.x, T = gridDim.x * (long long)L3_THREADS;
    l3_stream(u, t, n1, tid, T, L3Reduce<L3AccUT>{L3AccUT{}, s});
    if (v != nullptr) l3_stream(v, x, n2, tid, T, L3Reduce<L3AccVX>{L3AccVX{}, s});
    s.a = mrdis_wave_sum_d(s.a); s.p2 = mrdis_wave_sum_d(s.p2); s.t2 = mrdis_wave_sum_d(s.t2); s.se = mrdis_wave_sum_d(s.se);
    if ((threadIdx.x & 63) == 0) {
        double* r = red[threadIdx.x >> 6];
        r[0] = s.a; r[1] = s.p2; r[2] = s.t2; r[3] = s.se;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        part[4 * (long long)blockIdx.x + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// one workgroup: sums[4] = the partial rows added in a fixed order; terms = { dice, l2, dice + w_l2 * l2 } rounded once from fp64
__global__ __launch_bounds__(L3_THREADS) void nvnet_loss_finish_kernel(const double* __restrict__ part, int nblk, long long n2, double w_l2,
                                                                       double* __restrict__ sums, float* __restrict__ terms) {
    __shared__ double red[L3_THREADS / 64][4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < nblk; k += L3_THREADS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += part[4 * (long long)k + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = mrdis_wave_sum_d(s[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) red[threadIdx.x >> 6][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { r[j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]); sums[j] = r[j]; }
        const double dice = 1.0 - 2.0 * r[0] / (r[1] + r[2] + 1e-6);
        const double l2 = n2 > 0 ? r[3] / (double)n2 : 0.0;
        terms[0] = (float)dice; terms[1] = (float)l2; terms[2] = (float)(dice + w_l2 * l2);
    }
}

// du / dv in the layout of u / v (flat).  du == nullptr or dv == nullptr: that gradient is not wanted.  sums, g: device memory, no host sync.
__global__ __launch_bounds__(L3_THREADS) void nvnet_loss_bwd_kernel(const float* __restrict__ u, const float* __restrict__ t, float* __restrict__ du,
                                                                    long long n1, const float* __restrict__ v, const float* __restrict__ x,
                                                                    float* __restrict__ dv, long long n2, const double* __restrict__ sums,
                                                                    const float* __restrict__ g, double w_l2) {
    const double gg = (double)g[0];
    const double den = sums[1] + sums[2] + 1e-6;
    L3Coef c;
    c.c1 = -2.0 * gg / den; c.c2 = 4.0 * gg * sums[0] / (den * den); c.cv = n2 > 0 ? gg * w_l2 * 2.0 / (double)n2 : 0.0;
    const long long tid = blockIdx.x * (long long)L3_THREADS + threadIdx.x, T = gridDim.x * (long long)L3_THREADS;
    if (du != nullptr) l3_stream(u, t, n1, tid, T, L3Map<L3GradU>{L3GradU{c}, du});
    if (dv != nullptr) l3_stream(v, x, n2, tid, T, L3Map<L3GradV>{L3GradV{c}, dv});
}

// out[b][c][3] += { |pred > 0.5 and t == 1|, |pred > 0.5|, |t == 1| } over the P positions of sample b; memory [b][position][c].
// grid (gx, B), 256 threads; a thread takes groups of four positions = C float4 per tensor.  VEC: (P C) % 4 == 0 and 16-byte aligned bases.
template <int C, bool VEC>
__global__ __launch_bounds__(L3_THREADS) void seg_counts_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, long long P,
                                                                int apply_sigmoid, int* __restrict__ out) {
    __shared__ int red[L3_THREADS / 64][3 * C];
    const int b = blockIdx.y;
    const float* pb = pred + (long long)b * P * C;
    const float* tb = tgt + (long long)b * P * C;
    int cnt[C][3];
#pragma unroll
    for (int c = 0; c < C; ++c) { cnt[c][0] = 0; cnt[c][1] = 0; cnt[c][2] = 0; }
    const long long ngrp = (P + 3) >> 2;
    for (long long gi = blockIdx.x * (long long)L3_THREADS + threadIdx.x; gi < ngrp; gi += gridDim.x * (long long)L3_THREADS) {
        const long long e0 = gi * 4 * C;
        const long long left = P * C - e0;                 // floats of this sample from e0 on (a whole number of positions)
        float pv[4 * C], tv[4 * C];
        if (VEC && left >= 4 * C) {
            const f32x4* p4 = reinterpret_cast<const f32x4*>(pb + e0);
            const f32x4* t4 = reinterpret_cast<const f32x4*>(tb + e0);
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const f32x4 a = p4[j], q = t4[j];
                pv[4 * j] = a.x; pv[4 * j + 1] = a.y; pv[4 * j + 2] = a.z; pv[4 * j + 3] = a.w;
                tv[4 * j] = q.x; tv[4 * j + 1] = q.y; tv[4 * j + 2] = q.z; tv[4 * j + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4 * C; ++j) {
                const bool in = j < left;
                pv[j] = in ? pb[e0 + j] : -1.f;            // beyond the sample: neither predicted (sigmoid(-1) < 0.5) nor labelled
                tv[j] = in ? tb[e0 + j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4 * C; ++j) {
            const float q = apply_sigmoid ? mrdis_sigmoid(pv[j]) : pv[j];
            const bool pp = q > 0.5f, tt = tv[j] == 1.f;   // strictly above 0.5, util.py:986-987
            cnt[j % C][0] += (pp && tt) ? 1 : 0; cnt[j % C][1] += pp ? 1 : 0; cnt[j % C][2] += tt ? 1 : 0;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int v = cnt[c][k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][3 * c + k] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * C) {
        const int v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (v != 0) atomicAdd(out + (long long)b * 3 * C + threadIdx.x, v);
    }
}

// Do `sa` and `sb` describe ONE dense layout of `shape`?  MRDIS_EINVAL: the two differ; MRDIS_EUNSUPPORTED: alike but with holes or overlaps.
// Dimensions of extent 1 carry no layout.  *numel = element count.
int l3_layout(int nd, const long long* shape, const long long* sa, const long long* sb, long long* numel) {
    if (nd < 1 || nd > 8 || !shape || !sa || !sb) return MRDIS_EINVAL;
    int idx[8], m = 0;
    long long n = 1;
    for (int d = 0; d < nd; ++d) {
        if (shape[d] < 1) return MRDIS_EINVAL;
        n *= shape[d];
        if (shape[d] == 1) continue;
        if (sa[d] != sb[d]) return MRDIS_EINVAL;
        idx[m++] = d;
    }
    for (int i = 1; i < m; ++i)                            // insertion sort by stride, innermost first
        for (int j = i; j > 0 && sa[idx[j]] < sa[idx[j - 1]]; --j) { const int tmp = idx[j]; idx[j] = idx[j - 1]; idx[j - 1] = tmp; }
    long long want = 1;
    for (int i = 0; i < m; ++i) {
        if (sa[idx[i]] != want) return MRDIS_EUNSUPPORTED;
        want *= shape[idx[i]];
    }
    *numel = n;
    return MRDIS_OK;
}

int l3_blocks(long long n1, long long n2) {
    const long long nv = (n1 > n2 ? n1 : n2) >> 2;
    long long nb = (nv + L3_THREADS - 1) / L3_THREADS;
    return nb < 1 ? 1 : (nb > L3_MAX_BLOCKS ? L3_MAX_BLOCKS : (int)nb);
}

bool l3_aligned(const void* a, const void* b, const void* c) { return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0; }

template <int C>
void launch_seg_counts(const float* pred, const float* tgt, long long P, int B, int apply_sigmoid, int* out, hipStream_t s) {
    const long long ngrp = (P + 3) >> 2;
    long long gx = (ngrp + L3_THREADS - 1) / L3_THREADS;
    const long long cap = L3_MAX_BLOCKS / B > 0 ? L3_MAX_BLOCKS / B : 1;
    if (gx > cap) gx = cap;
    const bool vec = ((P * C) & 3) == 0 && l3_aligned(pred, tgt, nullptr);
    if (vec) MRDIS_LAUNCH((seg_counts_kernel<C, true>), dim3((unsigned)gx, B), dim3(L3_THREADS), 0, s, pred, tgt, P, apply_sigmoid, out);
    else MRDIS_LAUNCH((seg_counts_kernel<C, false>), dim3((unsigned)gx, B), dim3(L3_THREADS), 0, s, pred, tgt, P, apply_sigmoid, out);
}
}  // namespace

extern "C" size_t mrdis_nvnet_loss_workspace(long long n_ut, long long n_vx) {
    if (n_ut < 1 || n_vx < 0) return 0;
    return sizeof(double) * 4 * (size_t)l3_blocks(n_ut, n_vx);
}

extern "C" int mrdis_nvnet_loss_fwd(const float* uout, const long long* stride_u, const float* target, const long long* stride_t,
                                    const long long* shape_ut, int nd_ut, const float* vout, const long long* stride_v, const float* x,
                                    const long long* stride_x, const long long* shape_vx, int nd_vx, double w_l2, double* sums, float* terms,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!uout || !target || !sums || !terms || !workspace || (vout == nullptr) != (x == nullptr)) return MRDIS_EINVAL;
    long long n1 = 0, n2 = 0;
    int rc = l3_layout(nd_ut, shape_ut, stride_u, stride_t, &n1);
    if (rc != MRDIS_OK) return rc;
    if (vout != nullptr && (rc = l3_layout(nd_vx, shape_vx, stride_v, stride_x, &n2)) != MRDIS_OK) return rc;
    if (!l3_aligned(uout, target, nullptr) || !l3_aligned(vout, x, workspace) || (((uintptr_t)sums) & 7) != 0) return MRDIS_EALIGN;
    if (workspace_bytes < mrdis_nvnet_loss_workspace(n1, n2)) return MRDIS_EWORKSPACE;
    const int nb = l3_blocks(n1, n2);
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    mrdis_count(MRDIS_CNT_LOSS3D);
    MRDIS_LAUNCH(nvnet_loss_fwd_kernel, dim3(nb), dim3(L3_THREADS), 0, s, uout, target, n1, vout, x, n2, part);
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(nvnet_loss_finish_kernel, dim3(1), dim3(L3_THREADS), 0, s, (const double*)part, nb, n2, w_l2, sums, terms);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_nvnet_loss_bwd(const float* uout, const long long* stride_u, const float* target, const long long* stride_t,
                                    const long long* shape_ut, int nd_ut, const float* vout, const long long* stride_v, const float* x,
                                    const long long* stride_x, const long long* shape_vx, int nd_vx, double w_l2, const double* sums,
                                    const float* g, float* du, float* dv, void* stream) {
    if (!uout || !target || !sums || !g || (vout == nullptr) != (x == nullptr) || (dv != nullptr && vout == nullptr) || (!du && !dv))
        return MRDIS_EINVAL;
    long long n1 = 0, n2 = 0;
    int rc = l3_layout(nd_ut, shape_ut, stride_u, stride_t, &n1);
    if (rc != MRDIS_OK) return rc;
    if (vout != nullptr && (rc = l3_layout(nd_vx, shape_vx, stride_v, stride_x, &n2)) != MRDIS_OK) return rc;
    if (!l3_aligned(uout, target, du) || !l3_aligned(vout, x, dv) || (((uintptr_t)sums) & 7) != 0) return MRDIS_EALIGN;
    mrdis_count(MRDIS_CNT_LOSS3D);
    MRDIS_LAUNCH(nvnet_loss_bwd_kernel, dim3(l3_blocks(du ? n1 : 0, dv ? n2 : 0)), dim3(L3_THREADS), 0, (hipStream_t)stream, uout, target, du, n1,
                 vout, x, dv, n2, sums, g, w_l2);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_seg_counts(const float* pred, const float* target, int* out, int B, long long P, int C, int apply_sigmoid, void* stream) {
    if (!pred || !target || !out || B < 1 || P < 1 || C < 1) return MRDIS_EINVAL;
    if (C > 4 || B > 65535 || P * C >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    if ((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)out) & 3) != 0) return MRDIS_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    mrdis_count(MRDIS_CNT_SEGCOUNTS);
    switch (C) {
        case 1: launch_seg_counts<1>(pred, target, P, B, apply_sigmoid, out, s); break;
        case 2: launch_seg_counts<2>(pred, target, P, B, apply_sigmoid, out, s); break;
        case 3: launch_seg_counts<3>(pred, target, P, B, apply_sigmoid, out, s); break;
        default: launch_seg_counts<4>(pred, target, P, B, apply_sigmoid, out, s); break;
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
