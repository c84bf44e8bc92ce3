// Preprocessing of raw scans on the device (prep.py: prep_stats / prep_write / build_store_from_raw): the rule that made the reference's h5 volumes
// (data_preprocessing_BraTS.py:70-98, commented out there; live in data_preprocessing_ZeroDose.py:124-134), from the voxel array as a NIfTI file holds
// it to the fp32 volume of a VolumeStore (D, H', W') or a VolumeStore3D (H', W', D).
//   v = double(raw) * slope + inter in float64 (two roundings, as numpy's `raw * slope + inter`: no FMA), NaN -> 0; the crop removes (h0, h1) / (w0, w1)
//   voxels at the low / high end of H / W and keeps the depth whole.
//   mrdis_prep_stats   stats[0] n = #(v > 0), [1] sum = sum v, [2] ssd = sum_{v > 0} (v - norm)^2 with norm = sum / (n + 1): over the CROPPED volume;
//                      [3] vmax = max v (NaN ignored), [4] nan_inner = #NaN with d in [d_lo, D - d_hi): over the UNCROPPED volume
//   mrdis_prep_write   zscore: (v - norm) / (sqrt(ssd / (n + 1)) + 1e-8), -10 where v <= 0 | mean: v / norm | label: v; rounded to fp32 at the store
// The host composition makes eight passes over a float64 copy of the volume; here the raw voxels are read three times in their own dtype (twice
// for the statistics: ssd needs norm) and the fp32 volume is written once.  A BraTS volume is 18 MB of int16, so the second and third read come from
// the Infinity Cache.
//
// Statistics: four launches, no atomics.  A partial-sum kernel walks the voxels in the order of the file (h fastest); workgroup b of nb takes the
// voxels i with (i / (256 VEC)) % nb == b, a thread VEC consecutive ones per round, and adds them in ascending i; the wave and the workgroup add
// in a fixed tree and one workgroup adds the nb partials in a fixed order, so two runs give the same bits.  nb depends on the geometry and on
// VEC alone, never on the device.  First (n, sum, vmax, nan_inner), then ssd with norm read from the device.  Counts are kept in float64: exact
// below 2^53.  VEC = 16 bytes' worth of voxels where the array is dense in file order (stride_h 1, stride_w H, stride_d H W) and 16-byte aligned
// -- one 16-byte load per lane and round, 1 KB per wave --; any other stride triple takes VEC = 1 and one load of the voxel's size per lane.
//
// Write: a workgroup owns a 64 x 64 tile of (h, q) at one r -- (q, r) = (w, d) for the (D, H', W') layout, (d, w) for (H', W', D) --, reads it
// along h (file order: 64 consecutive voxels per wave and row), parks the fp32 results in an LDS tile of row stride 65 words (both phases
// conflict-free) and stores it along q: runs of 64 floats (256 bytes), shorter at the edge of an extent that is no multiple of 64.  In the
// (H', W', D) layout a run starts wherever (h' W' + w') D lands, so with D % 16 != 0 (BraTS: 155) most runs begin and end inside a 64-byte line
// that the neighbouring workgroup (w' + 1) completes; the L2 merges them.  With other strides the same kernel is correct and its reads are strided.
#include "mrdis_common.h"
#include <math.h>

namespace {
constexpr int PS_THREADS = 256;
constexpr int PS_MAX_BLOCKS = 1024;           // partial sums of one pass
constexpr int PS_ROUNDS = 4;                  // rounds per thread the grid is sized for
constexpr int PW_THREADS = 256;
constexpr int PW_T = 64;                      // tile edge of the write kernel
constexpr int PREP_MAX_EXTENT = 1024;

struct PrepGeom {
    int H, W, D;
    int h_lo, h_hi, w_lo, w_hi;               // the crop keeps h in [h_lo, h_hi), w in [w_lo, w_hi)
    int d_lo, d_hi;                           // nan_inner counts d in [d_lo, d_hi)
    long long sh, sw, sd;                     // element strides
    double slope, inter;
    unsigned total;                           // H W D < 2^31
};

template <typename T>
__device__ __forceinline__ double prep_value(T x, double slope, double inter) {
    return __dadd_rn(__dmul_rn((double)x, slope), inter);        // two roundings: no contraction into an FMA
}

__device__ __forceinline__ double prep_wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}

// sum (IS_MAX: maximum) over the workgroup in a fixed order; the result is valid in thread 0
template <bool IS_MAX>
__device__ __forceinline__ double prep_block_reduce(double v, double* red) {
    v = IS_MAX ? prep_wave_max_d(v) : mrdis_wave_sum_d(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                             // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int k = 1; k < PS_THREADS / 64; ++k) r = IS_MAX ? fmax(r, red[k]) : r + red[k];
    return r;
}

// PASS 1: part[4 b + {0, 1, 2, 3}] = (n, sum, vmax, nan_inner) of workgroup b; PASS 2: part[b] = ssd of workgroup b, norm from stats
template <typename T, int VEC, int PASS>
__global__ __launch_bounds__(PS_THREADS) void prep_partial_kernel(const T* __restrict__ raw, PrepGeom g, const double* __restrict__ stats,
                                                                  double* __restrict__ part) {
    __shared__ double red[PS_THREADS / 64];
    double a_n = 0.0, a_sum = 0.0, a_nan = 0.0, a_ssd = 0.0, a_max = -INFINITY;
    double norm = 0.0;
    if constexpr (PASS == 2) norm = stats[1] / (stats[0] + 1.0);
    const unsigned step = gridDim.x * (unsigned)(PS_THREADS * VEC);
    for (unsigned i = (blockIdx.x * (unsigned)PS_THREADS + threadIdx.x) * VEC; i < g.total; i += step) {
        const unsigned t = i / (unsigned)g.H;
        int h = (int)(i - t * (unsigned)g.H), w = (int)(t % (unsigned)g.W), d = (int)(t / (unsigned)g.W);
        T x[VEC];
        if constexpr (VEC > 1) {                                 // dense file order: voxel i sits at raw + i
            if (i + VEC <= g.total) {
                union { uint4 q; T e[VEC]; } u;
                u.q = *reinterpret_cast<const uint4*>(raw + i);
#pragma unroll
                for (int j = 0; j < VEC; ++j) x[j] = u.e[j];
            } else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) x[j] = i + j < g.total ? raw[i + j] : T(0);
            }
        } else {
            x[0] = raw[h * g.sh + w * g.sw + d * g.sd];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (i + j < g.total) {
                double v = prep_value(x[j], g.slope, g.inter);
                const bool isn = v != v;
                const bool in_crop = h >= g.h_lo && h < g.h_hi && w >= g.w_lo && w < g.w_hi;
                if (isn) v = 0.0;
                if constexpr (PASS == 1) {
                    if (isn) { if (d >= g.d_lo && d < g.d_hi) a_nan += 1.0; }
                    else a_max = fmax(a_max, v);
                    if (in_crop) { a_sum += v; if (v > 0.0) a_n += 1.0; }
                } else {
                    if (in_crop && v > 0.0) { const double e = v - norm; a_ssd += e * e; }
                }
            }
            if (++h == g.H) { h = 0; if (++w == g.W) { w = 0; ++d; } }
        }
    }
    if constexpr (PASS == 1) {
        const double n = prep_block_reduce<false>(a_n, red), s = prep_block_reduce<false>(a_sum, red);
        const double m = prep_block_reduce<true>(a_max, red), c = prep_block_reduce<false>(a_nan, red);
        if (threadIdx.x == 0) { double* p = part + 4 * (size_t)blockIdx.x; p[0] = n; p[1] = s; p[2] = m; p[3] = c; }
    } else {
        const double q = prep_block_reduce<false>(a_ssd, red);
        if (threadIdx.x == 0) part[blockIdx.x] = q;
    }
}

// one workgroup: the nb partials in a fixed order.  PASS 1 writes stats[0], [1], [3], [4]; PASS 2 writes stats[2]
template <int PASS>
__global__ __launch_bounds__(PS_THREADS) void prep_finish_kernel(const double* __restrict__ part, int nb, double* __restrict__ stats) {
    __shared__ double red[PS_THREADS / 64];
    if constexpr (PASS == 1) {
        double a_n = 0.0, a_sum = 0.0, a_nan = 0.0, a_max = -INFINITY;
        for (int b = threadIdx.x; b < nb; b += PS_THREADS) {
            const double* p = part + 4 * (size_t)b;
            a_n += p[0]; a_sum += p[1]; a_max = fmax(a_max, p[2]); a_nan += p[3];
        }
        const double n = prep_block_reduce<false>(a_n, red), s = prep_block_reduce<false>(a_sum, red);
        const double m = prep_block_reduce<true>(a_max, red), c = prep_block_reduce<false>(a_nan, red);
        if (threadIdx.x == 0) { stats[0] = n; stats[1] = s; stats[3] = m; stats[4] = c; }
    } else {
        double a = 0.0;
        for (int b = threadIdx.x; b < nb; b += PS_THREADS) a += part[b];
        const double q = prep_block_reduce<false>(a, red);
        if (threadIdx.x == 0) stats[2] = q;
    }
}

// grid: (tiles of h) x (tiles of q) in x, r in y.  layout 0: (q, r) = (w, d), out (D, H', W'); layout 1: (q, r) = (d, w), out (H', W', D)
template <typename T>
__global__ __launch_bounds__(PW_THREADS) void prep_write_kernel(const T* __restrict__ raw, PrepGeom g, const double* __restrict__ stats,
                                                                float* __restrict__ out, int kind, int layout, int ntq) {
    __shared__ float tile[PW_T][PW_T + 1];
    const int Hc = g.h_hi - g.h_lo, Wc = g.w_hi - g.w_lo;
    const int Qc = layout ? g.D : Wc;
    const int th = (int)blockIdx.x / ntq, tq = (int)blockIdx.x - th * ntq, r = (int)blockIdx.y;
    const int hb = th * PW_T, qb = tq * PW_T;
    const int hn = min(PW_T, Hc - hb), qn = min(PW_T, Qc - qb);
    const long long sq = layout ? g.sd : g.sw, sr = layout ? g.sw : g.sd;
    const int q_lo = layout ? 0 : g.w_lo, r_lo = layout ? g.w_lo : 0;
    const T* src = raw + (g.h_lo + hb) * g.sh + (q_lo + qb) * sq + (r_lo + r) * sr;
    const int tx = threadIdx.x & (PW_T - 1), ty = threadIdx.x / PW_T;
    double norm = 0.0, den = 1.0;
    if (kind != MRDIS_PREP_LABEL) {
        const double n1 = stats[0] + 1.0;
        norm = stats[1] / n1;
        den = sqrt(stats[2] / n1) + 1e-8;
    }
    // every thread loads its PW_ROWS voxels unconditionally, from indices clamped into the tile (a tile at the edge reads its last row / column
    // again and never past the volume), so the loads of a thread are independent and issue back to back; the tile rows and columns beyond
    // (hn, qn) hold copies that the store phase does not read
    constexpr int PW_ROWS = PW_T / (PW_THREADS / PW_T);
    const T* col = src + min(tx, hn - 1) * g.sh;
    T x[PW_ROWS];
#pragma unroll
    for (int k = 0; k < PW_ROWS; ++k) x[k] = col[min(ty + k * (PW_THREADS / PW_T), qn - 1) * sq];
#pragma unroll
    for (int k = 0; k < PW_ROWS; ++k) {
        double v = prep_value(x[k], g.slope, g.inter);
        if (v != v) v = 0.0;
        float o;
        if (kind == MRDIS_PREP_ZSCORE) o = v > 0.0 ? (float)((v - norm) / den) : -10.0f;
        else if (kind == MRDIS_PREP_MEAN) o = (float)(v / norm);
        else o = (float)v;
        tile[ty + k * (PW_THREADS / PW_T)][tx] = o;
    }
    __syncthreads();
    const long long oh = layout ? (long long)Wc * g.D : Wc, orr = layout ? g.D : (long long)Hc * Wc;
    float* dst = out + hb * oh + qb + r * orr;
    if (tx < qn) {
#pragma unroll
        for (int k = 0; k < PW_ROWS; ++k) {
            const int hh = ty + k * (PW_THREADS / PW_T);
            if (hh < hn) dst[hh * oh + tx] = tile[tx][hh];
        }
    }
}

size_t prep_dtype_bytes(int dtype) {
    switch (dtype) {
        case MRDIS_PREP_U8: return 1;
        case MRDIS_PREP_I16: case MRDIS_PREP_U16: return 2;
        case MRDIS_PREP_I32: case MRDIS_PREP_F32: return 4;
        case MRDIS_PREP_F64: return 8;
        default: return 0;
    }
}

bool prep_geometry_ok(int H, int W, int D) {
    return H >= 1 && W >= 1 && D >= 1 && H <= PREP_MAX_EXTENT && W <= PREP_MAX_EXTENT && D <= PREP_MAX_EXTENT && (long long)H * W * D < (1LL << 31);
}

// MRDIS_OK and g filled in, or the error code of the first thing that is wrong
int prep_geom(PrepGeom& g, const void* raw, int dtype, long long sh, long long sw, long long sd, int H, int W, int D, int h0, int h1, int w0, int w1,
              double slope, double inter) {
    const size_t eb = prep_dtype_bytes(dtype);
    if (!raw || !eb || sh < 1 || sw < 1 || sd < 1 || h0 < 0 || h1 < 0 || w0 < 0 || w1 < 0) return MRDIS_EINVAL;
    if (!prep_geometry_ok(H, W, D) || (long long)h0 + h1 >= H || (long long)w0 + w1 >= W) return MRDIS_EUNSUPPORTED;
    if (((uintptr_t)raw) & (eb - 1)) return MRDIS_EALIGN;
    g.H = H; g.W = W; g.D = D; g.h_lo = h0; g.h_hi = H - h1; g.w_lo = w0; g.w_hi = W - w1; g.d_lo = 0; g.d_hi = D;
    g.sh = sh; g.sw = sw; g.sd = sd; g.slope = slope; g.inter = inter; g.total = (unsigned)((long long)H * W * D);
    return MRDIS_OK;
}

template <typename T>
void prep_stats_launch(const void* raw, const PrepGeom& g, double* stats, double* part, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const T* p = (const T*)raw;
    const bool dense = g.sh == 1 && g.sw == g.H && g.sd == (long long)g.H * g.W && (((uintptr_t)raw) & 15) == 0;
    const int per = PS_THREADS * PS_ROUNDS * (dense ? VEC : 1);
    const int nb = min(PS_MAX_BLOCKS, mrdis_cdiv(g.total, per));
    double* part2 = part + 4 * PS_MAX_BLOCKS;
    if (dense) MRDIS_LAUNCH((prep_partial_kernel<T, VEC, 1>), dim3(nb), dim3(PS_THREADS), 0, s, p, g, stats, part);
    else MRDIS_LAUNCH((prep_partial_kernel<T, 1, 1>), dim3(nb), dim3(PS_THREADS), 0, s, p, g, stats, part);
    MRDIS_LAUNCH(prep_finish_kernel<1>, dim3(1), dim3(PS_THREADS), 0, s, part, nb, stats);
    if (dense) MRDIS_LAUNCH((prep_partial_kernel<T, VEC, 2>), dim3(nb), dim3(PS_THREADS), 0, s, p, g, stats, part2);
    else MRDIS_LAUNCH((prep_partial_kernel<T, 1, 2>), dim3(nb), dim3(PS_THREADS), 0, s, p, g, stats, part2);
    MRDIS_LAUNCH(prep_finish_kernel<2>, dim3(1), dim3(PS_THREADS), 0, s, part2, nb, stats);
}

template <typename T>
void prep_write_launch(const void* raw, const PrepGeom& g, const double* stats, float* out, int kind, int layout, hipStream_t s) {
    const int Hc = g.h_hi - g.h_lo, Wc = g.w_hi - g.w_lo;
    const int nth = mrdis_cdiv(Hc, PW_T), ntq = mrdis_cdiv(layout ? g.D : Wc, PW_T);
    MRDIS_LAUNCH(prep_write_kernel<T>, dim3(nth * ntq, layout ? Wc : g.D), dim3(PW_THREADS), 0, s, (const T*)raw, g, stats, out, kind, layout, ntq);
}

#define PREP_DISPATCH(dtype, fn, ...)                                       \
    switch (dtype) {                                                        \
        case MRDIS_PREP_U8: fn<unsigned char>(__VA_ARGS__); break;          \
        case MRDIS_PREP_I16: fn<short>(__VA_ARGS__); break;                 \
        case MRDIS_PREP_U16: fn<unsigned short>(__VA_ARGS__); break;        \
        case MRDIS_PREP_I32: fn<int>(__VA_ARGS__); break;                   \
        case MRDIS_PREP_F32: fn<float>(__VA_ARGS__); break;                 \
        default: fn<double>(__VA_ARGS__); break;                            \
    }
}  // namespace

extern "C" size_t mrdis_prep_workspace(int H, int W, int D) {
    return prep_geometry_ok(H, W, D) ? (size_t)5 * PS_MAX_BLOCKS * sizeof(double) : 0;
}

extern "C" int mrdis_prep_stats(const void* raw, int dtype, long long stride_h, long long stride_w, long long stride_d, int H, int W, int D,
                                int h0, int h1, int w0, int w1, int d_lo, int d_hi, double slope, double inter, double* stats,
                                void* workspace, size_t workspace_bytes, void* stream) {
    PrepGeom g;
    if (!stats || !workspace || d_lo < 0 || d_hi < 0) return MRDIS_EINVAL;
    const int rc = prep_geom(g, raw, dtype, stride_h, stride_w, stride_d, H, W, D, h0, h1, w0, w1, slope, inter);
    if (rc != MRDIS_OK) return rc;
    if ((((uintptr_t)stats) | ((uintptr_t)workspace)) & 7) return MRDIS_EALIGN;
    if (workspace_bytes < mrdis_prep_workspace(H, W, D)) return MRDIS_EWORKSPACE;
    g.d_lo = d_lo; g.d_hi = D - d_hi;
    mrdis_count(MRDIS_CNT_PREPSTATS);
    PREP_DISPATCH(dtype, prep_stats_launch, raw, g, stats, (double*)workspace, (hipStream_t)stream)
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_prep_write(const void* raw, int dtype, long long stride_h, long long stride_w, long long stride_d, int H, int W, int D,
                                int h0, int h1, int w0, int w1, double slope, double inter, const double* stats, int kind, int layout,
                                float* out, void* stream) {
    PrepGeom g;
    if (!stats || !out || kind < MRDIS_PREP_ZSCORE || kind > MRDIS_PREP_LABEL || layout < MRDIS_PREP_DHW || layout > MRDIS_PREP_HWD) return MRDIS_EINVAL;
    const int rc = prep_geom(g, raw, dtype, stride_h, stride_w, stride_d, H, W, D, h0, h1, w0, w1, slope, inter);
    if (rc != MRDIS_OK) return rc;
    if ((((uintptr_t)stats) & 7) || (((uintptr_t)out) & 3)) return MRDIS_EALIGN;
    mrdis_count(MRDIS_CNT_PREPWRITE);
    PREP_DISPATCH(dtype, prep_write_launch, raw, g, stats, out, kind, layout, (hipStream_t)stream)
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
