// The way out of the store (prep.py: save_nifti / export_store_volume): prep_write_kernel of mrdis_prep.hip run backwards.  B volumes of one
// geometry in store layout -- (H', W', D) of a VolumeStore3D, of the label volumes and of the synthesized volumes, or (D, H', W') of a VolumeStore --
// go to FILE order (B, D, W, H), h fastest, on the full canvas H = H' + h0 + h1, W = W' + w0 + w1 the crop was cut from: what read_nifti returns and
// write_nifti takes.  Per output voxel: `fill` outside the crop; inside, the source voxel s as it is (COPY), s (std + 1e-8) + norm with -10.0f -> 0
// (UNZSCORE) or s norm (UNMEAN) in float64 -- multiply and add rounded separately, as prep_value does --, then ONE conversion to the destination:
// fp32 by rounding, int16 / uint8 by NaN -> 0, round to nearest even, clamp.  norm and std come from stats + 5 b as mrdis_prep_stats left them.
// COPY of a uint8 voxel (it fits every destination) and fp32 -> fp32 COPY (the bits) give what the rule gives without going through float64, and
// the fill is converted once per thread: the label path then costs a quarter less.
//
// One launch, no atomics: every output voxel is written once, by one thread.  A workgroup owns a 64 x 64 tile of (h, q) of the CANVAS at one r and
// one b -- (q, r) = (d, w) for (H', W', D), (w, d) for (D, H', W') --, so the margin is written by the tiles that hold it and there is no second pass.
//   read   lane tx walks q, the source's fastest axis (64 consecutive voxels per wave and row of h); voxels outside the crop are not read
//   park   the converted values as 32-bit words in an LDS tile [h][q] of row stride 65 words.  Banks are (word % 32) per 32-lane half for
//          ds_write_b32 / ds_read_b32 and 65 = 1 (mod 32): the write puts a half's 32 consecutive q on 32 banks; the read below has lane l of row
//          q at bank (EPL l + q + const) % 32, and a half holds 32 / EPL lanes of each of EPL neighbouring rows (LH below): 32 banks once each.  (Rows whose
//          start addresses differ mod 4 bytes -- an odd H under a 1- or 2-byte destination -- shift against each other by < EPL words: 2-way on
//          at most EPL - 1 lanes of a half.)
//   store  along h, FOUR BYTES PER LANE: a lane packs EPL = 4 / sizeof(Td) neighbouring voxels of one row into one aligned 32-bit store.  The row
//          start (base + ((b D + d) W + w) H + hb elements) is not promised to be 4-byte aligned, so lane l takes the aligned word that holds
//          elements EPL l - mis .. EPL l - mis + EPL - 1 of the run, mis = misalignment of the run in elements; a word that hangs over either end
//          of the run goes out one element at a time (at most two such words per row).  One byte per lane costs 3.5x a store-only pass
//          (mrdis_seg2d_finish).
#include "mrdis_common.h"
#include <math.h>

namespace {
constexpr int EX_THREADS = 256;
constexpr int EX_T = 64;                      // tile edge
constexpr int EX_MAX_EXTENT = 1024;
constexpr int EX_MAX_B = 65535;

struct ExportGeom {
    int H, W, D;                              // the canvas
    int Hc, Wc;                               // the cropped extents of the source
    int h0, w0;                               // the source's origin on the canvas
};

template <typename Td>
__device__ __forceinline__ unsigned export_convert(double y) {
    if constexpr (sizeof(Td) == 4) {
        return __float_as_uint((float)y);
    } else {
        constexpr double lo = sizeof(Td) == 1 ? 0.0 : -32768.0, hi = sizeof(Td) == 1 ? 255.0 : 32767.0;
        if (y != y) return 0u;
        const double r = fmin(fmax(rint(y), lo), hi);                   // ties to even; +-inf saturate
        return (unsigned)(int)r & (sizeof(Td) == 1 ? 0xffu : 0xffffu);
    }
}

template <typename Td>
__device__ __forceinline__ Td export_from_word(unsigned v) {
    if constexpr (sizeof(Td) == 4) return __uint_as_float(v);
    else return (Td)v;
}

// the aligned 32-bit word `grp` of one output row: elements e0 .. e0 + EPL - 1 of the run of hn voxels that starts at `row`
template <typename Td>
__device__ __forceinline__ void export_store_group(Td* __restrict__ row, const unsigned (*tile)[EX_T + 1], int q, int grp, int mis, int hn) {
    constexpr int EPL = 4 / (int)sizeof(Td);
    const int e0 = EPL * grp - mis;
    if (e0 >= 0 && e0 + EPL <= hn) {
        unsigned word = 0;
#pragma unroll
        for (int j = 0; j < EPL; ++j) word |= tile[e0 + j][q] << (8 * (int)sizeof(Td) * j);
        *reinterpret_cast<unsigned*>(row + e0) = word;
    } else {
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            const int e = e0 + j;
            if (e >= 0 && e < hn) row[e] = export_from_word<Td>(tile[e][q]);
        }
    }
}

// grid: (tiles of h) x (tiles of q) in x, r in y, b in z.  layout MRDIS_PREP_DHW: (q, r) = (w, d), src (D, H', W'); MRDIS_PREP_HWD: (q, r) = (d, w), src (H', W', D)
template <typename Ts, typename Td>
__global__ __launch_bounds__(EX_THREADS) void export_kernel(const Ts* __restrict__ src, ExportGeom g, const double* __restrict__ stats,
                                                            Td* __restrict__ dst, int kind, int layout, int ntq, double fill) {
    __shared__ unsigned tile[EX_T][EX_T + 1];
    const int Q = layout ? g.D : g.W;
    const int th = (int)blockIdx.x / ntq, tq = (int)blockIdx.x - th * ntq, r = (int)blockIdx.y, b = (int)blockIdx.z;
    const int hb = th * EX_T, qb = tq * EX_T;
    const int hn = min(EX_T, g.H - hb), qn = min(EX_T, Q - qb);
    const int tx = threadIdx.x & (EX_T - 1), ty = threadIdx.x / EX_T;
    double norm = 0.0, sd = 1.0;
    if (kind != MRDIS_EXPORT_COPY) {
        const double* st = stats + 5 * (size_t)b;
        const double n1 = st[0] + 1.0;
        norm = st[1] / n1;
        sd = sqrt(st[2] / n1) + 1e-8;
    }
    {
        const int q = qb + tx;
        const int d = layout ? q : r, w = (layout ? r : q) - g.w0;                  // w: in the source's frame
        const bool col_in = tx < qn && w >= 0 && w < g.Wc;                           // tx < qn keeps d < D
        const Ts* sb = src + (long long)b * g.Hc * g.Wc * g.D + (layout ? (long long)w * g.D + d : ((long long)d * g.Hc) * g.Wc + w);
        const long long sh = layout ? (long long)g.Wc * g.D : g.Wc;
        constexpr int ROWS = EX_T / (EX_THREADS / EX_T);
        Ts x[ROWS];
        bool in[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {                                             // the loads of a thread are independent and issue back to back
            const int h = hb + ty + k * (EX_THREADS / EX_T) - g.h0;                  // in the source's frame
            in[k] = col_in && h >= 0 && h < g.Hc;
            x[k] = in[k] ? sb[h * sh] : Ts(0);
        }
        const unsigned fill_word = export_convert<Td>(fill);
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            unsigned v = fill_word;
            if (in[k]) {
                if constexpr (sizeof(Ts) == 1) {                                     // a uint8 voxel is in every destination's range: COPY without float64
                    v = sizeof(Td) == 4 ? __float_as_uint((float)x[k]) : (unsigned)x[k];
                } else if (sizeof(Td) == 4 && kind == MRDIS_EXPORT_COPY) {
                    v = __float_as_uint(x[k]);                                       // fp32 -> fp32: the bits
                } else {
                    double y = (double)x[k];
                    if (kind == MRDIS_EXPORT_UNZSCORE) y = x[k] == -10.0f ? 0.0 : __dadd_rn(__dmul_rn(y, sd), norm);   // two roundings: no contraction
                    else if (kind == MRDIS_EXPORT_UNMEAN) y = __dmul_rn(y, norm);
                    v = export_convert<Td>(y);
                }
            }
            tile[ty + k * (EX_THREADS / EX_T)][tx] = v;
        }
    }
    __syncthreads();
    constexpr int EPL = 4 / (int)sizeof(Td);                                          // voxels per lane and store
    constexpr int LPR = EX_T / EPL;                                                   // lanes per row: a wave holds EPL rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // a 32-lane half holds 32 / EPL lanes of each of the wave's EPL rows (see the bank rule at the top)
    constexpr int LH = 32 / EPL;                                                      // lanes of one row in a half: banks EPL l + rw + const, l < LH, rw < EPL
    const int l = (lane & (LH - 1)) | ((lane >> 5) * LH);
    const int rw = (lane & 31) / LH;
    for (int q = wave * EPL + rw; q < qn; q += (EX_THREADS / 64) * EPL) {
        const int d = layout ? qb + q : r, w = layout ? r : qb + q;
        Td* row = dst + (((long long)b * g.D + d) * g.W + w) * g.H + hb;
        const int mis = (int)(((uintptr_t)row & 3) / sizeof(Td));
        export_store_group<Td>(row, tile, q, l, mis, hn);
        if (mis && l == 0) export_store_group<Td>(row, tile, q, LPR, mis, hn);        // the word that hangs over the end of a misaligned run
    }
}

template <typename Ts, typename Td>
void export_launch(const void* src, const ExportGeom& g, const double* stats, void* dst, int B, int kind, int layout, double fill, hipStream_t s) {
    const int nth = mrdis_cdiv(g.H, EX_T), ntq = mrdis_cdiv(layout ? g.D : g.W, EX_T);
    MRDIS_LAUNCH((export_kernel<Ts, Td>), dim3(nth * ntq, layout ? g.W : g.D, B), dim3(EX_THREADS), 0, s, (const Ts*)src, g, stats, (Td*)dst, kind,
                 layout, ntq, fill);
}

template <typename Ts>
void export_launch_dst(int dst_dtype, const void* src, const ExportGeom& g, const double* stats, void* dst, int B, int kind, int layout, double fill,
                       hipStream_t s) {
    if (dst_dtype == MRDIS_PREP_U8) export_launch<Ts, unsigned char>(src, g, stats, dst, B, kind, layout, fill, s);
    else if (dst_dtype == MRDIS_PREP_I16) export_launch<Ts, short>(src, g, stats, dst, B, kind, layout, fill, s);
    else export_launch<Ts, float>(src, g, stats, dst, B, kind, layout, fill, s);
}
}  // namespace

extern "C" int mrdis_export_volume(const void* src, int src_dtype, int layout, int Hc, int Wc, int D, int h0, int h1, int w0, int w1, int B,
                                   int kind, const double* stats, double fill, void* dst, int dst_dtype, void* stream) {
    if (!src || !dst) return MRDIS_EINVAL;
    if (src_dtype != MRDIS_PREP_U8 && src_dtype != MRDIS_PREP_F32) return MRDIS_EUNSUPPORTED;
    if (dst_dtype != MRDIS_PREP_U8 && dst_dtype != MRDIS_PREP_I16 && dst_dtype != MRDIS_PREP_F32) return MRDIS_EUNSUPPORTED;
    if (layout != MRDIS_PREP_DHW && layout != MRDIS_PREP_HWD) return MRDIS_EUNSUPPORTED;
    if (kind < MRDIS_EXPORT_COPY || kind > MRDIS_EXPORT_UNMEAN) return MRDIS_EUNSUPPORTED;
    if (src_dtype == MRDIS_PREP_U8 && kind != MRDIS_EXPORT_COPY) return MRDIS_EUNSUPPORTED;
    if (kind != MRDIS_EXPORT_COPY && !stats) return MRDIS_EUNSUPPORTED;
    if (h0 < 0 || h1 < 0 || w0 < 0 || w1 < 0 || Hc < 1 || Wc < 1 || D < 1 || D > EX_MAX_EXTENT || B < 1 || B > EX_MAX_B) return MRDIS_EUNSUPPORTED;
    const long long H = (long long)Hc + h0 + h1, W = (long long)Wc + w0 + w1;
    if (H > EX_MAX_EXTENT || W > EX_MAX_EXTENT || H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    const size_t sb = src_dtype == MRDIS_PREP_U8 ? 1 : 4, db = dst_dtype == MRDIS_PREP_U8 ? 1 : dst_dtype == MRDIS_PREP_I16 ? 2 : 4;
    if ((((uintptr_t)src) & (sb - 1)) || (((uintptr_t)dst) & (db - 1)) || (((uintptr_t)stats) & 7)) return MRDIS_EALIGN;
    ExportGeom g;
    g.H = (int)H; g.W = (int)W; g.D = D; g.Hc = Hc; g.Wc = Wc; g.h0 = h0; g.w0 = w0;
    mrdis_count(MRDIS_CNT_EXPORT);
    if (src_dtype == MRDIS_PREP_U8) export_launch_dst<unsigned char>(dst_dtype, src, g, stats, dst, B, kind, layout, fill, (hipStream_t)stream);
    else export_launch_dst<float>(dst_dtype, src, g, stats, dst, B, kind, layout, fill, (hipStream_t)stream);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
