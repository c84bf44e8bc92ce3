// Whole-volume sliding-window prediction of the 3-D nets (model3d.predict_volumes): overlap accumulation and the label volume.
//
// A trained net sees a depth window of Dz slices; a subject has D > Dz.  The window slides along D, the sigmoid probabilities of overlapping
// windows (and of the H-flipped input, un-flipped here) are AVERAGED, and the label of a voxel is the most probable region if that probability
// is above 0.5.  Overlap rule and label rule are this package's own convention, like the objective: the reference ships no 3-D inference.
//   mrdis_seg_accum          acc[b][h][w][z0 + k][c] += sigmoid(logits[b][h'][w][k][c])          h' = H - 1 - h if flip_h, else h
//   mrdis_seg_label_volume   pbar_c = acc_c / (float)cover[z];  counts of mrdis_seg_counts on pbar;  label = 0 | 1 + argmax_c pbar_c  (3 -> 4 if relabel)
// The torch composition (sigmoid, flip, slice +=, divide, compare, max, argmax, where, three masked sums) makes eight to ten passes over
// 57 MB-per-subject tensors for each window; here a window costs one read of the logits and one read-modify-write of its part of acc, and the
// labels and counts one read of acc and of the ground truth.
//
// Access, both kernels.  Everything is depth-and-channel fastest: a (b, h, w) column is a run of Dz C (logits) or D C (acc) contiguous floats.
// The accesses that carry most bytes are 16 bytes per lane at 16-byte aligned addresses of ACC, consecutive lanes on consecutive 16-byte groups:
//   * accum: the window of a column starts z0 C floats into the column's D C, so it is 16-byte aligned only for some (column, z0) -- at
//     BraTS's last offset 155 - 64 = 91 with C = 3 for one column in four.  A lane takes one ALIGNED group of four acc floats (a 16-byte load
//     and a 16-byte store); the four logits that belong to it sit at whatever phase the two runs differ by, and are read with one 16-byte load
//     of 4-byte alignment (global memory takes it; the lines are the same ones the neighbouring lanes read).  The first and the last group
//     of a run may be partial: those go element by element (4-byte accesses) -- the only element path, and every launch whose runs do not
//     all start and end on a group boundary takes both.  A run shorter than a group (Dz C < 4) has no vector part at all.
//   * label volume: a lane takes one aligned group of four consecutive voxels of the whole (B, H W D) volume: C aligned 16-byte loads of
//     acc, one 16-byte load of the ground truth (4-byte aligned: its phase against the group is the sample's, (b H W D) % 4), and ONE
//     32-bit store of the four labels (256 contiguous bytes per wave instruction; never a byte per lane).  The groups that straddle a
//     sample boundary (H W D % 4 != 0) are partial for either sample and go voxel by voxel with byte stores, again the only element path.
// Ownership: within a launch exactly one thread owns an acc element / a label, so windows add in launch order and two runs give the same
// bits.  Counts: thread -> wave (shuffles) -> workgroup (LDS) -> one integer atomicAdd per (workgroup, channel, count), exact in any order.
// Grid: at most SV_MAX_BLOCKS workgroups, grid-stride (cdna_hip_programming.md Guideline 11); 39 / 61 VGPRs, so a SIMD holds its 8 waves and
// the loads of the other waves cover a wave's load -> sigmoid -> store chain.  Measured at 4 x 3 x 160 x 192, Dz 64, D 155: 5.2 and 4.75 TB/s,
// 96 % and 94 % of a store-only pass over the same bytes (profiles/segvol_bench.txt).
//
// Tile-wise prediction (model3d.predict_tiles): the same two steps for tiles (TH, TW, TD) that overlap along ALL three axes, weighted by a separable
// fp32 weight and with mirrored views (the rule: include/mrdis.h).
//   mrdis_tile_accum         acc[b][h0 + i][w0 + j][d0 + k][c] = fmaf((wh[i] ww[j]) wd[k], sigmoid(logits[b][i'][j'][k'][c]), acc[...])
//   mrdis_tile_label_volume  seg_label_kernel with den = (nh[h] nw[w]) nd[d] in place of (float)cover[z]: sv_voxel takes the denominator as a float
// tile_accum keeps seg_accum's scheme: a run is now the TD C floats of a tile column inside the D C floats of an acc column, a lane owns one
// ALIGNED group of four acc floats (16-byte load and store), partial groups at a run's ends go element by element.  The logits of a view that
// does not mirror d arrive by one 16-byte load at 4-byte alignment, as in seg_accum.  A d-mirrored view reverses the voxel order inside the run
// but not the channel order, so for C < 4 no four acc floats map onto four consecutive logits: that view reads its logits with four 4-byte
// loads per lane (the same lines, each touched by the neighbouring lanes as well) -- the slower path; acc stays on 16-byte accesses.  The
// weight costs one L1-resident load of wd per voxel a group touches (two for C >= 3) and wh[i] ww[j] once per item; the item's three divisions
// (by Q, TW, TH) are a multiply and a shift each (SvDiv).  Measured at B 4, C 3, store 160 x 192 x 155, tile 128^3
// (profiles/tilepred_bench.txt): tile_accum 5.05 TB/s (4.8 d-mirrored), the tile label volume 3.95 TB/s -- 1.08 x (1.13 x) and 1.13 x the time of a
// store-only pass over the same bytes, 1.05 x and 1.19 x seg_accum / seg_label_volume: the index arithmetic and the weight loads are not free.
#include "mrdis_common.h"
#include <math.h>

namespace {
constexpr int SV_THREADS = 256;
constexpr int SV_MAX_BLOCKS = 2048;          // 256 CUs x 8 workgroups

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte access at 4-byte alignment

struct SvAccGeom { int H, W, Dz, D, C, z0, flip, ncol; };

// grid-stride over items = ncol * Q < 2^31: item = (column, aligned acc group q of the column's window).  L = Dz C floats per run.
__global__ __launch_bounds__(SV_THREADS) void seg_accum_kernel(const float* __restrict__ logits, float* __restrict__ acc, SvAccGeom g, int L, int Q) {
    const unsigned items = (unsigned)g.ncol * (unsigned)Q;
    for (unsigned i = blockIdx.x * (unsigned)SV_THREADS + threadIdx.x; i < items; i += gridDim.x * (unsigned)SV_THREADS) {
        const unsigned col = i / (unsigned)Q;
        const int q = (int)(i - col * (unsigned)Q);
        const long long s = ((long long)col * g.D + g.z0) * g.C;              // first acc float of this column's window
        const long long e0 = ((s >> 2) + q) << 2;                    // this lane's aligned group: acc floats [e0, e0 + 4)
        if (e0 >= s + L) continue;                                   // (Q is the largest group count any phase needs)
        unsigned scol = col;
        if (g.flip) {
            const unsigned bh = col / (unsigned)g.W, w = col - bh * (unsigned)g.W;
            const unsigned b = bh / (unsigned)g.H, h = bh - b * (unsigned)g.H;
            scol = (b * (unsigned)g.H + ((unsigned)g.H - 1u - h)) * (unsigned)g.W + w;
        }
        const float* src = logits + (long long)scol * L + (e0 - s);            // the logit that belongs to acc[e0] (may lie before the run for a head group)
        if (e0 >= s && e0 + 4 <= s + L) {
            const f32x4u u = *reinterpret_cast<const f32x4u*>(src);
            f32x4* dst = reinterpret_cast<f32x4*>(acc + e0);
            f32x4 a = *dst;
            a.x += mrdis_sigmoid(u.x); a.y += mrdis_sigmoid(u.y); a.z += mrdis_sigmoid(u.z); a.w += mrdis_sigmoid(u.w);
            *dst = a;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = e0 + k;
                if (e >= s && e < s + L) acc[e] += mrdis_sigmoid(src[k]);
            }
        }
    }
}

// n / d for n < 2^31 by a multiply and a shift: m = ceil(2^s / d), s = 31 + ceil(log2 d) (m < 2^32; exact for every n < 2^31).  The host forms
// it once per launch; the three runtime divisions of an item (by Q, TW, TH) were a third of its instructions.
struct SvDiv { unsigned m; int s; };
SvDiv sv_div(unsigned d) {
    int l = 0;
    while ((1u << l) < d) ++l;
    SvDiv r;
    r.s = 31 + l;
    r.m = (unsigned)((((unsigned long long)1 << r.s) + d - 1) / d);
    return r;
}
__device__ __forceinline__ unsigned sv_quot(unsigned n, SvDiv d) { return (unsigned)(((unsigned long long)n * d.m) >> d.s); }

struct SvTileGeom { int H, W, D, TH, TW, TD, h0, w0, d0, fh, fw, ncol; SvDiv dq, dtw, dth; };

// grid-stride over items = ncol * Q < 2^31: item = (tile column (b, i, j), aligned acc group q of the column's run).  L = TD C floats per run.
// FD: the view mirrors d -- acc voxel k of the run reads logit voxel TD - 1 - k, element loads.
template <int C, bool FD>
__global__ __launch_bounds__(SV_THREADS) void tile_accum_kernel(const float* __restrict__ logits, float* __restrict__ acc, const float* __restrict__ wh,
                                                                const float* __restrict__ ww, const float* __restrict__ wd, SvTileGeom g, int L, int Q) {
    constexpr int NV = C == 1 ? 4 : (C == 2 ? 3 : 2);                // voxels four consecutive floats can touch
    const unsigned items = (unsigned)g.ncol * (unsigned)Q;
    for (unsigned it = blockIdx.x * (unsigned)SV_THREADS + threadIdx.x; it < items; it += gridDim.x * (unsigned)SV_THREADS) {
        const unsigned col = sv_quot(it, g.dq);
        const int q = (int)(it - col * (unsigned)Q);
        const unsigned bi = sv_quot(col, g.dtw), j = col - bi * (unsigned)g.TW;
        const unsigned b = sv_quot(bi, g.dth), i = bi - b * (unsigned)g.TH;
        const long long acol = ((long long)b * g.H + (g.h0 + (int)i)) * g.W + (g.w0 + (int)j);
        const long long s = (acol * g.D + g.d0) * C;                 // first acc float of this column's run
        const long long e0 = ((s >> 2) + q) << 2;                    // this lane's aligned group: acc floats [e0, e0 + 4)
        if (e0 >= s + L) continue;                                   // (Q is the largest group count any phase needs)
        const unsigned si = g.fh ? (unsigned)g.TH - 1u - i : i, sj = g.fw ? (unsigned)g.TW - 1u - j : j;
        const float* src = logits + (long long)((b * (unsigned)g.TH + si) * (unsigned)g.TW + sj) * L;          // the source run: the weight stays at (i, j)
        const float whw = wh[i] * ww[j];                             // first rounding of the weight
        const int t0 = (int)(e0 - s);                                // run position of acc[e0] (negative for a head group)
        if (t0 >= 0 && t0 + 4 <= L) {
            const int k0 = t0 / C, c0 = t0 - k0 * C;
            float wk[NV];                                            // one load of wd per voxel the group touches (the last may lie past the group: clamped)
#pragma unroll
            for (int v = 0; v < NV; ++v) wk[v] = whw * wd[min(k0 + v, g.TD - 1)];      // second rounding
            float u[4], w[4];
            if (!FD) {
                const f32x4u x = *reinterpret_cast<const f32x4u*>(src + t0);
                u[0] = x.x; u[1] = x.y; u[2] = x.z; u[3] = x.w;
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int v = (c0 + m) / C;                          // voxel of element m, counted from k0: below NV
                if (FD) u[m] = src[(g.TD - 1 - k0 - v) * C + (c0 + m - v * C)];
                float x = wk[0];
#pragma unroll
                for (int n = 1; n < NV; ++n) x = v >= n ? wk[n] : x;
                w[m] = x;
            }
            f32x4* dst = reinterpret_cast<f32x4*>(acc + e0);
            f32x4 a = *dst;
            a.x = fmaf(w[0], mrdis_sigmoid(u[0]), a.x); a.y = fmaf(w[1], mrdis_sigmoid(u[1]), a.y);
            a.z = fmaf(w[2], mrdis_sigmoid(u[2]), a.z); a.w = fmaf(w[3], mrdis_sigmoid(u[3]), a.w);
            *dst = a;
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int t = t0 + m;
                if (t >= 0 && t < L) {
                    const int k = t / C, c = t - k * C;
                    const float u = src[(FD ? g.TD - 1 - k : k) * C + c];
                    acc[e0 + m] = fmaf(whw * wd[k], mrdis_sigmoid(u), acc[e0 + m]);
                }
            }
        }
    }
}

// the rule of one voxel: a[c] accumulated probabilities, den = the summed weight of its accumulations (sliding window: the cover of its depth,
// exact in fp32), t = its (relabelled) ground-truth label
template <int C>
__device__ __forceinline__ int sv_voxel(const float* a, float den, float t, int relabel, int (&cnt)[C][3]) {
    float best = 0.f;
    int arg = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float p = den > 0.f ? a[c] / den : 0.f;               // IEEE division; nothing accumulated: nothing is predicted there
        const bool pp = p > 0.5f, tt = t == (float)(c + 1);         // strictly above 0.5, as mrdis_seg_counts
        cnt[c][0] += (pp && tt) ? 1 : 0; cnt[c][1] += pp ? 1 : 0; cnt[c][2] += tt ? 1 : 0;
        if (c == 0 || p > best) { best = p; arg = c; }               // lowest c on a tie
    }
    int label = best > 0.5f ? 1 + arg : 0;
    if (relabel && label == 3) label = 4;
    return label;
}

// The denominator of a voxel.  SvCover: (float)cover[z] of the sliding window, no state.  SvNorms: (nh[h] nw[w]) nd[z] of the tiles, two fp32
// roundings; its state is the column (h, w) with the first product: one division per group of four voxels, a step where a column ends inside it.
struct SvCover {
    const int* cover;
    struct St {};
    __device__ __forceinline__ St start(int, int) const { return St{}; }
    __device__ __forceinline__ void next(St&, int) const {}
    __device__ __forceinline__ float at(const St&, int z) const { return (float)cover[z]; }
};
struct SvNorms {
    const float *nh, *nw, *nd;
    struct St { int h, w; float hw; };
    __device__ __forceinline__ St start(int col, int W) const { St s; s.h = col / W; s.w = col - s.h * W; s.hw = nh[s.h] * nw[s.w]; return s; }
    __device__ __forceinline__ void next(St& s, int W) const { if (++s.w == W) { s.w = 0; ++s.h; } s.hw = nh[s.h] * nw[s.w]; }
    __device__ __forceinline__ float at(const St& s, int z) const { return s.hw * nd[z]; }
};

// grid (gx, B), 256 threads; P = H W D voxels per sample.  A thread takes aligned groups of four voxels of the flat (B P) volume that overlap sample b.
template <int C, typename Den>
__global__ __launch_bounds__(SV_THREADS) void seg_label_kernel(const float* __restrict__ acc, Den den,
                                                               const unsigned long long* __restrict__ targets, unsigned char* __restrict__ labels,
                                                               int* __restrict__ counts, long long P, int D, int W, int relabel) {
    __shared__ int red[SV_THREADS / 64][3 * C];
    const int b = blockIdx.y;
    const long long v0 = (long long)b * P, v1 = v0 + P;             // this sample's voxels of the flat volume
    const float* tgt = targets != nullptr ? reinterpret_cast<const float*>(targets[b]) : nullptr;
    int cnt[C][3];
#pragma unroll
    for (int c = 0; c < C; ++c) { cnt[c][0] = 0; cnt[c][1] = 0; cnt[c][2] = 0; }
    const long long g0 = v0 >> 2, ngrp = ((v1 + 3) >> 2) - g0;
    for (long long gi = blockIdx.x * (long long)SV_THREADS + threadIdx.x; gi < ngrp; gi += gridDim.x * (long long)SV_THREADS) {
        const long long e0 = (g0 + gi) << 2;                         // flat voxels [e0, e0 + 4)
        int z = (int)(e0 - v0) % D;                                  // depth of voxel e0 (of the previous sample's tail if e0 < v0: then unused)
        if (z < 0) z += D;
        if (e0 >= v0 && e0 + 4 <= v1) {
            float a[4 * C];
            const f32x4* a4 = reinterpret_cast<const f32x4*>(acc + e0 * C);
#pragma unroll
            for (int j = 0; j < C; ++j) { const f32x4 r = a4[j]; a[4 * j] = r.x; a[4 * j + 1] = r.y; a[4 * j + 2] = r.z; a[4 * j + 3] = r.w; }
            f32x4u t4 = {0.f, 0.f, 0.f, 0.f};
            if (tgt != nullptr) t4 = *reinterpret_cast<const f32x4u*>(tgt + (e0 - v0));
            const float t[4] = {t4.x, t4.y, t4.z, t4.w};
            unsigned packed = 0;
            typename Den::St st = den.start((int)(e0 - v0) / D, W);   // column of voxel e0 in its sample: all four voxels lie inside it
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float tk = (relabel && t[k] == 4.f) ? 3.f : t[k];
                packed |= (unsigned)sv_voxel<C>(a + k * C, den.at(st, z), tk, relabel, cnt) << (8 * k);
                if (++z == D) { z = 0; if (k < 3) den.next(st, W); }  // (after the last voxel the next column may not exist)
            }
            *reinterpret_cast<unsigned*>(labels + e0) = packed;
        } else {
            for (int k = 0; k < 4; ++k) {
                const long long e = e0 + k;
                if (e >= v0 && e < v1) {
                    float a[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) a[c] = acc[e * C + c];
                    float tk = tgt != nullptr ? tgt[e - v0] : 0.f;
                    if (relabel && tk == 4.f) tk = 3.f;
                    labels[e] = (unsigned char)sv_voxel<C>(a, den.at(den.start((int)(e - v0) / D, W), z), tk, relabel, cnt);
                }
                if (++z == D) z = 0;
            }
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
        if (v != 0) atomicAdd(counts + (long long)b * 3 * C + threadIdx.x, v);
    }
}

int sv_blocks(long long items, long long cap) {
    long long nb = (items + SV_THREADS - 1) / SV_THREADS;
    if (cap < 1) cap = 1;
    return nb < 1 ? 1 : (nb > cap ? (int)cap : (int)nb);
}

template <int C, typename Den>
void launch_seg_label(const float* acc, Den den, const unsigned long long* targets, unsigned char* labels, int* counts, int B, long long P,
                      int D, int W, int relabel, hipStream_t s) {
    const int gx = sv_blocks((P + 3) / 4 + 1, SV_MAX_BLOCKS / B);
    MRDIS_LAUNCH((seg_label_kernel<C, Den>), dim3(gx, B), dim3(SV_THREADS), 0, s, acc, den, targets, labels, counts, P, D, W, relabel);
}

template <typename Den>
void launch_seg_label_c(int C, const float* acc, Den den, const unsigned long long* t, unsigned char* labels, int* counts, int B, long long P, int D,
                        int W, int relabel, hipStream_t s) {
    switch (C) {
        case 1: launch_seg_label<1>(acc, den, t, labels, counts, B, P, D, W, relabel, s); break;
        case 2: launch_seg_label<2>(acc, den, t, labels, counts, B, P, D, W, relabel, s); break;
        case 3: launch_seg_label<3>(acc, den, t, labels, counts, B, P, D, W, relabel, s); break;
        default: launch_seg_label<4>(acc, den, t, labels, counts, B, P, D, W, relabel, s); break;
    }
}

template <int C>
void launch_tile_accum(bool fd, int blocks, hipStream_t s, const float* logits, float* acc, const float* wh, const float* ww, const float* wd,
                       const SvTileGeom& g, int L, int Q) {
    if (fd) MRDIS_LAUNCH((tile_accum_kernel<C, true>), dim3(blocks), dim3(SV_THREADS), 0, s, logits, acc, wh, ww, wd, g, L, Q);
    else MRDIS_LAUNCH((tile_accum_kernel<C, false>), dim3(blocks), dim3(SV_THREADS), 0, s, logits, acc, wh, ww, wd, g, L, Q);
}
}  // namespace

extern "C" int mrdis_seg_accum(const float* logits, float* acc, int B, int H, int W, int Dz, int D, int C, int z0, int flip_h, void* stream) {
    if (!logits || !acc || B < 1 || H < 1 || W < 1 || Dz < 1 || D < Dz || C < 1 || C > 4 || z0 < 0 || z0 > D - Dz) return MRDIS_EINVAL;
    if ((((uintptr_t)acc) & 15) != 0 || (((uintptr_t)logits) & 3) != 0) return MRDIS_EALIGN;
    SvAccGeom g;
    const int L = Dz * C, Q = (L + 6) >> 2;                          // groups a run of L floats overlaps at the worst phase (3)
    if ((long long)B * H * W * Q >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    g.H = H; g.W = W; g.Dz = Dz; g.D = D; g.C = C; g.z0 = z0; g.flip = flip_h ? 1 : 0; g.ncol = B * H * W;
    mrdis_count(MRDIS_CNT_SEGACCUM);
    MRDIS_LAUNCH(seg_accum_kernel, dim3(sv_blocks((long long)g.ncol * Q, SV_MAX_BLOCKS)), dim3(SV_THREADS), 0, (hipStream_t)stream, logits, acc, g, L, Q);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_seg_label_volume(const float* acc, const int* cover, const void* targets, unsigned char* labels, int* counts, int B, int H,
                                      int W, int D, int C, int relabel, void* stream) {
    if (!acc || !cover || !labels || !counts || B < 1 || H < 1 || W < 1 || D < 1 || C < 1 || C > 4) return MRDIS_EINVAL;
    if (B > 65535 || (long long)H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    if ((((uintptr_t)acc) & 15) != 0 || ((((uintptr_t)labels) | ((uintptr_t)cover) | ((uintptr_t)counts)) & 3) != 0 || (((uintptr_t)targets) & 7) != 0)
        return MRDIS_EALIGN;
    const long long P = (long long)H * W * D;
    const unsigned long long* t = reinterpret_cast<const unsigned long long*>(targets);
    hipStream_t s = (hipStream_t)stream;
    mrdis_count(MRDIS_CNT_SEGLABELS);
    launch_seg_label_c(C, acc, SvCover{cover}, t, labels, counts, B, P, D, W, relabel, s);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_tile_accum(const float* logits, float* acc, const float* wh, const float* ww, const float* wd, int B, int H, int W, int D, int TH,
                                int TW, int TD, int C, int h0, int w0, int d0, int flips, void* stream) {
    if (!logits || !acc || !wh || !ww || !wd || B < 1 || TH < 1 || TW < 1 || TD < 1 || H < TH || W < TW || D < TD || C < 1 || C > 4) return MRDIS_EINVAL;
    if (h0 < 0 || h0 > H - TH || w0 < 0 || w0 > W - TW || d0 < 0 || d0 > D - TD || (flips & ~(1 | 4 | 8)) != 0) return MRDIS_EINVAL;
    if ((((uintptr_t)acc) & 15) != 0 || ((((uintptr_t)logits) | ((uintptr_t)wh) | ((uintptr_t)ww) | ((uintptr_t)wd)) & 3) != 0) return MRDIS_EALIGN;
    const int L = TD * C, Q = (L + 6) >> 2;                          // groups a run of L floats overlaps at the worst phase (3)
    if ((long long)B * TH * TW * Q >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    SvTileGeom g;
    g.H = H; g.W = W; g.D = D; g.TH = TH; g.TW = TW; g.TD = TD; g.h0 = h0; g.w0 = w0; g.d0 = d0; g.fh = flips & 1; g.fw = (flips >> 2) & 1;
    g.ncol = B * TH * TW; g.dq = sv_div((unsigned)Q); g.dtw = sv_div((unsigned)TW); g.dth = sv_div((unsigned)TH);
    const int blocks = sv_blocks((long long)g.ncol * Q, SV_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    const bool fd = (flips & 8) != 0;
    mrdis_count(MRDIS_CNT_TILEACCUM);
    switch (C) {
        case 1: launch_tile_accum<1>(fd, blocks, s, logits, acc, wh, ww, wd, g, L, Q); break;
        case 2: launch_tile_accum<2>(fd, blocks, s, logits, acc, wh, ww, wd, g, L, Q); break;
        case 3: launch_tile_accum<3>(fd, blocks, s, logits, acc, wh, ww, wd, g, L, Q); break;
        default: launch_tile_accum<4>(fd, blocks, s, logits, acc, wh, ww, wd, g, L, Q); break;
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_tile_label_volume(const float* acc, const float* nh, const float* nw, const float* nd, const void* targets, unsigned char* labels,
                                       int* counts, int B, int H, int W, int D, int C, int relabel, void* stream) {
    if (!acc || !nh || !nw || !nd || !labels || !counts || B < 1 || H < 1 || W < 1 || D < 1 || C < 1 || C > 4) return MRDIS_EINVAL;
    if (B > 65535 || (long long)H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    if ((((uintptr_t)acc) & 15) != 0 || (((uintptr_t)targets) & 7) != 0 ||
        ((((uintptr_t)labels) | ((uintptr_t)nh) | ((uintptr_t)nw) | ((uintptr_t)nd) | ((uintptr_t)counts)) & 3) != 0)
        return MRDIS_EALIGN;
    const long long P = (long long)H * W * D;
    mrdis_count(MRDIS_CNT_TILELABELS);
    launch_seg_label_c(C, acc, SvNorms{nh, nw, nd}, reinterpret_cast<const unsigned long long*>(targets), labels, counts, B, P, D, W, relabel,
                       (hipStream_t)stream);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
