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

// the rule of one voxel: a[c] accumulated probabilities, cv = cover of its depth, t = its (relabelled) ground-truth label
template <int C>
__device__ __forceinline__ int sv_voxel(const float* a, int cv, float t, int relabel, int (&cnt)[C][3]) {
    float best = 0.f;
    int arg = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float p = cv > 0 ? a[c] / (float)cv : 0.f;            // IEEE division; cover 0: nothing is predicted there
        const bool pp = p > 0.5f, tt = t == (float)(c + 1);         // strictly above 0.5, as mrdis_seg_counts
        cnt[c][0] += (pp && tt) ? 1 : 0; cnt[c][1] += pp ? 1 : 0; cnt[c][2] += tt ? 1 : 0;
        if (c == 0 || p > best) { best = p; arg = c; }               // lowest c on a tie
    }
    int label = best > 0.5f ? 1 + arg : 0;
    if (relabel && label == 3) label = 4;
    return label;
}

// grid (gx, B), 256 threads; P = H W D voxels per sample.  A thread takes aligned groups of four voxels of the flat (B P) volume that overlap sample b.
template <int C>
__global__ __launch_bounds__(SV_THREADS) void seg_label_kernel(const float* __restrict__ acc, const int* __restrict__ cover,
                                                               const unsigned long long* __restrict__ targets, unsigned char* __restrict__ labels,
                                                               int* __restrict__ counts, long long P, int D, int relabel) {
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
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float tk = (relabel && t[k] == 4.f) ? 3.f : t[k];
                packed |= (unsigned)sv_voxel<C>(a + k * C, cover[z], tk, relabel, cnt) << (8 * k);
                if (++z == D) z = 0;
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
                    labels[e] = (unsigned char)sv_voxel<C>(a, cover[z], tk, relabel, cnt);
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

template <int C>
void launch_seg_label(const float* acc, const int* cover, const unsigned long long* targets, unsigned char* labels, int* counts, int B, long long P,
                      int D, int relabel, hipStream_t s) {
    const int gx = sv_blocks((P + 3) / 4 + 1, SV_MAX_BLOCKS / B);
    MRDIS_LAUNCH((seg_label_kernel<C>), dim3(gx, B), dim3(SV_THREADS), 0, s, acc, cover, targets, labels, counts, P, D, relabel);
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
    switch (C) {
        case 1: launch_seg_label<1>(acc, cover, t, labels, counts, B, P, D, relabel, s); break;
        case 2: launch_seg_label<2>(acc, cover, t, labels, counts, B, P, D, relabel, s); break;
        case 3: launch_seg_label<3>(acc, cover, t, labels, counts, B, P, D, relabel, s); break;
        default: launch_seg_label<4>(acc, cover, t, labels, counts, B, P, D, relabel, s); break;
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
