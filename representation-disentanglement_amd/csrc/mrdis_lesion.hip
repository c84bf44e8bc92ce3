// Lesion-wise scoring of label volumes (lesion.lesion_scores): region membership planes, binary dilation, the matching of predicted components
// to dilated ground-truth lesions and the expansion of the matched sets into per-lesion masks.  Integer arithmetic and integer atomics only:
// exact, and the same bits from run to run.  Volumes are (B, H, W, D) with D contiguous, as mrdis_seg_label_volume writes its labels.
//
//   mrdis_region_planes   planes bit r = the voxel lies in predicted region r, bit 4 + r = in ground-truth region r: the membership that
//                         mrdis_region_surfaces decides (mrdis_region_nib, mrdis_device.h), without the surface rule.  ONE launch.
//   mrdis_dilate          dst = src dilated `iterations` times by the 6 / 18 / 26 neighbourhood, every BIT of a byte on its own (the OR of that
//                         bit over the neighbourhood), so all regions of the planes dilate in one pass.  ONE LAUNCH PER ITERATION, each with a
//                         halo of one voxel: iteration i reads what iteration i - 1 wrote (src -> dst for one iteration, ping-pong between dst
//                         and the workspace for more, the last one landing in dst).  A halo of n voxels in one launch would stage
//                         (8 + 2n)(8 + 2n)(64 + 2n) bytes per 8 x 8 x 64 tile, 3.3x the tile at n = 3, to save passes that move one byte per
//                         voxel each way; the chain of launches keeps one kernel and one halo.
//                         Counter "dilate": one per launch of either entry point (1 per mrdis_region_planes call, `iterations` per mrdis_dilate call).
//   mrdis_lesion_match    per voxel: bit (lesion j, component k) of a bit matrix by atomicOr where a predicted voxel lies in a dilated lesion,
//                         |T_L| by atomicAdd, the lesion's root voxel and item by a plain store of its one root voxel.  ONE launch ("lesmatch").
//   mrdis_lesion_expand   the 0/1 masks T_L and S_L of a chunk of lesions, (n, H, W, D) uint8 each.  ONE launch ("lesexpand").
//
// dilate_kernel.  A workgroup owns a tile of 8 x 8 x 64 voxels and stages it with a halo of one voxel (one 32-bit WORD = four voxels along D)
// in LDS as words: 10 x 10 lines of 18 words.  The three-wide OR along D is word arithmetic -- c | c << 8 | c >> 8 with the end bytes of the
// neighbouring words carried in -- kept in a second LDS array (10 x 10 x 16 words); an output word is then the OR of
//   6:  d3(h, w) | c(h +- 1, w) | c(h, w +- 1)          18:  d3 of the centre and its four face lines | c of the four diagonal lines
//   26: d3 of all nine lines.
// A lane loads and stores four consecutive voxels of a line as one dword at whatever alignment the line has (D need not be a multiple of four;
// the hardware takes an unaligned dword); only a line's last partial word goes byte by byte.  Everything beyond the volume reads as 0: nothing
// wraps around a border or crosses into another sample (every voxel is addressed by coordinates that are checked against H, W, D).
//
// No workgroup waits for another, the launches of a call do not depend on the volumes' content, and no order ever comes from an atomic: dense
// lesion and component numbers are ranks of root indices, made by the caller's scan.
#include "mrdis_common.h"

namespace {
constexpr int LS_THREADS = 256;
constexpr int LS_MAX_BLOCKS = 2048;          // 256 CUs x 8 workgroups, for the grid-stride passes
constexpr int LS_MAX_EXTENT = 1024;
constexpr int DL_TH = 8, DL_TW = 8, DL_TK = 16;                  // the tile: 8 x 8 lines of 16 words = 64 voxels
constexpr int DL_LH = DL_TH + 2, DL_LW = DL_TW + 2, DL_LK = DL_TK + 2;
static_assert(DL_TH * DL_TW * DL_TK == 4 * LS_THREADS, "four output words per thread");

bool ls_geometry_ok(int B, int H, int W, int D) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || D < 1 || H > LS_MAX_EXTENT || W > LS_MAX_EXTENT || D > LS_MAX_EXTENT) return false;
    return (long long)H * W * D < (1LL << 31);
}
unsigned ls_stride_blocks(long long items, long long rows) {
    long long nb = (items + LS_THREADS - 1) / LS_THREADS, cap = LS_MAX_BLOCKS / rows;
    if (cap < 1) cap = 1;
    return (unsigned)(nb > cap ? cap : (nb < 1 ? 1 : nb));
}

// ---------------------------------------------------------------------------------------------- region planes
// grid (gx, B).  A thread takes aligned groups of four voxels of the flat (B P) volume that overlap sample b (the grouping of region_surfaces_kernel).
__global__ __launch_bounds__(LS_THREADS) void region_planes_kernel(const unsigned char* __restrict__ labels, const unsigned long long* __restrict__ targets,
                                                                   unsigned char* __restrict__ planes, long long P, unsigned lut) {
    const int b = blockIdx.y;
    const long long v0 = (long long)b * P, v1 = v0 + P;
    const float* tgt = targets != nullptr ? reinterpret_cast<const float*>(targets[b]) : nullptr;
    const long long g0 = v0 >> 2, ngrp = ((v1 + 3) >> 2) - g0;
    for (long long gi = blockIdx.x * (long long)LS_THREADS + threadIdx.x; gi < ngrp; gi += gridDim.x * (long long)LS_THREADS) {
        const long long e0 = (g0 + gi) << 2;
        if (e0 >= v0 && e0 + 4 <= v1) {
            const unsigned l4 = *reinterpret_cast<const unsigned*>(labels + e0);
            unsigned packed = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) packed |= mrdis_region_nib((unsigned char)((l4 >> (8 * k)) & 255u), lut) << (8 * k);
            if (tgt != nullptr) {
                const f32x4u t4 = *reinterpret_cast<const f32x4u*>(tgt + (e0 - v0));
                packed |= (mrdis_region_nib(t4.x, lut) << 4) | (mrdis_region_nib(t4.y, lut) << 12) | (mrdis_region_nib(t4.z, lut) << 20) |
                          (mrdis_region_nib(t4.w, lut) << 28);
            }
            *reinterpret_cast<unsigned*>(planes + e0) = packed;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = e0 + k;
                if (e < v0 || e >= v1) continue;
                unsigned n = mrdis_region_nib(labels[e], lut);
                if (tgt != nullptr) n |= mrdis_region_nib(tgt[e - v0], lut) << 4;
                planes[e] = (unsigned char)n;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- dilation, one iteration
struct DlGeom { int H, W, D, tw, tk, conn; long long P; };

// grid (tiles, B), 256 threads
__global__ __launch_bounds__(LS_THREADS) void dilate_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, DlGeom g) {
    __shared__ unsigned raw[DL_LH * DL_LW][DL_LK];                // the tile and its halo, four voxels per word
    __shared__ unsigned d3[DL_LH * DL_LW][DL_TK];                 // the OR of each voxel with its two neighbours along D
    const int t = blockIdx.x;
    const int per_h = g.tw * g.tk;
    const int th = t / per_h, rem = t - th * per_h;
    const int tw = rem / g.tk;
    const int h0 = th * DL_TH, w0 = tw * DL_TW, d0 = (rem - tw * g.tk) * (4 * DL_TK);
    const long long base = (long long)blockIdx.y * g.P;
    for (int idx = threadIdx.x; idx < DL_LH * DL_LW * DL_LK; idx += LS_THREADS) {
        const int line = idx / DL_LK, kk = idx - line * DL_LK;
        const int hh = line / DL_LW, ww = line - hh * DL_LW;
        const int h = h0 - 1 + hh, w = w0 - 1 + ww, d = d0 - 4 + 4 * kk;
        unsigned word = 0u;
        if (h >= 0 && h < g.H && w >= 0 && w < g.W && d + 4 > 0 && d < g.D) {
            const unsigned char* p = src + base + ((long long)h * g.W + w) * g.D;
            if (d >= 0 && d + 4 <= g.D) {
                word = *reinterpret_cast<const u32u1*>(p + d);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (d + i >= 0 && d + i < g.D) word |= (unsigned)p[d + i] << (8 * i);
            }
        }
        raw[line][kk] = word;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < DL_LH * DL_LW * DL_TK; idx += LS_THREADS) {
        const int line = idx / DL_TK, k = idx - line * DL_TK;
        const unsigned l = raw[line][k], c = raw[line][k + 1], r = raw[line][k + 2];
        d3[line][k] = c | (c << 8) | (l >> 24) | (c >> 8) | (r << 24);
    }
    __syncthreads();
    const int k = threadIdx.x & (DL_TK - 1);
#pragma unroll
    for (int rnd = 0; rnd < 4; ++rnd) {
        const int li = rnd * (LS_THREADS / DL_TK) + (threadIdx.x >> 4);      // 0 .. 63: the line of the tile
        const int lh = li / DL_TW, lw = li - lh * DL_TW;
        const int c = (lh + 1) * DL_LW + (lw + 1);                           // its line in LDS
        unsigned out = d3[c][k];
        if (g.conn == 6) {
            out |= raw[c - DL_LW][k + 1] | raw[c + DL_LW][k + 1] | raw[c - 1][k + 1] | raw[c + 1][k + 1];
        } else {
            out |= d3[c - DL_LW][k] | d3[c + DL_LW][k] | d3[c - 1][k] | d3[c + 1][k];
            if (g.conn == 18) out |= raw[c - DL_LW - 1][k + 1] | raw[c - DL_LW + 1][k + 1] | raw[c + DL_LW - 1][k + 1] | raw[c + DL_LW + 1][k + 1];
            else out |= d3[c - DL_LW - 1][k] | d3[c - DL_LW + 1][k] | d3[c + DL_LW - 1][k] | d3[c + DL_LW + 1][k];
        }
        const int h = h0 + lh, w = w0 + lw, d = d0 + 4 * k;
        if (h >= g.H || w >= g.W || d >= g.D) continue;
        unsigned char* p = dst + base + ((long long)h * g.W + w) * g.D;
        if (d + 4 <= g.D) {
            *reinterpret_cast<u32u1*>(p + d) = out;
        } else {
            for (int i = 0; d + i < g.D; ++i) p[d + i] = (unsigned char)((out >> (8 * i)) & 255u);
        }
    }
}

// ---------------------------------------------------------------------------------------------- matching
struct LsGeom {
    int R, items;           // regions; items = B R, item = b R + r
    int words;              // 32-bit words of a row of the bit matrix
    int n_lesions;
    long long P;
};

// grid (gx, B R), grid-stride over the voxels of item (b, r).  comp_* (B R, P): canonical component ids of the dilated ground truth (l) and of the
// prediction (p), -1 on background; rank_* (B R, P): at a ROOT voxel the dense number of its component over the whole call, in (item, root) order;
// first_p (B R): the dense number of the item's first predicted component.
__global__ __launch_bounds__(LS_THREADS) void lesion_match_kernel(const unsigned char* __restrict__ planes, const int* __restrict__ comp_l,
                                                                  const int* __restrict__ rank_l, const int* __restrict__ comp_p,
                                                                  const int* __restrict__ rank_p, const int* __restrict__ first_p, int* bits,
                                                                  int* tcount, int* __restrict__ root, int* __restrict__ item, LsGeom g) {
    const int it = blockIdx.y;
    const int b = it / g.R, r = it - b * g.R;
    const long long ibase = (long long)it * g.P;
    const unsigned char* pl = planes + (long long)b * g.P;
    const int kfirst = first_p[it];
    const int lane = threadIdx.x & 63;
    for (long long i0 = (long long)blockIdx.x * LS_THREADS; i0 < g.P; i0 += (long long)gridDim.x * LS_THREADS) {      // (the trip count is uniform over the workgroup)
        const long long v = i0 + threadIdx.x;
        int j = -1, k = -1;
        bool tvox = false;
        if (v < g.P) {
            const int cl = comp_l[ibase + v];
            if (cl >= 0 && cl < g.P) {
                j = rank_l[ibase + cl];
                if (j < 0 || j >= g.n_lesions) j = -1;               // (a rank the caller's scan did not make: touch nothing)
            }
            if (j >= 0) {
                if ((long long)cl == v) { root[j] = cl; item[j] = it; }      // the lesion's one root voxel
                tvox = ((pl[v] >> (4 + r)) & 1u) != 0u;
                const int cp = comp_p[ibase + v];
                if (cp >= 0 && cp < g.P) {
                    k = rank_p[ibase + cp] - kfirst;
                    if (k < 0 || k >= 32 * g.words) k = -1;
                }
            }
        }
        // |T_L|: one add per distinct lesion of the wave
        unsigned long long todo = __builtin_amdgcn_ballot_w64(tvox);
        while (todo != 0ull) {
            const int leader = __builtin_ctzll(todo);
            const int jl = __shfl(j, leader, 64);
            const unsigned long long same = __builtin_amdgcn_ballot_w64(tvox && j == jl);
            if (lane == leader) atomicAdd(tcount + jl, (int)__builtin_popcountll(same));
            todo &= ~same;
        }
        // bit (j, k): one OR per distinct pair of the wave, and none where the bit is already seen set (a stale read only costs an atomic)
        todo = __builtin_amdgcn_ballot_w64(k >= 0);
        while (todo != 0ull) {
            const int leader = __builtin_ctzll(todo);
            const int jl = __shfl(j, leader, 64), kl = __shfl(k, leader, 64);
            const unsigned long long same = __builtin_amdgcn_ballot_w64(k >= 0 && j == jl && k == kl);
            if (lane == leader) {
                int* word = bits + (long long)jl * g.words + (kl >> 5);
                const int bit = (int)(1u << (kl & 31));
                if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0) atomicOr(word, bit);
            }
            todo &= ~same;
        }
    }
}

// ---------------------------------------------------------------------------------------------- expansion
// grid (gx, n): row jl of the two stacks is lesion j0 + jl.  A thread takes aligned groups of four voxels of the flat (n P) stacks that overlap row jl.
__global__ __launch_bounds__(LS_THREADS) void lesion_expand_kernel(const unsigned char* __restrict__ planes, const int* __restrict__ comp_l,
                                                                   const int* __restrict__ rank_l, const int* __restrict__ comp_p,
                                                                   const int* __restrict__ rank_p, const int* __restrict__ first_p,
                                                                   const int* __restrict__ bits, const int* __restrict__ item, int j0,
                                                                   unsigned char* __restrict__ stack_s, unsigned char* __restrict__ stack_t, LsGeom g) {
    const int jl = blockIdx.y, j = j0 + jl;
    int it = item[j];
    const bool known = it >= 0 && it < g.items;                       // (an item the match did not write: the row is written as zeros)
    if (!known) it = 0;
    const int b = it / g.R, r = it - b * g.R;
    const long long ibase = (long long)it * g.P;
    const unsigned char* pl = planes + (long long)b * g.P;
    const int* row = bits + (long long)j * g.words;
    const int kfirst = first_p[it];
    const long long v0 = (long long)jl * g.P, v1 = v0 + g.P;
    const long long g0 = v0 >> 2, ngrp = ((v1 + 3) >> 2) - g0;
    for (long long gi = blockIdx.x * (long long)LS_THREADS + threadIdx.x; gi < ngrp; gi += gridDim.x * (long long)LS_THREADS) {
        const long long e0 = (g0 + gi) << 2;
        const bool whole = e0 >= v0 && e0 + 4 <= v1;
        int cl[4] = {-1, -1, -1, -1}, cp[4] = {-1, -1, -1, -1};
        if (whole && known) {
            const i32x4u a = *reinterpret_cast<const i32x4u*>(comp_l + ibase + (e0 - v0));
            const i32x4u c = *reinterpret_cast<const i32x4u*>(comp_p + ibase + (e0 - v0));
            cl[0] = a.x; cl[1] = a.y; cl[2] = a.z; cl[3] = a.w;
            cp[0] = c.x; cp[1] = c.y; cp[2] = c.z; cp[3] = c.w;
        } else if (known) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long e = e0 + q;
                if (e >= v0 && e < v1) { cl[q] = comp_l[ibase + (e - v0)]; cp[q] = comp_p[ibase + (e - v0)]; }
            }
        }
        unsigned ps = 0u, pt = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long v = e0 + q - v0;
            if (cl[q] >= 0 && cl[q] < g.P && ((pl[v] >> (4 + r)) & 1u) != 0u && rank_l[ibase + cl[q]] == j) pt |= 1u << (8 * q);
            if (cp[q] >= 0 && cp[q] < g.P) {
                const int k = rank_p[ibase + cp[q]] - kfirst;
                if (k >= 0 && k < 32 * g.words && (((unsigned)row[k >> 5] >> (k & 31)) & 1u) != 0u) ps |= 1u << (8 * q);
            }
        }
        if (whole) {
            *reinterpret_cast<unsigned*>(stack_s + e0) = ps;
            *reinterpret_cast<unsigned*>(stack_t + e0) = pt;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long e = e0 + q;
                if (e >= v0 && e < v1) {
                    stack_s[e] = (unsigned char)((ps >> (8 * q)) & 255u);
                    stack_t[e] = (unsigned char)((pt >> (8 * q)) & 255u);
                }
            }
        }
    }
}
}  // namespace

extern "C" int mrdis_region_planes(const unsigned char* labels, const void* targets, const int* region_masks, int R, unsigned char* planes, int B,
                                   int H, int W, int D, void* stream) {
    if (!ls_geometry_ok(B, H, W, D)) return MRDIS_EUNSUPPORTED;
    if (!labels || !region_masks || !planes || R < 1 || R > MRDIS_SURF_MAX_REGIONS) return MRDIS_EINVAL;
    if (((((uintptr_t)labels) | ((uintptr_t)planes)) & 3) != 0 || (((uintptr_t)targets) & 7) != 0) return MRDIS_EALIGN;
    unsigned lut = 0u;                                               // nibble l: the regions that hold label l
    for (int r = 0; r < R; ++r) {
        if (region_masks[r] < 0 || region_masks[r] > 255) return MRDIS_EINVAL;
        for (int l = 0; l < 8; ++l)
            if ((region_masks[r] >> l) & 1) lut |= 1u << (4 * l + r);
    }
    const long long P = (long long)H * W * D;
    mrdis_count(MRDIS_CNT_DILATE);
    MRDIS_LAUNCH(region_planes_kernel, dim3(ls_stride_blocks((P + 3) / 4 + 1, B), B), dim3(LS_THREADS), 0, (hipStream_t)stream, labels,
                 reinterpret_cast<const unsigned long long*>(targets), planes, P, lut);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" size_t mrdis_dilate_workspace(int iterations, int B, int H, int W, int D) {
    if (iterations < 1 || iterations > MRDIS_DILATE_MAX_ITERATIONS || !ls_geometry_ok(B, H, W, D)) return 0;
    return iterations >= 2 ? (size_t)B * H * W * D : 0;
}

extern "C" int mrdis_dilate(const unsigned char* src, unsigned char* dst, int connectivity, int iterations, void* workspace, size_t workspace_bytes,
                            int B, int H, int W, int D, void* stream) {
    if (!ls_geometry_ok(B, H, W, D)) return MRDIS_EUNSUPPORTED;
    if (!src || !dst || src == dst || iterations < 1 || iterations > MRDIS_DILATE_MAX_ITERATIONS) return MRDIS_EINVAL;
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return MRDIS_EINVAL;
    if (iterations >= 2 && (!workspace || workspace_bytes < mrdis_dilate_workspace(iterations, B, H, W, D))) return MRDIS_EWORKSPACE;
    DlGeom g;
    g.H = H; g.W = W; g.D = D; g.P = (long long)H * W * D; g.conn = connectivity;
    g.tw = mrdis_cdiv(W, DL_TW); g.tk = mrdis_cdiv(D, 4 * DL_TK);
    const unsigned tiles = (unsigned)mrdis_cdiv(H, DL_TH) * (unsigned)g.tw * (unsigned)g.tk;
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    const unsigned char* from = src;
    for (int i = 1; i <= iterations; ++i) {
        unsigned char* to = ((iterations - i) & 1) == 0 ? dst : ws;      // the last iteration lands in dst
        mrdis_count(MRDIS_CNT_DILATE);
        MRDIS_LAUNCH(dilate_kernel, dim3(tiles, B), dim3(LS_THREADS), 0, (hipStream_t)stream, from, to, g);
        MRDIS_CHECK_LAUNCH();
        from = to;
    }
    return MRDIS_OK;
}

static bool ls_match_args_ok(LsGeom& g, int words, int n_lesions, int B, int R, int H, int W, int D) {
    if (R < 1 || R > MRDIS_SURF_MAX_REGIONS || (long long)B * R > 65535 || words < 1 || words > (1 << 20) || n_lesions < 1) return false;
    g.R = R; g.items = B * R; g.words = words; g.n_lesions = n_lesions; g.P = (long long)H * W * D;
    return true;
}

extern "C" int mrdis_lesion_match(const unsigned char* planes, const int* comp_l, const int* rank_l, const int* comp_p, const int* rank_p,
                                  const int* first_p, int words, int n_lesions, int* bits, int* tcount, int* root, int* item, int B, int R, int H,
                                  int W, int D, void* stream) {
    if (!ls_geometry_ok(B, H, W, D)) return MRDIS_EUNSUPPORTED;
    LsGeom g;
    if (!planes || !comp_l || !rank_l || !comp_p || !rank_p || !first_p || !bits || !tcount || !root || !item) return MRDIS_EINVAL;
    if (!ls_match_args_ok(g, words, n_lesions, B, R, H, W, D)) return MRDIS_EINVAL;
    if (((((uintptr_t)comp_l) | ((uintptr_t)rank_l) | ((uintptr_t)comp_p) | ((uintptr_t)rank_p) | ((uintptr_t)first_p) | ((uintptr_t)bits) |
          ((uintptr_t)tcount) | ((uintptr_t)root) | ((uintptr_t)item)) & 3) != 0)
        return MRDIS_EALIGN;
    mrdis_count(MRDIS_CNT_LESMATCH);
    MRDIS_LAUNCH(lesion_match_kernel, dim3(ls_stride_blocks(g.P, g.items), g.items), dim3(LS_THREADS), 0, (hipStream_t)stream, planes, comp_l, rank_l,
                 comp_p, rank_p, first_p, bits, tcount, root, item, g);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_lesion_expand(const unsigned char* planes, const int* comp_l, const int* rank_l, const int* comp_p, const int* rank_p,
                                   const int* first_p, const int* bits, int words, const int* item, int n_lesions, int j0, int n,
                                   unsigned char* stack_s, unsigned char* stack_t, int B, int R, int H, int W, int D, void* stream) {
    if (!ls_geometry_ok(B, H, W, D)) return MRDIS_EUNSUPPORTED;
    LsGeom g;
    if (!planes || !comp_l || !rank_l || !comp_p || !rank_p || !first_p || !bits || !item || !stack_s || !stack_t) return MRDIS_EINVAL;
    if (!ls_match_args_ok(g, words, n_lesions, B, R, H, W, D) || j0 < 0 || n < 1 || n > 65535 || (long long)j0 + n > n_lesions) return MRDIS_EINVAL;
    if (((((uintptr_t)comp_l) | ((uintptr_t)rank_l) | ((uintptr_t)comp_p) | ((uintptr_t)rank_p) | ((uintptr_t)first_p) | ((uintptr_t)bits) |
          ((uintptr_t)item) | ((uintptr_t)stack_s) | ((uintptr_t)stack_t)) & 3) != 0)
        return MRDIS_EALIGN;
    mrdis_count(MRDIS_CNT_LESEXPAND);
    MRDIS_LAUNCH(lesion_expand_kernel, dim3(ls_stride_blocks((g.P + 3) / 4 + 1, n), n), dim3(LS_THREADS), 0, (hipStream_t)stream, planes, comp_l,
                 rank_l, comp_p, rank_p, first_p, bits, item, j0, stack_s, stack_t, g);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
