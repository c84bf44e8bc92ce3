// Region scoring of predicted label volumes (surfdist.region_scores): region surfaces, the exact squared Euclidean distance transform and the
// histogram of surface distances behind the 95th-percentile Hausdorff distance.  All of it is integer arithmetic: exact, and the same bits
// from run to run.  Volumes are (B, H, W, D) with D contiguous, as mrdis_seg_label_volume writes its labels.
//
//   mrdis_region_surfaces   flags bit r = surface voxel of predicted region r, bit 4 + r = of ground-truth region r; counts (B, R, 5)
//   mrdis_edt_sq            out[s] = squared distance to the nearest voxel of source s (a bit of the flags / a plain mask), MRDIS_EDT_FAR if none
//   mrdis_surface_hist      the same transform of the 2 R surfaces, whose last pass adds into hist (B, R, 2, bins) instead of storing distances
//
// region_surfaces.  A label l <= 7 becomes the NIBBLE of the regions that hold it (bit r of the nibble = bit l of region_masks[r]): one 32-bit
// table, eight nibbles, built on the host.  Surface bits of all regions at once: nib(v) & ~(nib(n1) & ... & nib(n6)), a neighbour beyond the
// border reading as 0.  A lane takes one aligned group of four consecutive voxels of the flat (B, H W D) volume (the grouping of
// mrdis_seg_label_volume): one 32-bit load of the labels, one 16-byte load of the ground truth (4-byte aligned), one 32-bit store of the flags.
// The six neighbours are only read for a voxel that lies in some region (a tumour is a few per cent of the volume), with scalar loads that the
// voxel's coordinates guard.  Counts: thread -> wave (shuffles) -> workgroup (LDS) -> one integer atomicAdd per (workgroup, count).
//
// Distance transform, separable (Saito & Toriwaki): pass D is a 1-D nearest-feature scan, passes W and H are min-plus products with the
// parabola (i - j)^2:   g2[i] = min_j g1[j]^2 + (i - j)^2 along W,   d2[i] = min_j g2[j] + (i - j)^2 along H.
//   * pass D (edt_scan_kernel): one wave per line, 64 consecutive d per step.  The set voxels of a step are one 64-bit ballot; the nearest set
//     voxel below / above a lane is a count-leading / count-trailing-zeros of the masked ballot, or the carry of the steps before / after.  The
//     line (at most 16 steps: D <= 1024) stays in registers, the flags are read once for all sources.  Output: the DISTANCE (not squared) as
//     uint16, 0xFFFF = no feature on this line.
//   * passes W and H (edt_minplus_kernel): a workgroup owns a tile of the WHOLE line by TD consecutive d (D is the contiguous axis, so every
//     global access of the tile is a run of TD elements), converted on load to int32 squared distances in LDS, [j][d]: lane = bank, no conflict.
//     The minimum is brute force over the LDS-resident line: a wave takes four outputs i at a time, so one LDS read feeds four add / min pairs
//     and (i - j)^2 is wave-uniform (scalar) when TD = 64.  TD = 64 for lines up to 512 (128 KB of LDS at most), 32 beyond (1024 x 32 x 4 B).
//     Measured against the lower envelope of parabolas as a stand-alone kernel (tools/micro/edt_envelope.hip, profiles/surfdist_envelope_probe.txt):
//     at n = 240 the envelope's serial stack walk, one wave per CU for its LDS, takes 1.44x the time of this form.
//   * sentinel: "no feature" is MRDIS_EDT_FAR = 2^30.  FAR + (i - j)^2 <= 2^30 + 1023^2 < 2^31 does not overflow, every finite value is at most
//     3 x 1023^2 < 2^22 and so always wins the minimum, and each pass clamps what it writes back to FAR: a line without a feature stays exactly FAR.
//   * the last pass in histogram form (HIST): outputs are only computed where the partner surface has a voxel (a group of four i without one is
//     skipped, which is most of them), and instead of a store the squared distance d2 < FAR adds 1 into the histogram row of (b, r, direction).
//     Bins below SD_LBINS go through a per-workgroup LDS sub-histogram, flushed with one global integer atomic per non-empty bin
//     (cdna_hip_programming.md Guideline 12); larger d2 add straight to memory.
// The batch and the sources are grid dimensions: three launches per transform, whatever B and S.
#include "mrdis_common.h"

namespace {
constexpr int SD_THREADS = 256;
constexpr int SD_MAX_BLOCKS = 2048;          // 256 CUs x 8 workgroups
constexpr int SD_MAX_EXTENT = 1024;
constexpr int SD_CHUNKS = SD_MAX_EXTENT / 64;
constexpr int SD_LBINS = 256;                // squared distances below this go through the LDS sub-histogram
constexpr int SD_IT = 4;                     // outputs per thread and pass over the line
constexpr unsigned SD_FAR = (unsigned)MRDIS_EDT_FAR;

// ---------------------------------------------------------------------------------------------- region surfaces
// (the nibble of a label: mrdis_region_nib, mrdis_device.h -- shared with mrdis_lesion.hip, whose planes must agree with these flags voxel for voxel)

// the AND of the six neighbours' nibbles of voxel el = (h, w, d) of one sample; a neighbour beyond the border is outside every region
template <typename T>
__device__ __forceinline__ unsigned sd_neighbours(const T* __restrict__ v, long long el, int h, int w, int d, int H, int W, int D, unsigned lut) {
    const long long WD = (long long)W * D;
    unsigned all = 15u;
    all &= d > 0 ? mrdis_region_nib(v[el - 1], lut) : 0u;
    all &= d < D - 1 ? mrdis_region_nib(v[el + 1], lut) : 0u;
    all &= w > 0 ? mrdis_region_nib(v[el - D], lut) : 0u;
    all &= w < W - 1 ? mrdis_region_nib(v[el + D], lut) : 0u;
    all &= h > 0 ? mrdis_region_nib(v[el - WD], lut) : 0u;
    all &= h < H - 1 ? mrdis_region_nib(v[el + WD], lut) : 0u;
    return all;
}

// grid (gx, B), 256 threads; P = H W D voxels per sample.  A thread takes aligned groups of four voxels of the flat (B P) volume that overlap sample b.
__global__ __launch_bounds__(SD_THREADS) void region_surfaces_kernel(const unsigned char* __restrict__ labels, const unsigned long long* __restrict__ targets,
                                                                     unsigned char* __restrict__ flags, int* __restrict__ counts, long long P, int H,
                                                                     int W, int D, int R, unsigned lut) {
    __shared__ int red[SD_THREADS / 64][20];
    const int b = blockIdx.y;
    const long long v0 = (long long)b * P, v1 = v0 + P;
    const unsigned char* lab = labels + v0;                          // this sample's labels, indexed like its ground truth
    const float* tgt = targets != nullptr ? reinterpret_cast<const float*>(targets[b]) : nullptr;
    int cnt[4][5];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 5; ++k) cnt[r][k] = 0;
    const long long g0 = v0 >> 2, ngrp = ((v1 + 3) >> 2) - g0;
    for (long long gi = blockIdx.x * (long long)SD_THREADS + threadIdx.x; gi < ngrp; gi += gridDim.x * (long long)SD_THREADS) {
        const long long e0 = (g0 + gi) << 2;                         // flat voxels [e0, e0 + 4)
        const bool whole = e0 >= v0 && e0 + 4 <= v1;
        unsigned lp[4] = {0u, 0u, 0u, 0u};                           // nibbles of the four voxels: prediction, ground truth
        unsigned lt[4] = {0u, 0u, 0u, 0u};
        if (whole) {
            const unsigned l4 = *reinterpret_cast<const unsigned*>(labels + e0);
#pragma unroll
            for (int k = 0; k < 4; ++k) lp[k] = mrdis_region_nib((unsigned char)((l4 >> (8 * k)) & 255u), lut);
            if (tgt != nullptr) {
                const f32x4u t4 = *reinterpret_cast<const f32x4u*>(tgt + (e0 - v0));
                lt[0] = mrdis_region_nib(t4.x, lut); lt[1] = mrdis_region_nib(t4.y, lut); lt[2] = mrdis_region_nib(t4.z, lut); lt[3] = mrdis_region_nib(t4.w, lut);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = e0 + k;
                if (e >= v0 && e < v1) {
                    lp[k] = mrdis_region_nib(labels[e], lut);
                    if (tgt != nullptr) lt[k] = mrdis_region_nib(tgt[e - v0], lut);
                }
            }
        }
        unsigned packed = 0u;
        if ((lp[0] | lp[1] | lp[2] | lp[3] | lt[0] | lt[1] | lt[2] | lt[3]) != 0u) {      // some voxel of the group lies in some region
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if ((lp[k] | lt[k]) == 0u) continue;                 // (a voxel outside the sample has both nibbles 0)
                const long long el = e0 + k - v0;
                const int d = (int)(el % D);
                const long long hw = el / D;
                const int w = (int)(hw % W), h = (int)(hw / W);
                const unsigned sp = lp[k] != 0u ? lp[k] & ~sd_neighbours(lab, el, h, w, d, H, W, D, lut) : 0u;
                const unsigned st = lt[k] != 0u ? lt[k] & ~sd_neighbours(tgt, el, h, w, d, H, W, D, lut) : 0u;
                packed |= (sp | (st << 4)) << (8 * k);
                const unsigned both = lp[k] & lt[k];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    cnt[r][0] += (int)((both >> r) & 1u); cnt[r][1] += (int)((lp[k] >> r) & 1u); cnt[r][2] += (int)((lt[k] >> r) & 1u);
                    cnt[r][3] += (int)((sp >> r) & 1u); cnt[r][4] += (int)((st >> r) & 1u);
                }
            }
        }
        if (whole) {
            *reinterpret_cast<unsigned*>(flags + e0) = packed;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = e0 + k;
                if (e >= v0 && e < v1) flags[e] = (unsigned char)((packed >> (8 * k)) & 255u);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            int v = cnt[r][k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][5 * r + k] = v;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 5 * R) {
        const int v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (v != 0) atomicAdd(counts + (long long)b * 5 * R + threadIdx.x, v);
    }
}

// ---------------------------------------------------------------------------------------------- pass D: nearest feature along the contiguous axis
// One wave per line of D voxels, grid-stride over the B H W lines.  masks: byte s = the bits of a source byte that make a voxel a feature of
// source s.  g1 (S, lines, D) uint16.
__global__ __launch_bounds__(SD_THREADS) void edt_scan_kernel(const unsigned char* __restrict__ src, unsigned long long masks, int S,
                                                              unsigned short* __restrict__ g1, long long lines, int D) {
    const int lane = threadIdx.x & 63;
    const int nc = (D + 63) >> 6;
    const unsigned long long le_mask = ~0ull >> (63 - lane), ge_mask = ~0ull << lane;
    const long long N = lines * D;
    for (long long line = blockIdx.x * (long long)(SD_THREADS / 64) + (threadIdx.x >> 6); line < lines; line += gridDim.x * (long long)(SD_THREADS / 64)) {
        const long long base = line * D;
        unsigned v[SD_CHUNKS];
#pragma unroll
        for (int c = 0; c < SD_CHUNKS; ++c) {
            const int d = c * 64 + lane;
            v[c] = (c < nc && d < D) ? (unsigned)src[base + d] : 0u;
        }
        for (int s = 0; s < S; ++s) {
            const unsigned mk = (unsigned)(masks >> (8 * s)) & 255u;
            unsigned dl[SD_CHUNKS];
            int carry = -1;                                          // the last feature of the steps before this one, -1: none yet
#pragma unroll
            for (int c = 0; c < SD_CHUNKS; ++c) {
                dl[c] = 0xFFFFu;
                if (c < nc) {
                    const unsigned long long m = __builtin_amdgcn_ballot_w64((v[c] & mk) != 0u);
                    const unsigned long long le = m & le_mask;
                    const int left = le != 0ull ? c * 64 + 63 - __builtin_clzll(le) : carry;
                    if (left >= 0) dl[c] = (unsigned)(c * 64 + lane - left);
                    if (m != 0ull) carry = c * 64 + 63 - __builtin_clzll(m);
                }
            }
            carry = -1;                                              // the first feature of the steps after this one
            unsigned short* out = g1 + (long long)s * N + base;
#pragma unroll
            for (int c = SD_CHUNKS - 1; c >= 0; --c) {
                if (c < nc) {
                    const unsigned long long m = __builtin_amdgcn_ballot_w64((v[c] & mk) != 0u);
                    const unsigned long long ge = m & ge_mask;
                    const int right = ge != 0ull ? c * 64 + __builtin_ctzll(ge) : carry;
                    const int d = c * 64 + lane;
                    unsigned res = dl[c];
                    if (right >= 0) res = min(res, (unsigned)(right - d));
                    if (d < D) out[d] = (unsigned short)res;
                    if (m != 0ull) carry = c * 64 + __builtin_ctzll(m);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- passes W and H: min-plus with (i - j)^2
struct SdLineGeom {
    int n;                  // line length (W or H)
    int m;                  // lines per (source, sample, d): H for the W pass, W for the H pass
    long long lstride;      // elements between consecutive voxels of a line
    long long ostride;      // elements between consecutive lines
    int D, dtiles, R;
    long long P;            // voxels per sample
    long long N;            // voxels per source (B P)
    long long bins;
};

__device__ __forceinline__ unsigned sd_load_sq(const unsigned short* p) { const unsigned v = *p; return v == 0xFFFFu ? SD_FAR : v * v; }
__device__ __forceinline__ unsigned sd_load_sq(const int* p) { return (unsigned)*p; }

// grid (m dtiles, B, S), 256 threads, n TD 4 bytes of dynamic LDS.  HIST: flags / hist instead of out (see the header of this file).
template <typename TIn, int TD, bool HIST>
__global__ __launch_bounds__(SD_THREADS) void edt_minplus_kernel(const TIn* __restrict__ in, int* __restrict__ out, const unsigned char* __restrict__ flags,
                                                                 int* __restrict__ hist, SdLineGeom g) {
    extern __shared__ __attribute__((aligned(16))) unsigned sd_tile[];      // [n][TD]
    __shared__ int lhist[HIST ? SD_LBINS : 1];
    constexpr int NG = SD_THREADS / TD;                              // groups of outputs that work side by side
    const int o = blockIdx.x / g.dtiles, dt = blockIdx.x - o * g.dtiles;
    const int b = blockIdx.y, s = blockIdx.z;
    const long long vox0 = (long long)b * g.P + (long long)o * g.ostride + (long long)dt * TD;      // voxel (line o, i = 0, first d of the tile) of the sample
    const TIn* src = in + (long long)s * g.N + vox0;
    const int dmax = g.D - dt * TD;                                  // d of the tile that exist: dd < dmax
    if (HIST)
        for (int k = threadIdx.x; k < SD_LBINS; k += SD_THREADS) lhist[k] = 0;
    for (int idx = threadIdx.x; idx < g.n * TD; idx += SD_THREADS) {
        const int j = idx / TD, dd = idx - j * TD;
        sd_tile[idx] = dd < dmax ? sd_load_sq(src + (long long)j * g.lstride + dd) : SD_FAR;
    }
    __syncthreads();
    const int dd = threadIdx.x % TD;
    const int ig = TD == 64 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x / TD);
    const bool live = dd < dmax;
    // HIST: source s < R is the surface of predicted region r = s, measured at the ground truth's surface voxels (bit 4 + r): direction 0;
    // source s >= R the ground truth's surface of r = s - R, measured at the prediction's (bit r): direction 1
    const int r = HIST ? (s < g.R ? s : s - g.R) : 0;
    const unsigned partner = HIST ? (s < g.R ? 16u << r : 1u << r) : 0u;
    int* hrow = HIST ? hist + (((long long)b * g.R + r) * 2 + (s < g.R ? 0 : 1)) * g.bins : nullptr;
    for (int i0 = ig * SD_IT; i0 < g.n; i0 += NG * SD_IT) {
        bool need[SD_IT];
        bool any = false;
#pragma unroll
        for (int t = 0; t < SD_IT; ++t) {
            need[t] = live && i0 + t < g.n;
            if (HIST && need[t]) need[t] = (flags[vox0 + (long long)(i0 + t) * g.lstride + dd] & partner) != 0u;
            any = any || need[t];
        }
        if (!any) continue;
        unsigned acc[SD_IT];
#pragma unroll
        for (int t = 0; t < SD_IT; ++t) acc[t] = SD_FAR;
        for (int j = 0; j < g.n; ++j) {
            const unsigned gj = sd_tile[j * TD + dd];
#pragma unroll
            for (int t = 0; t < SD_IT; ++t) {
                const int di = i0 + t - j;
                acc[t] = min(acc[t], gj + (unsigned)(di * di));
            }
        }
#pragma unroll
        for (int t = 0; t < SD_IT; ++t) {
            if (!need[t]) continue;
            const unsigned v = min(acc[t], SD_FAR);
            if (HIST) {
                if (v < (unsigned)SD_LBINS) atomicAdd(&lhist[v], 1);
                else if ((long long)v < g.bins) atomicAdd(hrow + v, 1);          // (FAR: the source surface is empty, nothing is added)
            } else {
                out[(long long)s * g.N + vox0 + (long long)(i0 + t) * g.lstride + dd] = (int)v;
            }
        }
    }
    if (HIST) {
        __syncthreads();
        for (int k = threadIdx.x; k < SD_LBINS; k += SD_THREADS) {
            const int c = lhist[k];
            if (c != 0 && (long long)k < g.bins) atomicAdd(hrow + k, c);
        }
    }
}

bool sd_geometry_ok(int B, int H, int W, int D) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || D < 1 || H > SD_MAX_EXTENT || W > SD_MAX_EXTENT || D > SD_MAX_EXTENT) return false;
    const long long far2 = (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) + (long long)(D - 1) * (D - 1);
    return far2 < (long long)MRDIS_EDT_FAR;
}
size_t sd_g1_bytes(int S, long long N) { return ((size_t)S * (size_t)N * 2 + 15) & ~(size_t)15; }

template <typename TIn, bool HIST>
int sd_launch_minplus(const TIn* in, int* out, const unsigned char* flags, int* hist, const SdLineGeom& g0, int B, int S, hipStream_t s) {
    SdLineGeom g = g0;
    if (g.n <= 512) {
        constexpr int TD = 64;
        g.dtiles = mrdis_cdiv(g.D, TD);
        const size_t lds = (size_t)g.n * TD * 4;
        if (!mrdis_lds_optin((const void*)edt_minplus_kernel<TIn, TD, HIST>, 128 * 1024)) return MRDIS_ELAUNCH;      // (static LDS comes on top: always opt in)
        MRDIS_LAUNCH((edt_minplus_kernel<TIn, TD, HIST>), dim3(g.m * g.dtiles, B, S), dim3(SD_THREADS), lds, s, in, out, flags, hist, g);
    } else {
        constexpr int TD = 32;
        g.dtiles = mrdis_cdiv(g.D, TD);
        const size_t lds = (size_t)g.n * TD * 4;
        if (!mrdis_lds_optin((const void*)edt_minplus_kernel<TIn, TD, HIST>, 128 * 1024)) return MRDIS_ELAUNCH;
        MRDIS_LAUNCH((edt_minplus_kernel<TIn, TD, HIST>), dim3(g.m * g.dtiles, B, S), dim3(SD_THREADS), lds, s, in, out, flags, hist, g);
    }
    return MRDIS_OK;
}

// the three passes over S sources; `hist` given: the last pass is the histogram form over the flags in `src`
int sd_transform(const unsigned char* src, unsigned long long masks, int S, int* out, int* hist, long long bins, int R, void* workspace,
                 size_t workspace_bytes, int B, int H, int W, int D, hipStream_t s) {
    const long long P = (long long)H * W * D, N = P * B, lines = (long long)B * H * W;
    if (workspace_bytes < sd_g1_bytes(S, N) + (size_t)S * (size_t)N * 4) return MRDIS_EWORKSPACE;
    unsigned short* g1 = reinterpret_cast<unsigned short*>(workspace);
    int* g2 = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + sd_g1_bytes(S, N));
    const long long nb = (lines + SD_THREADS / 64 - 1) / (SD_THREADS / 64);
    mrdis_count(MRDIS_CNT_EDT);
    MRDIS_LAUNCH(edt_scan_kernel, dim3((unsigned)(nb > 8 * SD_MAX_BLOCKS ? 8 * SD_MAX_BLOCKS : nb)), dim3(SD_THREADS), 0, s, src, masks, S, g1, lines, D);
    MRDIS_CHECK_LAUNCH();
    SdLineGeom g;
    g.D = D; g.dtiles = 0; g.R = R; g.P = P; g.N = N; g.bins = bins;
    g.n = W; g.m = H; g.lstride = D; g.ostride = (long long)W * D;                   // along W
    mrdis_count(MRDIS_CNT_EDT);
    int rc = sd_launch_minplus<unsigned short, false>(g1, g2, nullptr, nullptr, g, B, S, s);
    if (rc != MRDIS_OK) return rc;
    MRDIS_CHECK_LAUNCH();
    g.n = H; g.m = W; g.lstride = (long long)W * D; g.ostride = D;                   // along H
    if (hist != nullptr) {
        mrdis_count(MRDIS_CNT_SURFHIST);
        rc = sd_launch_minplus<int, true>(g2, nullptr, src, hist, g, B, S, s);
    } else {
        mrdis_count(MRDIS_CNT_EDT);
        rc = sd_launch_minplus<int, false>(g2, out, nullptr, nullptr, g, B, S, s);
    }
    if (rc != MRDIS_OK) return rc;
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
}  // namespace

extern "C" int mrdis_region_surfaces(const unsigned char* labels, const void* targets, const int* region_masks, int R, unsigned char* flags,
                                     int* counts, int B, int H, int W, int D, void* stream) {
    if (!labels || !region_masks || !flags || !counts || R < 1 || R > MRDIS_SURF_MAX_REGIONS || B < 1 || H < 1 || W < 1 || D < 1) return MRDIS_EINVAL;
    if (B > 65535 || (long long)H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    if (((((uintptr_t)labels) | ((uintptr_t)flags) | ((uintptr_t)counts)) & 3) != 0 || (((uintptr_t)targets) & 7) != 0) return MRDIS_EALIGN;
    unsigned lut = 0u;                                               // nibble l: the regions that hold label l
    for (int r = 0; r < R; ++r) {
        if (region_masks[r] < 0 || region_masks[r] > 255) return MRDIS_EINVAL;
        for (int l = 0; l < 8; ++l)
            if ((region_masks[r] >> l) & 1) lut |= 1u << (4 * l + r);
    }
    const long long P = (long long)H * W * D;
    long long nb = ((P + 3) / 4 + 1 + SD_THREADS - 1) / SD_THREADS, cap = SD_MAX_BLOCKS / B;
    if (cap < 1) cap = 1;
    if (nb > cap) nb = cap;
    mrdis_count(MRDIS_CNT_REGSURF);
    MRDIS_LAUNCH(region_surfaces_kernel, dim3((unsigned)nb, B), dim3(SD_THREADS), 0, (hipStream_t)stream, labels,
                 reinterpret_cast<const unsigned long long*>(targets), flags, counts, P, H, W, D, R, lut);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" size_t mrdis_edt_workspace(int S, int B, int H, int W, int D) {
    if (S < 1 || S > MRDIS_EDT_MAX_SRC || !sd_geometry_ok(B, H, W, D)) return 0;
    const long long N = (long long)B * H * W * D;
    return sd_g1_bytes(S, N) + (size_t)S * (size_t)N * 4;
}

extern "C" int mrdis_edt_sq(const unsigned char* src, const unsigned char* src_masks, int S, int* out, void* workspace, size_t workspace_bytes,
                            int B, int H, int W, int D, void* stream) {
    if (!src || !src_masks || !out || !workspace || S < 1 || S > MRDIS_EDT_MAX_SRC || !sd_geometry_ok(B, H, W, D)) return MRDIS_EINVAL;
    if (((((uintptr_t)out) | ((uintptr_t)workspace)) & 15) != 0) return MRDIS_EALIGN;
    unsigned long long masks = 0ull;
    for (int s = 0; s < S; ++s) masks |= (unsigned long long)src_masks[s] << (8 * s);
    return sd_transform(src, masks, S, out, nullptr, 0, 0, workspace, workspace_bytes, B, H, W, D, (hipStream_t)stream);
}

extern "C" int mrdis_surface_hist(const unsigned char* flags, int R, int* hist, long long bins, void* workspace, size_t workspace_bytes, int B,
                                  int H, int W, int D, void* stream) {
    if (!flags || !hist || !workspace || R < 1 || R > MRDIS_SURF_MAX_REGIONS || !sd_geometry_ok(B, H, W, D)) return MRDIS_EINVAL;
    if (bins != (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) + (long long)(D - 1) * (D - 1) + 1) return MRDIS_EINVAL;
    if ((((uintptr_t)workspace) & 15) != 0 || (((uintptr_t)hist) & 3) != 0) return MRDIS_EALIGN;
    unsigned long long masks = 0ull;                                 // sources 0 .. R - 1: bit r (prediction), R .. 2 R - 1: bit 4 + r (ground truth)
    for (int r = 0; r < R; ++r) {
        masks |= (unsigned long long)(1u << r) << (8 * r);
        masks |= (unsigned long long)(16u << r) << (8 * (R + r));
    }
    return sd_transform(flags, masks, 2 * R, nullptr, hist, bins, R, workspace, workspace_bytes, B, H, W, D, (hipStream_t)stream);
}
