// Patch training for the 3-D nets: random (PH, PW, PD) sub-volumes of the whole stored scan, a share of them centred on a tumour voxel.
// THIS PACKAGE'S CONVENTIONS -- the reference trains on one fixed depth crop and has no patch sampling.  Three entry points:
//
//   mrdis_fg_block_counts   once per subject: how many voxels of each class lie in every block of 1024 consecutive flat indices
//                           f = (h W + w) D + d of the label volume.  The exclusive prefix over the blocks (made by the caller, once) answers
//                           "which block holds the r-th voxel of class c" by a binary search.
//   mrdis_patch_origins     per batch: one workgroup per sample turns the sample's table row -- five uint32 draws made on the host -- into the
//                           patch origin (h0, w0, d0) and the chosen class.  pick(u, n) = (u n) >> 32 maps a draw onto 0 .. n - 1.
//                             uniform:     h0 = pick(u_h, H - PH + 1), w0 and d0 likewise
//                             foreground:  class = present[pick(u_class, |present|)] over the classes with a non-zero total, in list order;
//                                          r = pick(u_voxel, n_class); the centre is the r-th voxel (0-based) of that class in increasing
//                                          flat index; h0 = clamp(hc - PH / 2, 0, H - PH), w0 and d0 likewise (clamping, never padding)
//                             centre:      h0 = (H - PH) / 2 ... (the evaluation loaders)
//                           A foreground sample without label volume, prefix table or present class takes the uniform rule with the same draws.
//   mrdis_patch_gather      per batch, inputs and targets: mrdis_volume_gather's item rules (mrdis_volgather.h) at the sample's origin, with a
//                           flip bit per axis:  out[b][i][j][k][m] = T_b(vol(b, m)[h0 + i'][w0 + j'][d0 + k']),  i' = PH - 1 - i if flipped in H.
//                           T_b's m0 is the minimum of the WHOLE stored volume (the table's minima pointers), not the patch's own minimum:
//                           that would cost a reduction per batch, and for the z-scored store both are the -10 background marker whenever
//                           the patch holds any background.
//
// Everything that varies from batch to batch is read from device memory (the table, the origins, the prefix tables), so the three launches of
// a batch replay from a captured graph with the next batch's table.  Integer and copy arithmetic throughout except T_b's two fp32 roundings;
// ballots and popcounts instead of atomics: the same bits on every run.
//
// Table row (64-bit words, ld >= 2 M + 7): the 2 M + 3 words of mrdis_volume_gather, then
//   [2M+1]  bit 0 flip H, bit 1 augment, bit 2 flip W, bit 3 flip D, bit 4 foreground sample, bit 5 centre patch
//   [2M+3]  pointer to the subject's prefix table, int32 (nblk + 1, K) (0 = none)
//   [2M+4]  u_class | u_voxel << 32        [2M+5]  u_h | u_w << 32        [2M+6]  u_d
//
// The gather is mrdis_volgather.h's kernels under its VgPatch policy (origins read from device memory and clamped there, three flips); only the
// counting and the origin kernels are written here.  Its access pattern: as mrdis_volgather.hip.  Lanes run along the patch's flat position p = (i PW + j) PD + k, so a wave's loads
// are runs of PD consecutive floats of one (h, w) column (ascending, or descending under a D flip: the same lines either way) starting at any
// d0 -- only the stores need alignment -- and land in LDS as row m of the [C][P + pad] tile; the tile leaves as 16-byte stores, m fastest.
#include "mrdis_volgather.h"

namespace {
constexpr int PT_BLOCK = 1024;              // flat indices per counted block
constexpr int PT_MAXK = MRDIS_PATCH_MAX_CLASSES;

struct PtClasses { float v[PT_MAXK]; };

__device__ __forceinline__ unsigned pt_pick(unsigned u, unsigned n) { return (unsigned)(((unsigned long long)u * n) >> 32); }

// grid nblk, 256 threads: wave w counts the indices [256 w, 256 w + 256) of the block, four ballots per class
__global__ __launch_bounds__(256) void fg_block_counts_kernel(const float* __restrict__ seg, PtClasses cls, int K, int* __restrict__ counts, long long total) {
    __shared__ int part[4][PT_MAXK];
    const int tid = threadIdx.x, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * PT_BLOCK + wave * 256;
    int cnt[PT_MAXK];
#pragma unroll
    for (int c = 0; c < PT_MAXK; ++c) cnt[c] = 0;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const long long f = base + it * 64 + (tid & 63);
        const bool in = f < total;
        const float t = in ? seg[f] : 0.f;
#pragma unroll
        for (int c = 0; c < PT_MAXK; ++c)
            if (c < K) cnt[c] += __popcll(__ballot(in && t == cls.v[c]));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < PT_MAXK; ++c) part[wave][c] = cnt[c];
    }
    __syncthreads();
    if (tid < K) counts[(long long)blockIdx.x * K + tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
}

// grid B, 64 threads (one wave); every lane computes the same origin, lane 0 writes it
__global__ __launch_bounds__(64) void patch_origins_kernel(const unsigned long long* __restrict__ table, int ld, int* __restrict__ origins, PtClasses cls, int K,
                                                           VgGeom g) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* row = table + (long long)b * ld;
    const int M = g.M;
    const unsigned flags = (unsigned)row[2 * M + 1];
    const float* seg = reinterpret_cast<const float*>(row[2 * M]);
    const int* prefix = reinterpret_cast<const int*>(row[2 * M + 3]);
    const unsigned u_class = (unsigned)(row[2 * M + 4] & 0xffffffffull), u_voxel = (unsigned)(row[2 * M + 4] >> 32);
    const unsigned u_h = (unsigned)(row[2 * M + 5] & 0xffffffffull), u_w = (unsigned)(row[2 * M + 5] >> 32), u_d = (unsigned)(row[2 * M + 6] & 0xffffffffull);
    const int rh = g.H - g.PH, rw = g.W - g.PW, rd = g.D - g.PD;
    int h0, w0, d0, chosen = -1;
    if (flags & 32u) {
        h0 = rh / 2; w0 = rw / 2; d0 = rd / 2;
    } else {
        h0 = (int)pt_pick(u_h, (unsigned)rh + 1u); w0 = (int)pt_pick(u_w, (unsigned)rw + 1u); d0 = (int)pt_pick(u_d, (unsigned)rd + 1u);
        const long long total = (long long)g.H * g.W * g.D;
        const int nblk = (int)((total + PT_BLOCK - 1) / PT_BLOCK);
        if ((flags & 16u) && seg != nullptr && prefix != nullptr && K > 0) {
            const int* tot = prefix + (long long)nblk * K;
            int present = 0;
            for (int c = 0; c < K; ++c) present += tot[c] > 0;
            if (present > 0) {
                int want = (int)pt_pick(u_class, (unsigned)present);
                for (int c = 0; c < K; ++c)
                    if (tot[c] > 0 && want-- == 0) chosen = c;
                int r = (int)pt_pick(u_voxel, (unsigned)tot[chosen]);
                // the block: the last one whose exclusive prefix is <= r (prefix is non-decreasing, prefix[0] = 0 <= r < prefix[nblk])
                int lo = 0, hi = nblk - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (prefix[(long long)mid * K + chosen] <= r) lo = mid; else hi = mid - 1;
                }
                r -= prefix[(long long)lo * K + chosen];
                const float want_v = cls.v[chosen];
                long long centre = -1;
                for (int it = 0; it < PT_BLOCK / 64; ++it) {
                    const long long f = (long long)lo * PT_BLOCK + it * 64 + lane;
                    const bool hit = f < total && seg[f] == want_v;
                    const unsigned long long bal = __ballot(hit);
                    const int n = __popcll(bal);
                    if (r < n) {
                        // the r-th set bit of the ballot: the lane with exactly r set bits below it
                        const bool mine = hit && __popcll(bal & ((1ull << lane) - 1ull)) == r;
                        const unsigned long long who = __ballot(mine);
                        centre = (long long)lo * PT_BLOCK + it * 64 + (__ffsll((long long)who) - 1);
                        break;
                    }
                    r -= n;
                }
                if (centre >= 0) {      // (always, when the prefix table belongs to this label volume)
                    const int dc = (int)(centre % g.D);
                    const long long q = centre / g.D;
                    const int wc = (int)(q % g.W), hc = (int)(q / g.W);
                    h0 = vg_clamp(hc - g.PH / 2, rh); w0 = vg_clamp(wc - g.PW / 2, rw); d0 = vg_clamp(dc - g.PD / 2, rd);
                } else {
                    chosen = -1;
                }
            }
        }
    }
    if (lane == 0) {
        int* o = origins + 4 * b;
        o[0] = h0; o[1] = w0; o[2] = d0; o[3] = chosen;
    }
}

bool pt_classes(const int* classes, int K, PtClasses* out) {
    if (K < 0 || K > PT_MAXK || (K > 0 && classes == nullptr)) return false;
    for (int c = 0; c < PT_MAXK; ++c) out->v[c] = c < K ? (float)classes[c] : 0.f;
    for (int c = 0; c < K; ++c) {
        if (classes[c] < 1 || classes[c] > 255) return false;
        for (int d = 0; d < c; ++d) if (classes[d] == classes[c]) return false;
    }
    return true;
}
}  // namespace

extern "C" int mrdis_fg_block_counts(const float* seg, const int* classes, int K, int* counts, int H, int W, int D, void* stream) {
    PtClasses cls;
    if (!seg || !counts || K < 1 || !pt_classes(classes, K, &cls) || H < 1 || W < 1 || D < 1) return MRDIS_EINVAL;
    const long long total = (long long)H * W * D;
    if (total >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    mrdis_count(MRDIS_CNT_FGCOUNT);
    MRDIS_LAUNCH(fg_block_counts_kernel, dim3(mrdis_cdiv(total, PT_BLOCK)), dim3(256), 0, (hipStream_t)stream, seg, cls, K, counts, total);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_patch_origins(const void* table, int ld_table, int* origins, const int* classes, int K, int B, int M, int H, int W, int D, int PH,
                                   int PW, int PD, void* stream) {
    PtClasses cls;
    if (!table || !origins || B < 1 || M < 1 || M > 64 || !vg_box_fits(H, W, D, PH, PW, PD) || ld_table < 2 * M + 7 || !pt_classes(classes, K, &cls))
        return MRDIS_EINVAL;
    if (B > 65535 || (long long)H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    VgGeom g;
    g.M = M; g.C = 0; g.H = H; g.W = W; g.D = D; g.PH = PH; g.PW = PW; g.PD = PD; g.N = PH * PW * PD; g.relabel = 0;
    mrdis_count(MRDIS_CNT_PATCHORIGIN);
    MRDIS_LAUNCH(patch_origins_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(table), ld_table, origins, cls, K, g);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_patch_gather(const void* table, int ld_table, const int* origins, float* out, float* mask, int B, int M, int H, int W, int D,
                                  int PH, int PW, int PD, int mode, int K, int relabel, void* stream) {
    VgGeom g;
    const int rc = vg_check(origins != nullptr, table, out, ld_table, 7, B, M, H, W, D, PH, PW, PD, mode, K, relabel, &g);
    if (rc != MRDIS_OK) return rc;
    VgPatch patch;
    patch.origins = origins;
    return vg_gather(MRDIS_CNT_PATCHGATHER, table, ld_table, patch, out, mask, g, mode, K, B, stream);
}
