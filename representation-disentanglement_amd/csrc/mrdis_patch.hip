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
// Access pattern of the gather: as mrdis_volgather.hip.  Lanes run along the patch's flat position p = (i PW + j) PD + k, so a wave's loads
// are runs of PD consecutive floats of one (h, w) column (ascending, or descending under a D flip: the same lines either way) starting at any
// d0 -- only the stores need alignment -- and land in LDS as row m of the [C][P + pad] tile; the tile leaves as 16-byte stores, m fastest.
#include "mrdis_volgather.h"

namespace {
constexpr int PT_BLOCK = 1024;              // flat indices per counted block
constexpr int PT_MAXK = MRDIS_PATCH_MAX_CLASSES;

struct PtClasses { float v[PT_MAXK]; };
struct PtGeom { int M, C, H, W, D, PH, PW, PD, N, relabel; };

__device__ __forceinline__ unsigned pt_pick(unsigned u, unsigned n) { return (unsigned)(((unsigned long long)u * n) >> 32); }
__device__ __forceinline__ int pt_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

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
                                                           PtGeom g) {
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
                    h0 = pt_clamp(hc - g.PH / 2, rh); w0 = pt_clamp(wc - g.PW / 2, rw); d0 = pt_clamp(dc - g.PD / 2, rd);
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

struct PtItem { int h0, w0, d0; bool fh, fw, fd, aug; };

__device__ __forceinline__ PtItem pt_item(const unsigned long long* row, const int* __restrict__ origins, int b, const PtGeom& g) {
    const unsigned flags = (unsigned)row[2 * g.M + 1];
    PtItem it;
    // the origins come from device memory: clamped here, so that no table can send a read outside the volume
    it.h0 = pt_clamp(origins[4 * b], g.H - g.PH); it.w0 = pt_clamp(origins[4 * b + 1], g.W - g.PW); it.d0 = pt_clamp(origins[4 * b + 2], g.D - g.PD);
    it.fh = flags & 1u; it.aug = flags & 2u; it.fw = flags & 4u; it.fd = flags & 8u;
    return it;
}
__device__ __forceinline__ long long pt_src(int p, const PtGeom& g, const PtItem& it) {
    const int q = p / g.PD, k = p - q * g.PD;
    const int i = q / g.PW, j = q - i * g.PW;
    const int hs = it.h0 + (it.fh ? g.PH - 1 - i : i), ws = it.w0 + (it.fw ? g.PW - 1 - j : j), ds = it.d0 + (it.fd ? g.PD - 1 - k : k);
    return ((long long)hs * g.W + ws) * g.D + ds;
}

// MODE 0: inputs (C = M), MODE 1: targets (C = max(K, 1)).  grid (tiles, B), 256 threads, P % 256 == 0, (N C) % 4 == 0, out 16-byte aligned.
// CM = 4: M == 4 (the BraTS set) with the four loads of a position issued together; CM = 0: M at run time.
template <int MODE, int CM>
__global__ __launch_bounds__(256) void patchgather_tile_kernel(const unsigned long long* __restrict__ table, int ld, const int* __restrict__ origins,
                                                               float* __restrict__ out, float* __restrict__ mask, PtGeom g, int K, int P, int S) {
    __shared__ float tile[VG_LDS_FLOATS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int p0 = blockIdx.x * P;
    const int n = g.N - p0 < P ? g.N - p0 : P;
    const unsigned long long* row = table + (long long)b * ld;
    const PtItem it = pt_item(row, origins, b, g);
    if (MODE == 0) {
        const float scale = __uint_as_float((unsigned)(row[2 * g.M + 2] & 0xffffffffull)), shift = __uint_as_float((unsigned)(row[2 * g.M + 2] >> 32));
        const float m0 = it.aug ? vg_item_min(row, g.M) : 0.f;
        if (mask != nullptr && blockIdx.x == 0 && tid < g.M) mask[b * g.M + tid] = row[tid] != 0ull ? 1.f : 0.f;
        for (int i = tid; i < n; i += 256) {
            const long long src = pt_src(p0 + i, g, it);
            if (CM > 0) {
                float v[CM > 0 ? CM : 1];
#pragma unroll
                for (int m = 0; m < CM; ++m) v[m] = vg_input(reinterpret_cast<const float*>(row[m]), src, it.aug, scale, shift, m0);
#pragma unroll
                for (int m = 0; m < CM; ++m) tile[m * S + i] = v[m];
            } else {
                for (int m = 0; m < g.M; ++m)
                    tile[m * S + i] = vg_input(reinterpret_cast<const float*>(row[m]), src, it.aug, scale, shift, m0);
            }
        }
    } else {
        const float* seg = reinterpret_cast<const float*>(row[2 * g.M]);
        for (int i = tid; i < n; i += 256) {
            const float t = vg_label(seg, pt_src(p0 + i, g, it), g.relabel);
            for (int c = 0; c < g.C; ++c) tile[c * S + i] = vg_target(t, c, K);
        }
    }
    __syncthreads();
    vg_store_tile(tile, out + ((long long)b * g.N + p0) * g.C, n, g.C, S, tid);
}

// every geometry: one thread per output float.  grid (x, B), grid-stride over the N C floats of a sample.
template <int MODE>
__global__ __launch_bounds__(256) void patchgather_elem_kernel(const unsigned long long* __restrict__ table, int ld, const int* __restrict__ origins,
                                                               float* __restrict__ out, float* __restrict__ mask, PtGeom g, int K) {
    const int b = blockIdx.y;
    const unsigned long long* row = table + (long long)b * ld;
    const PtItem it = pt_item(row, origins, b, g);
    const float scale = __uint_as_float((unsigned)(row[2 * g.M + 2] & 0xffffffffull)), shift = __uint_as_float((unsigned)(row[2 * g.M + 2] >> 32));
    const float m0 = (MODE == 0 && it.aug) ? vg_item_min(row, g.M) : 0.f;
    if (MODE == 0 && mask != nullptr && blockIdx.x == 0 && (int)threadIdx.x < g.M) mask[b * g.M + threadIdx.x] = row[threadIdx.x] != 0ull ? 1.f : 0.f;
    const long long total = (long long)g.N * g.C;
    float* dst = out + (long long)b * total;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
        const int p = (int)(e / g.C), c = (int)(e - (long long)p * g.C);
        const long long src = pt_src(p, g, it);
        if (MODE == 0) dst[e] = vg_input(reinterpret_cast<const float*>(row[c]), src, it.aug, scale, shift, m0);
        else dst[e] = vg_target(vg_label(reinterpret_cast<const float*>(row[2 * g.M]), src, g.relabel), c, K);
    }
}

template <int MODE>
int launch_patchgather(const unsigned long long* table, int ld, const int* origins, float* out, float* mask, const PtGeom& g, int K, int B, hipStream_t s) {
    const long long total = (long long)g.N * g.C;
    const bool tiled = !mrdis_opt(MRDIS_OPT_VOLGEN) && g.C <= VG_MAXC_TILE && (total & 3) == 0 && (((uintptr_t)out) & 15) == 0;
    mrdis_count(MRDIS_CNT_PATCHGATHER);
    if (tiled) {
        int P, S;
        vg_tile_shape(g.C, &P, &S);
        if (MODE == 0 && g.M == 4)
            MRDIS_LAUNCH((patchgather_tile_kernel<MODE, 4>), dim3(mrdis_cdiv(g.N, P), B), dim3(256), 0, s, table, ld, origins, out, mask, g, K, P, S);
        else
            MRDIS_LAUNCH((patchgather_tile_kernel<MODE, 0>), dim3(mrdis_cdiv(g.N, P), B), dim3(256), 0, s, table, ld, origins, out, mask, g, K, P, S);
    } else {
        long long gx = (total + 255) / 256; if (gx > 4096) gx = 4096;
        MRDIS_LAUNCH((patchgather_elem_kernel<MODE>), dim3((unsigned)gx, B), dim3(256), 0, s, table, ld, origins, out, mask, g, K);
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
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
bool pt_geometry(int H, int W, int D, int PH, int PW, int PD) {
    return H >= 1 && W >= 1 && D >= 1 && PH >= 1 && PW >= 1 && PD >= 1 && PH <= H && PW <= W && PD <= D;
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
    if (!table || !origins || B < 1 || M < 1 || M > 64 || !pt_geometry(H, W, D, PH, PW, PD) || ld_table < 2 * M + 7 || !pt_classes(classes, K, &cls))
        return MRDIS_EINVAL;
    if (B > 65535 || (long long)H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    PtGeom g;
    g.M = M; g.C = 0; g.H = H; g.W = W; g.D = D; g.PH = PH; g.PW = PW; g.PD = PD; g.N = PH * PW * PD; g.relabel = 0;
    mrdis_count(MRDIS_CNT_PATCHORIGIN);
    MRDIS_LAUNCH(patch_origins_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(table), ld_table, origins, cls, K, g);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_patch_gather(const void* table, int ld_table, const int* origins, float* out, float* mask, int B, int M, int H, int W, int D,
                                  int PH, int PW, int PD, int mode, int K, int relabel, void* stream) {
    if (!table || !origins || !out || B < 1 || M < 1 || M > 64 || !pt_geometry(H, W, D, PH, PW, PD) || ld_table < 2 * M + 7 ||
        (mode != 0 && mode != 1) || K < 0 || K > 64 || (mode == 0 && K != 0)) return MRDIS_EINVAL;
    if (B > 65535 || (long long)H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    PtGeom g;
    g.M = M; g.C = mode == 0 ? M : (K > 0 ? K : 1); g.H = H; g.W = W; g.D = D; g.PH = PH; g.PW = PW; g.PD = PD; g.N = PH * PW * PD; g.relabel = relabel;
    const unsigned long long* t = reinterpret_cast<const unsigned long long*>(table);
    return mode == 0 ? launch_patchgather<0>(t, ld_table, origins, out, mask, g, 0, B, (hipStream_t)stream)
                     : launch_patchgather<1>(t, ld_table, origins, out, nullptr, g, K, B, (hipStream_t)stream);
}
