// Batch assembly for the 3-D nets (ZeroDoseDataset3D.__getitem__ + default collate, util.py:723-810) from volumes resident in HBM.
//
// The 3-D store keeps every volume as the reference's h5 file has it, (H, W, D) with D fastest, so the depth crop [z0, z0 + Dz) of one (h, w)
// column is one contiguous run and a batch is a pure interleave of M such volumes:
//   inputs [b][h][w][z][m] = T_b( vol(b, m)[hs][w][z0 + z] )        hs = H - 1 - h if the item is flipped, else h     (channels-last-3d, what model3d reads)
//   targets[b][h][w][z]    = seg(b)[hs][w][z0 + z], label 4 -> 3 (BraTS)      or, with K region channels, [b][h][w][z][c] = (label == c + 1)
// A contrast that is missing for the subject or was dropped (pointer 0 in the table) reads as 0 everywhere.
//
// T_b is the reference's augmentation (util.py:798-805): v = x * scale + shift in fp32 (two roundings, no contraction: the same bits as a torch
// mul followed by an add), then `inputs[inputs == inputs.min()] = -10` over the whole item.  No reduction pass runs for that minimum:
//   * scale lies in [0.9, 1.1], so x -> x * scale + shift is increasing and the elements that equal the transformed minimum are exactly the
//     elements whose RAW value equals the item's raw minimum m0 (two raw values would have to differ by less than an ulp of `shift` to be
//     told apart raw and merged transformed: background markers and intensities are not that close);
//   * m0 = min over the present, not-dropped contrasts of that volume's minimum inside the crop -- kept with the store, computed once per
//     volume -- and 0 if any contrast is absent (its zeros take part in the reference's min());
//   * so the kernel compares the raw value with m0 and writes -10 there, x * scale + shift elsewhere.
//
// Everything that changes from batch to batch comes from ONE device table (B rows of 2 M + 3 64-bit words, one pinned H2D copy per batch), so a
// captured launch replays with the next batch's draws:
//   [0, M)   volume pointers (0 = absent or dropped)        [M, 2M)  pointers to those volumes' crop minima (fp32, device)
//   [2M]     target volume pointer (0 = absent)             [2M+1]   bit 0 flip, bit 1 aug           [2M+2]  scale bits | shift bits << 32
//
// Access pattern.  The store is z-fastest per volume, the output is m-fastest, then z.  A workgroup takes P consecutive output positions
// p = (h W + w) Dz + z of one sample: lanes run along p, so every load of a wave is one contiguous run per (h, w) column (256 bytes at Dz = 64)
// and lands in LDS as row m of a [C][P + pad] tile (conflict-free 4-byte writes); the tile then leaves as consecutive 16-byte stores, 1 KB per
// wave instruction, each lane collecting its four floats from LDS rows (C = 4: four conflict-free row reads; the pad keeps C = 8 / 16 so).
// This is not the 2-D loader's first form (28-byte pieces at a 112-byte stride, 0.6 TB/s): no store here is narrower than a full line.
// Any geometry the tile form does not take (C > 32, (H W Dz C) % 4 != 0, unaligned output) runs the element kernel below it: one thread per
// output float, coalesced 4-byte stores, strided reads.
#include "mrdis_volgather.h"                                    // the rules and the tile shared with mrdis_patch.hip

namespace {
struct VgGeom { int M, C, H, W, D, z0, Dz, N, relabel; };

__device__ __forceinline__ long long vg_src(int p, const VgGeom& g, bool flip) {
    const int q = p / g.Dz, z = p - q * g.Dz;
    const int h = q / g.W, w = q - h * g.W;
    const int hs = flip ? g.H - 1 - h : h;
    return ((long long)hs * g.W + w) * g.D + g.z0 + z;
}

// MODE 0: inputs (C = M), MODE 1: targets (C = max(K, 1)).  grid (tiles, B), 256 threads, P % 256 == 0, (N C) % 4 == 0, out 16-byte aligned.
// CM = 4: M == 4 (the BraTS set) with the four loads of a position issued together; CM = 0: M at run time.
template <int MODE, int CM>
__global__ __launch_bounds__(256) void volgather_tile_kernel(const unsigned long long* __restrict__ table, int ld, float* __restrict__ out,
                                                             float* __restrict__ mask, VgGeom g, int K, int P, int S) {
    __shared__ float tile[VG_LDS_FLOATS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int p0 = blockIdx.x * P;
    const int n = g.N - p0 < P ? g.N - p0 : P;
    const unsigned long long* row = table + (long long)b * ld;
    const unsigned flags = (unsigned)row[2 * g.M + 1];
    const bool flip = flags & 1u, aug = flags & 2u;
    if (MODE == 0) {
        const float scale = __uint_as_float((unsigned)(row[2 * g.M + 2] & 0xffffffffull)), shift = __uint_as_float((unsigned)(row[2 * g.M + 2] >> 32));
        const float m0 = aug ? vg_item_min(row, g.M) : 0.f;
        if (mask != nullptr && blockIdx.x == 0 && tid < g.M) mask[b * g.M + tid] = row[tid] != 0ull ? 1.f : 0.f;
        for (int i = tid; i < n; i += 256) {
            const long long src = vg_src(p0 + i, g, flip);
            if (CM > 0) {
                float v[CM > 0 ? CM : 1];
#pragma unroll
                for (int m = 0; m < CM; ++m) v[m] = vg_input(reinterpret_cast<const float*>(row[m]), src, aug, scale, shift, m0);
#pragma unroll
                for (int m = 0; m < CM; ++m) tile[m * S + i] = v[m];
            } else {
                for (int m = 0; m < g.M; ++m)
                    tile[m * S + i] = vg_input(reinterpret_cast<const float*>(row[m]), src, aug, scale, shift, m0);
            }
        }
    } else {
        const float* seg = reinterpret_cast<const float*>(row[2 * g.M]);
        for (int i = tid; i < n; i += 256) {
            const float t = vg_label(seg, vg_src(p0 + i, g, flip), g.relabel);
            for (int c = 0; c < g.C; ++c) tile[c * S + i] = vg_target(t, c, K);
        }
    }
    __syncthreads();
    vg_store_tile(tile, out + ((long long)b * g.N + p0) * g.C, n, g.C, S, tid);
}

// every geometry: one thread per output float.  grid (x, B), grid-stride over the N C floats of a sample.
template <int MODE>
__global__ __launch_bounds__(256) void volgather_elem_kernel(const unsigned long long* __restrict__ table, int ld, float* __restrict__ out,
                                                             float* __restrict__ mask, VgGeom g, int K) {
    const int b = blockIdx.y;
    const unsigned long long* row = table + (long long)b * ld;
    const unsigned flags = (unsigned)row[2 * g.M + 1];
    const bool flip = flags & 1u, aug = flags & 2u;
    const float scale = __uint_as_float((unsigned)(row[2 * g.M + 2] & 0xffffffffull)), shift = __uint_as_float((unsigned)(row[2 * g.M + 2] >> 32));
    const float m0 = (MODE == 0 && aug) ? vg_item_min(row, g.M) : 0.f;
    if (MODE == 0 && mask != nullptr && blockIdx.x == 0 && (int)threadIdx.x < g.M) mask[b * g.M + threadIdx.x] = row[threadIdx.x] != 0ull ? 1.f : 0.f;
    const long long total = (long long)g.N * g.C;
    float* dst = out + (long long)b * total;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
        const int p = (int)(e / g.C), c = (int)(e - (long long)p * g.C);
        const long long src = vg_src(p, g, flip);
        if (MODE == 0) dst[e] = vg_input(reinterpret_cast<const float*>(row[c]), src, aug, scale, shift, m0);
        else dst[e] = vg_target(vg_label(reinterpret_cast<const float*>(row[2 * g.M]), src, g.relabel), c, K);
    }
}

template <int MODE>
int launch_volgather(const unsigned long long* table, int ld, float* out, float* mask, const VgGeom& g, int K, int B, hipStream_t s) {
    const long long total = (long long)g.N * g.C;
    const bool tiled = !mrdis_opt(MRDIS_OPT_VOLGEN) && g.C <= VG_MAXC_TILE && (total & 3) == 0 && (((uintptr_t)out) & 15) == 0;
    mrdis_count(MRDIS_CNT_VOLGATHER);
    if (tiled) {
        int P, S;
        vg_tile_shape(g.C, &P, &S);
        if (MODE == 0 && g.M == 4)
            MRDIS_LAUNCH((volgather_tile_kernel<MODE, 4>), dim3(mrdis_cdiv(g.N, P), B), dim3(256), 0, s, table, ld, out, mask, g, K, P, S);
        else
            MRDIS_LAUNCH((volgather_tile_kernel<MODE, 0>), dim3(mrdis_cdiv(g.N, P), B), dim3(256), 0, s, table, ld, out, mask, g, K, P, S);
    } else {
        long long gx = (total + 255) / 256; if (gx > 4096) gx = 4096;
        MRDIS_LAUNCH((volgather_elem_kernel<MODE>), dim3((unsigned)gx, B), dim3(256), 0, s, table, ld, out, mask, g, K);
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
}  // namespace

extern "C" int mrdis_volume_gather(const void* table, int ld_table, float* out, float* mask, int B, int M, int H, int W, int D, int z0, int Dz,
                                   int mode, int K, int relabel, void* stream) {
    if (!table || !out || B < 1 || M < 1 || M > 64 || H < 1 || W < 1 || D < 1 || z0 < 0 || Dz < 1 || z0 + Dz > D || ld_table < 2 * M + 3 ||
        (mode != 0 && mode != 1) || K < 0 || K > 64 || (mode == 0 && K != 0)) return MRDIS_EINVAL;
    if (B > 65535 || (long long)H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    VgGeom g;
    g.M = M; g.C = mode == 0 ? M : (K > 0 ? K : 1); g.H = H; g.W = W; g.D = D; g.z0 = z0; g.Dz = Dz; g.N = H * W * Dz; g.relabel = relabel;
    const unsigned long long* t = reinterpret_cast<const unsigned long long*>(table);
    return mode == 0 ? launch_volgather<0>(t, ld_table, out, mask, g, 0, B, (hipStream_t)stream)
                     : launch_volgather<1>(t, ld_table, out, nullptr, g, K, B, (hipStream_t)stream);
}
