// The gather of the 3-D store, written once for its three entry points: mrdis_volume_gather (mrdis_volgather.hip: the reference's depth crop),
// mrdis_patch_gather (mrdis_patch.hip: random patches) and mrdis_patch_warp (mrdis_warp.hip: rotated and zoomed patches).  Here are the
// geometry, the decode of a table row, the per-element rules of an item -- T_b, the label rule, the region channels -- the source of an output
// voxel that is copied, the LDS tile with its fill and store phases, the flat tile kernel, the element kernel, the launch decision and the
// argument check.  The three sources add what tells them apart: how an output position finds its source (a policy type, below) and, for
// the warp, its brick-shaped tile kernel and its resampling arithmetic.
// The rules and the table row are documented where they were first written, in the header comment of mrdis_volgather.hip; the words a
// patch row and a warp row add, in those of mrdis_patch.hip and mrdis_warp.hip.
#pragma once
#include "mrdis_common.h"

constexpr int VG_TILE_FLOATS = 8192;        // 32 KB tile: P = 1024 positions at C <= 8, 512 at C <= 16, 256 at C <= 32
constexpr int VG_MAXC_TILE = 32;
constexpr int VG_LDS_FLOATS = VG_TILE_FLOATS + VG_MAXC_TILE * 4;

// M contrasts, C output channels (inputs: M; targets: max(K, 1)), the stored volumes (H, W, D), the output box (PH, PW, PD) of a sample -- the
// depth crop's (H, W, Dz), a patch -- with its N = PH PW PD positions
struct VgGeom { int M, C, H, W, D, PH, PW, PD, N, relabel; };

static inline bool vg_box_fits(int H, int W, int D, int PH, int PW, int PD) {
    return H >= 1 && W >= 1 && D >= 1 && PH >= 1 && PW >= 1 && PD >= 1 && PH <= H && PW <= W && PD <= D;
}

// What the entry points check alike, in their order of precedence (MRDIS_EINVAL before MRDIS_EUNSUPPORTED), then the geometry.  `ok`: what
// an entry point checks of its own; `extra`: the words of its table row beyond the 2 M pointers.
static inline int vg_check(bool ok, const void* table, const float* out, int ld_table, int extra, int B, int M, int H, int W, int D, int PH, int PW,
                           int PD, int mode, int K, int relabel, VgGeom* g) {
    if (!ok || !table || !out || B < 1 || M < 1 || M > 64 || !vg_box_fits(H, W, D, PH, PW, PD) || ld_table < 2 * M + extra ||
        (mode != 0 && mode != 1) || K < 0 || K > 64 || (mode == 0 && K != 0)) return MRDIS_EINVAL;
    if (B > 65535 || (long long)H * W * D >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    g->M = M; g->C = mode == 0 ? M : (K > 0 ? K : 1); g->H = H; g->W = W; g->D = D; g->PH = PH; g->PW = PW; g->PD = PD; g->N = PH * PW * PD;
    g->relabel = relabel;
    return MRDIS_OK;
}

// the item's raw minimum (mrdis_volgather.hip); every thread walks the M <= 64 uniform table words
static __device__ __forceinline__ float vg_item_min(const unsigned long long* row, int M) {
    float m0 = __builtin_inff();
    bool absent = false;
    for (int m = 0; m < M; ++m) {
        if (row[m] != 0ull) m0 = fminf(m0, *reinterpret_cast<const float*>(row[M + m]));
        else absent = true;
    }
    return absent ? fminf(m0, 0.f) : m0;
}
static __device__ __forceinline__ float vg_input(const float* vol, long long src, bool aug, float scale, float shift, float m0) {
#pragma clang fp contract(off)              // two roundings, never one fused multiply-add (hipcc contracts by default, __fmul_rn / __fadd_rn included)
    const float x = vol ? vol[src] : 0.f;
    if (!aug) return x;
    const float xs = x * scale;
    return x == m0 ? -10.f : xs + shift;
}
static __device__ __forceinline__ float vg_label(const float* seg, long long src, int relabel) {
    const float t = seg ? seg[src] : 0.f;
    return (relabel && t == 4.f) ? 3.f : t;              // util.py:785
}
static __device__ __forceinline__ float vg_target(float t, int c, int K) { return K == 0 ? t : (t == (float)(c + 1) ? 1.f : 0.f); }

// The head of sample b's table row, decoded once per workgroup: the row's words, the target volume [2M], the flag word [2M+1], T_b's scale,
// shift and m0 (MODE 0 with the augment bit only).  MODE 0 also writes the sample's mask row, from the first workgroup along x (a null
// mask: none).  `*it`: where the policy `pol` (below) places the sample's box -- asked as soon as the flag word is there, so that its loads
// go out beside the row's and ahead of m0's chain of dependent loads and of the mask store.
struct VgRow { const unsigned long long* w; const float* seg; unsigned flags; bool aug; float scale, shift, m0; };

template <int MODE, class POL>
static __device__ __forceinline__ VgRow vg_row(const unsigned long long* table, int ld, int b, const VgGeom& g, float* mask, const POL& pol, typename POL::Item* it) {
    const int M = g.M;
    VgRow r;
    r.w = table + (long long)b * ld;
    r.seg = reinterpret_cast<const float*>(r.w[2 * M]);
    r.flags = (unsigned)r.w[2 * M + 1];
    r.aug = r.flags & 2u;
    *it = pol.item(r, b, g);
    r.scale = __uint_as_float((unsigned)(r.w[2 * M + 2] & 0xffffffffull)); r.shift = __uint_as_float((unsigned)(r.w[2 * M + 2] >> 32));
    r.m0 = (MODE == 0 && r.aug) ? vg_item_min(r.w, M) : 0.f;
    if (MODE == 0 && mask != nullptr && blockIdx.x == 0 && (int)threadIdx.x < M) mask[b * M + threadIdx.x] = r.w[threadIdx.x] != 0ull ? 1.f : 0.f;
    return r;
}

// Where a sample's box lies in the volume and which of its axes run backwards; the source of output voxel (i, j, k) of the box when the
// sample is copied: out[b][i][j][k] reads vol[o0 + i'][o1 + j'][o2 + k'], i' = PH - 1 - i under the H flip
struct VgItem { int o[3]; bool fh, fw, fd; };

static __device__ __forceinline__ int vg_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
static __device__ __forceinline__ long long vg_copy_src(int i, int j, int k, const VgGeom& g, const VgItem& it) {
    const int hs = it.o[0] + (it.fh ? g.PH - 1 - i : i), ws = it.o[1] + (it.fw ? g.PW - 1 - j : j), ds = it.o[2] + (it.fd ? g.PD - 1 - k : k);
    return ((long long)hs * g.W + ws) * g.D + ds;
}
// the flat position p = (i PW + j) PD + k of the box
static __device__ __forceinline__ void vg_unflat(int p, const VgGeom& g, int* i, int* j, int* k) {
    const int q = p / g.PD;
    *k = p - q * g.PD; *i = q / g.PW; *j = q - *i * g.PW;
}
// contrast m, and output float c, of a copied voxel
static __device__ __forceinline__ float vg_row_input(const VgRow& r, int m, long long src) {
    return vg_input(reinterpret_cast<const float*>(r.w[m]), src, r.aug, r.scale, r.shift, r.m0);
}
template <int MODE>
static __device__ __forceinline__ float vg_copy_value(const VgRow& r, long long src, int c, const VgGeom& g, int K) {
    if (MODE == 0) return vg_row_input(r, c, src);
    return vg_target(vg_label(r.seg, src, g.relabel), c, K);
}

// Position to source: the policy types, passed to the kernels by value.  `item` places sample b's box (r: its decoded row) and
// `value` gives output float c of voxel (i, j, k) to the element kernel.
struct VgCopy {                             // every sample is copied
    template <int MODE>
    static __device__ __forceinline__ float value(const VgRow& r, const VgItem& it, int i, int j, int k, int c, const VgGeom& g, int K) {
        return vg_copy_value<MODE>(r, vg_copy_src(i, j, k, g, it), c, g, K);
    }
};
struct VgCrop : VgCopy {                    // the depth crop [z0, z0 + PD) of the whole H x W, the host's z0 (checked there); the H flip only
    int z0;
    typedef VgItem Item;
    __device__ __forceinline__ Item item(const VgRow& r, int b, const VgGeom& g) const {
        Item it;
        it.o[0] = 0; it.o[1] = 0; it.o[2] = z0;
        it.fh = r.flags & 1u; it.fw = false; it.fd = false;
        return it;
    }
};
struct VgPatch : VgCopy {                   // a patch at origins[4 b .. 4 b + 2] (mrdis_patch_origins), a flip bit per axis
    const int* origins;
    typedef VgItem Item;
    __device__ __forceinline__ Item item(const VgRow& r, int b, const VgGeom& g) const {
        Item it;
        // the origins come from device memory: clamped here, so that no table can send a read outside the volume
        it.o[0] = vg_clamp(origins[4 * b], g.H - g.PH); it.o[1] = vg_clamp(origins[4 * b + 1], g.W - g.PW); it.o[2] = vg_clamp(origins[4 * b + 2], g.D - g.PD);
        it.fh = r.flags & 1u; it.fw = r.flags & 4u; it.fd = r.flags & 8u;
        return it;
    }
};

// positions per tile and the row stride of the [C][S] LDS tile: a lane's four reads of the store phase sit 4 S apart per neighbouring lane at
// C = 8 (S % 8 == 4 puts the two rows on opposite halves of the 32 banks) and at C = 16 (S % 8 == 2: four rows, 8 banks apart); C = 4 reads
// whole rows and needs none
struct VgFlat { int P, S; };
static inline VgFlat vg_tile_shape(int C) {
    VgFlat sh;
    int p = VG_TILE_FLOATS / C / 256 * 256; if (p > 1024) p = 1024;
    if (p < 256) p = 256;                   // C > VG_MAXC_TILE is never tiled (vg_launch): only keeps the callers' grid arithmetic defined
    sh.P = p;
    sh.S = p + ((C % 16) == 0 ? 2 : (C % 8) == 0 ? 4 : (C % 4) == 0 ? 0 : 1);
    return sh;
}

// fill phase of one copied voxel: column `col` = tile + its position.  CM = 4: M == 4 (the BraTS set) with the four loads issued together;
// CM = 0: M at run time
template <int CM>
static __device__ __forceinline__ void vg_fill_inputs(float* col, int S, const VgRow& r, long long src, int M) {
    if (CM > 0) {
        float v[CM > 0 ? CM : 1];
#pragma unroll
        for (int m = 0; m < CM; ++m) v[m] = vg_row_input(r, m, src);
#pragma unroll
        for (int m = 0; m < CM; ++m) col[m * S] = v[m];
    } else {
        for (int m = 0; m < M; ++m) col[m * S] = vg_row_input(r, m, src);
    }
}
static __device__ __forceinline__ void vg_fill_targets(float* col, int S, const VgRow& r, long long src, const VgGeom& g, int K) {
    const float t = vg_label(r.seg, src, g.relabel);
    for (int c = 0; c < g.C; ++c) col[c * S] = vg_target(t, c, K);
}

// store phase: the n positions x C channels of the tile leave as consecutive 16-byte stores, channel fastest ((n C) % 4 == 0, dst 16-byte aligned)
static __device__ __forceinline__ void vg_store_tile(const float* tile, float* out, int n, int C, int S, int tid) {
    const int nv = n * C / 4;
    f32x4* dst = reinterpret_cast<f32x4*>(out);
    if ((C & 3) == 0) {
        for (int f = tid; f < nv; f += 256) {
            const int e = 4 * f, p = e / C, c = e - p * C;
            const f32x4 v = {tile[c * S + p], tile[(c + 1) * S + p], tile[(c + 2) * S + p], tile[(c + 3) * S + p]};
            dst[f] = v;
        }
    } else {
        for (int f = tid; f < nv; f += 256) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * f + k, p = e / C, c = e - p * C;
                v[k] = tile[c * S + p];
            }
            const f32x4 v4 = {v[0], v[1], v[2], v[3]};
            dst[f] = v4;
        }
    }
}

namespace {
// The flat tile: a workgroup takes sh.P consecutive positions of one sample's box.  MODE 0: inputs (C = M), MODE 1: targets (C = max(K, 1)).
// grid (tiles, B), 256 threads, P % 256 == 0, (N C) % 4 == 0, out 16-byte aligned.
template <int MODE, int CM, class POL>
__global__ __launch_bounds__(256) void vg_tile_kernel(const unsigned long long* __restrict__ table, int ld, POL pol, float* __restrict__ out,
                                                      float* __restrict__ mask, VgGeom g, int K, VgFlat sh) {
    __shared__ float tile[VG_LDS_FLOATS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int p0 = blockIdx.x * sh.P;
    const int n = g.N - p0 < sh.P ? g.N - p0 : sh.P;
    typename POL::Item it;
    const VgRow r = vg_row<MODE>(table, ld, b, g, mask, pol, &it);
    for (int p = tid; p < n; p += 256) {
        int i, j, k;
        vg_unflat(p0 + p, g, &i, &j, &k);
        const long long src = vg_copy_src(i, j, k, g, it);
        if (MODE == 0) vg_fill_inputs<CM>(tile + p, sh.S, r, src, g.M);
        else vg_fill_targets(tile + p, sh.S, r, src, g, K);
    }
    __syncthreads();
    vg_store_tile(tile, out + ((long long)b * g.N + p0) * g.C, n, g.C, sh.S, tid);
}

// every geometry: one thread per output float.  grid (x, B), grid-stride over the N C floats of a sample.
template <int MODE, class POL>
__global__ __launch_bounds__(256) void vg_elem_kernel(const unsigned long long* __restrict__ table, int ld, POL pol, float* __restrict__ out,
                                                      float* __restrict__ mask, VgGeom g, int K) {
    const int b = blockIdx.y;
    typename POL::Item it;
    const VgRow r = vg_row<MODE>(table, ld, b, g, mask, pol, &it);
    const long long total = (long long)g.N * g.C;
    float* dst = out + (long long)b * total;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
        const int p = (int)(e / g.C), c = (int)(e - (long long)p * g.C);
        int i, j, k;
        vg_unflat(p, g, &i, &j, &k);
        dst[e] = POL::template value<MODE>(r, it, i, j, k, c, g, K);
    }
}

// One call, one launch, one count of `counter`.  The tiled kernel (tile4 where MODE 0 meets M == 4, else tile0; `tiles` workgroups per sample,
// shape argument sh) runs when C <= 32, the output is 16-byte aligned and `whole` -- its rows of floats end on 16-byte stores; any other
// geometry, and every one under debug_volgen, runs the element kernel.
template <int MODE, class POL, class KERNEL, class SHAPE>
int vg_launch(int counter, bool whole, unsigned tiles, KERNEL tile4, KERNEL tile0, SHAPE sh, const unsigned long long* table, int ld, POL pol, float* out,
              float* mask, const VgGeom& g, int K, int B, hipStream_t s) {
    const long long total = (long long)g.N * g.C;
    const bool tiled = !mrdis_opt(MRDIS_OPT_VOLGEN) && g.C <= VG_MAXC_TILE && whole && (((uintptr_t)out) & 15) == 0;
    mrdis_count(counter);
    if (tiled) {
        const KERNEL kernel = (MODE == 0 && g.M == 4) ? tile4 : tile0;
        MRDIS_LAUNCH(kernel, dim3(tiles, B), dim3(256), 0, s, table, ld, pol, out, mask, g, K, sh);
    } else {
        long long gx = (total + 255) / 256; if (gx > 4096) gx = 4096;
        MRDIS_LAUNCH((vg_elem_kernel<MODE, POL>), dim3((unsigned)gx, B), dim3(256), 0, s, table, ld, pol, out, mask, g, K);
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

// the gathers on the flat tile: inputs with the mask (mode 0), or targets
template <class POL>
int vg_gather(int counter, const void* table, int ld, POL pol, float* out, float* mask, const VgGeom& g, int mode, int K, int B, void* stream) {
    const unsigned long long* t = reinterpret_cast<const unsigned long long*>(table);
    const VgFlat sh = vg_tile_shape(g.C);
    const bool whole = (((long long)g.N * g.C) & 3) == 0;
    const unsigned tiles = mrdis_cdiv(g.N, sh.P);
    return mode == 0 ? vg_launch<0>(counter, whole, tiles, vg_tile_kernel<0, 4, POL>, vg_tile_kernel<0, 0, POL>, sh, t, ld, pol, out, mask, g, 0, B, (hipStream_t)stream)
                     : vg_launch<1>(counter, whole, tiles, vg_tile_kernel<1, 0, POL>, vg_tile_kernel<1, 0, POL>, sh, t, ld, pol, out, nullptr, g, K, B, (hipStream_t)stream);
}
}  // namespace
