// Rotated and zoomed training patches for the 3-D nets: mrdis_patch_gather (mrdis_patch.hip) with an affine resampling of the samples whose
// warp bit is set.  THIS PACKAGE'S CONVENTIONS -- the reference has no spatial augmentation.  One entry point, mrdis_patch_warp.
//
// All coordinates are integers.  The host rounds A = (R_h R_w R_d) / zoom once to Q16 (patch3d.warp_matrix) and the kernel evaluates, in units
// of 2^-17 voxel and in 64 bits,
//     s[r] = ((2 origin[r] + P[r] - 1) << 16) + sum_c a[r][c] (2 o'[c] - (P[c] - 1))          o' = the output index after the flip rule
//     floor index i0 = s >> 17,  fraction f = s & (2^17 - 1),  nearest index = (s + 2^16) >> 17
// so which label a voxel takes, and where the background marker lands, never depends on a float rounding; only the trilinear weights
// f / 2^17 (exact in fp32) meet the intensities.  i0, i0 + 1 and the nearest index are clamped per axis into the volume (edge replication,
// nothing is padded), after the origins (as in mrdis_patch.hip) and the matrix entries (to +-2^18 = +-4.0): no table can send a read outside.
//
//   targets  the raw label at the nearest index, then vg_label's relabel and vg_target's region channels
//   inputs   per contrast (an absent one reads 0 everywhere), m0 = vg_item_min of the WHOLE volumes as in mrdis_patch.hip.  With the augment
//            bit: -10 exactly where the nearest voxel equals m0; elsewhere every corner that equals m0 takes the nearest voxel's value (the
//            background marker never bleeds into tissue), the eight corners are interpolated along d, then w, then h as a + t (b - a) --
//            three fp32 roundings each, never a fused multiply-add -- and x * scale + shift follows with vg_input's two roundings.
//            Without the augment bit: the interpolated raw corners.
// A sample with the warp bit clear takes mrdis_patch_gather's rules (vg_input / vg_label at origin + o'), bit for bit.
//
// Table row (64-bit words, ld >= 2 M + 12): the 2 M + 7 words of mrdis_patch.hip, flag word [2M+1] bit 6 = warp, then [2M+7 .. 2M+11] the nine
// Q16 entries, row-major, two int32 per word, the low half first.
//
// Shape of the tiled kernel.  A workgroup owns a compact BH x BW x BD brick of the output patch (8 x 8 x 16 at C <= 8), not a flat run of
// positions: a flat run of 1024 positions is 8 (h, w) columns of a 128-deep patch, whose source under a 30 degree rotation is eight slanted
// lines 128 voxels long; the brick's source is a box about 1.4 / zoom times its own size, a few cache lines wide on every axis, so the eight
// corner loads of neighbouring lanes and of the workgroup's four passes hit lines the vector cache already holds.  The source neighbourhood is
// read through the caches, not staged in LDS (the rotated box has no fixed extent and its rows no fixed alignment, and the L1 /
// L2 hit rates make the loads cheaper than a staging pass would be).  Lanes run along the brick's flat position q = (bi BW + bj) BD + bk; the
// values land in the [C][S] LDS tile of mrdis_volgather.h as row c, position q, and leave through vg_store_tile one brick row (BD positions x C
// channels, contiguous in the output) per group of BD C / 4 lanes: 16-byte stores, channel fastest.  The warp flag is uniform per workgroup
// (blockIdx.y is the sample): a sample without it takes the straight-copy branch, one load per voxel and contrast.
#include "mrdis_volgather.h"

namespace {
constexpr int WP_FLAG = MRDIS_PATCH_WARP_FLAG;
constexpr int WP_AMAX = 1 << 18;            // |a[r][c]| on the device: 4.0 in Q16 (the host makes at most 2.0: zoom >= 0.5)

struct WpBrick { int lbh, lbw, lbd, nbw, nbd, S; };       // log2 of the brick extents; bricks along w and d; the tile's row stride

// a patch (VgItem: the clamped origin and the flips), whether it is resampled, and its matrix
struct WpItem : VgItem { bool warp; int a[9]; };
// the eight corner offsets (bit 2: h + 1, bit 1: w + 1, bit 0: d + 1), the nearest voxel's offset and the three weights
struct WpSrc { long long c[8]; long long n; float th, tw, td; };

__device__ __forceinline__ int wp_clamp64(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

__device__ __forceinline__ WpSrc wp_src(int i, int j, int k, const VgGeom& g, const WpItem& it) {
    const int P[3] = {g.PH, g.PW, g.PD}, dim[3] = {g.H, g.W, g.D};
    const int op[3] = {it.fh ? g.PH - 1 - i : i, it.fw ? g.PW - 1 - j : j, it.fd ? g.PD - 1 - k : k};
    long long t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = 2LL * op[c] - (P[c] - 1);
    int lo[3], hi[3], nr[3];
    float w[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        // |a| <= 2^18 and |t| < 2^32: every term below 2^50
        const long long s = ((2LL * it.o[r] + P[r] - 1) << 16) + it.a[3 * r] * t[0] + it.a[3 * r + 1] * t[1] + it.a[3 * r + 2] * t[2];
        const long long i0 = s >> 17;
        lo[r] = wp_clamp64(i0, dim[r] - 1); hi[r] = wp_clamp64(i0 + 1, dim[r] - 1); nr[r] = wp_clamp64((s + 65536) >> 17, dim[r] - 1);
        w[r] = (float)(int)(s & 131071) * (1.f / 131072.f);
    }
    WpSrc src;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        src.c[c] = ((long long)((c & 4) ? hi[0] : lo[0]) * g.W + ((c & 2) ? hi[1] : lo[1])) * g.D + ((c & 1) ? hi[2] : lo[2]);
    src.n = ((long long)nr[0] * g.W + nr[1]) * g.D + nr[2];
    src.th = w[0]; src.tw = w[1]; src.td = w[2];
    return src;
}

struct WpVals { float c[8]; float n; };
__device__ __forceinline__ WpVals wp_fetch(const float* vol, const WpSrc& src) {
    WpVals v;
#pragma unroll
    for (int c = 0; c < 8; ++c) v.c[c] = vol ? vol[src.c[c]] : 0.f;
    v.n = vol ? vol[src.n] : 0.f;
    return v;
}
__device__ __forceinline__ float wp_lerp(float a, float b, float t) {
#pragma clang fp contract(off)              // three roundings: the difference, the product, the sum
    const float d = b - a;
    const float p = t * d;
    return a + p;
}
__device__ __forceinline__ float wp_input(WpVals v, const WpSrc& src, bool aug, float scale, float shift, float m0) {
#pragma clang fp contract(off)
    if (aug) {
        if (v.n == m0) return -10.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) v.c[c] = v.c[c] == m0 ? v.n : v.c[c];
    }
    const float x00 = wp_lerp(v.c[0], v.c[1], src.td), x01 = wp_lerp(v.c[2], v.c[3], src.td);
    const float x10 = wp_lerp(v.c[4], v.c[5], src.td), x11 = wp_lerp(v.c[6], v.c[7], src.td);
    const float y0 = wp_lerp(x00, x01, src.tw), y1 = wp_lerp(x10, x11, src.tw);
    const float x = wp_lerp(y0, y1, src.th);
    if (!aug) return x;
    const float xs = x * scale;
    return xs + shift;
}
__device__ __forceinline__ float wp_row_input(const VgRow& r, int m, const WpSrc& src) {
    return wp_input(wp_fetch(reinterpret_cast<const float*>(r.w[m]), src), src, r.aug, r.scale, r.shift, r.m0);
}

// The position-to-source policy of this entry point (mrdis_volgather.h): VgPatch's box, a row with the warp bit resampled.  The matrix
// entries are clamped as the origins are.
struct WpWarp : VgPatch {
    typedef WpItem Item;
    __device__ __forceinline__ Item item(const VgRow& r, int b, const VgGeom& g) const {
        Item it;
        static_cast<VgItem&>(it) = VgPatch::item(r, b, g);
        it.warp = r.flags & (unsigned)WP_FLAG;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const unsigned long long w = r.w[2 * g.M + 7 + (e >> 1)];
            const int v = (int)(unsigned)((e & 1) ? (w >> 32) : (w & 0xffffffffull));
            it.a[e] = v < -WP_AMAX ? -WP_AMAX : (v > WP_AMAX ? WP_AMAX : v);
        }
        return it;
    }
    template <int MODE>
    static __device__ __forceinline__ float value(const VgRow& r, const Item& it, int i, int j, int k, int c, const VgGeom& g, int K) {
        if (!it.warp) return VgCopy::value<MODE>(r, it, i, j, k, c, g, K);
        const WpSrc src = wp_src(i, j, k, g, it);
        if (MODE == 0) return wp_row_input(r, c, src);
        return vg_target(vg_label(r.seg, src.n, g.relabel), c, K);
    }
};

// MODE 0: inputs (C = M), MODE 1: targets (C = max(K, 1)).  grid (bricks, B), 256 threads; (PD C) % 4 == 0, out 16-byte aligned.
// CM = 4: M == 4 (the BraTS set) with the 36 loads of a position issued together; CM = 0: M at run time.
template <int MODE, int CM>
__global__ __launch_bounds__(256) void patchwarp_tile_kernel(const unsigned long long* __restrict__ table, int ld, WpWarp pol, float* __restrict__ out,
                                                             float* __restrict__ mask, VgGeom g, int K, WpBrick br) {
    __shared__ float tile[VG_LDS_FLOATS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int BD = 1 << br.lbd, BW = 1 << br.lbw, P = 1 << (br.lbh + br.lbw + br.lbd), S = br.S;
    // the brick of this workgroup: d fastest
    const int xd = blockIdx.x % br.nbd, xq = blockIdx.x / br.nbd;
    const int i0 = (xq / br.nbw) << br.lbh, j0 = (xq % br.nbw) << br.lbw, k0 = xd << br.lbd;
    WpItem it;
    const VgRow r = vg_row<MODE>(table, ld, b, g, mask, pol, &it);
    for (int q = tid; q < P; q += 256) {
        const int i = i0 + (q >> (br.lbd + br.lbw)), j = j0 + ((q >> br.lbd) & (BW - 1)), k = k0 + (q & (BD - 1));
        if (i >= g.PH || j >= g.PW || k >= g.PD) continue;
        if (MODE == 1) {
            vg_fill_targets(tile + q, S, r, it.warp ? wp_src(i, j, k, g, it).n : vg_copy_src(i, j, k, g, it), g, K);
        } else if (!it.warp) {
            vg_fill_inputs<CM>(tile + q, S, r, vg_copy_src(i, j, k, g, it), g.M);
        } else {
            const WpSrc src = wp_src(i, j, k, g, it);
            if (CM > 0) {
                WpVals v[CM > 0 ? CM : 1];
#pragma unroll
                for (int m = 0; m < CM; ++m) v[m] = wp_fetch(reinterpret_cast<const float*>(r.w[m]), src);
#pragma unroll
                for (int m = 0; m < CM; ++m) tile[m * S + q] = wp_input(v[m], src, r.aug, r.scale, r.shift, r.m0);
            } else {
                for (int m = 0; m < g.M; ++m) tile[m * S + q] = wp_row_input(r, m, src);
            }
        }
    }
    __syncthreads();
    // store phase: brick row r = (bi, bj) is BD consecutive positions of the tile and kn C consecutive floats of the output; tpr lanes per row,
    // each at most one 16-byte store per pass (vg_store_tile's loop runs once: kn C / 4 <= tpr <= 256)
    const int tpr = (BD * g.C) >> 2, rpp = 256 / tpr, rows = P >> br.lbd;
    const int kn = g.PD - k0 < BD ? g.PD - k0 : BD;
    const int rsub = tid / tpr, lane = tid - rsub * tpr;
    if (rsub < rpp) {
        for (int rw = rsub; rw < rows; rw += rpp) {
            const int i = i0 + (rw >> br.lbw), j = j0 + (rw & (BW - 1));
            if (i < g.PH && j < g.PW)
                vg_store_tile(tile + (rw << br.lbd), out + ((long long)b * g.N + ((long long)i * g.PW + j) * g.PD + k0) * g.C, kn, g.C, S, lane);
        }
    }
}

int wp_log2(int v) { int l = 0; while ((2 << l) <= v) ++l; return l; }

// the brick and the tile stride for C channels: P = 1024 positions at C <= 8, 512 at C <= 16, 256 at C <= 32 (powers of two within
// vg_tile_shape's P, with its padding); rows of 16 positions along d, longer ones under four channels while the patch is that deep, so that a
// row of the output stays 256 bytes or more; the (h, w) extents as square as powers of two get
WpBrick wp_brick(const VgGeom& g) {
    const VgFlat flat = vg_tile_shape(g.C);
    const int P = 1 << wp_log2(flat.P);
    int lbd = 4;
    if (g.C < 4) while (lbd < 6 && (1 << lbd) < g.PD) ++lbd;
    const int lrows = wp_log2(P) - lbd;
    WpBrick br;
    br.lbd = lbd; br.lbh = lrows / 2; br.lbw = lrows - lrows / 2;
    br.nbw = mrdis_cdiv(g.PW, 1 << br.lbw); br.nbd = mrdis_cdiv(g.PD, 1 << lbd);
    br.S = P + (flat.S - flat.P);
    return br;
}
}  // namespace

extern "C" int mrdis_patch_warp(const void* table, int ld_table, const int* origins, float* out, float* mask, int B, int M, int H, int W, int D,
                                int PH, int PW, int PD, int mode, int K, int relabel, void* stream) {
    VgGeom g;
    const int rc = vg_check(origins != nullptr, table, out, ld_table, 12, B, M, H, W, D, PH, PW, PD, mode, K, relabel, &g);
    if (rc != MRDIS_OK) return rc;
    WpWarp pol;
    pol.origins = origins;
    const unsigned long long* t = reinterpret_cast<const unsigned long long*>(table);
    const WpBrick br = wp_brick(g);
    const unsigned bricks = (unsigned)((long long)mrdis_cdiv(g.PH, 1 << br.lbh) * br.nbw * br.nbd);
    // a brick row is (PD - k0) C floats with k0 % 16 == 0: whole 16-byte stores need (PD C) % 4 == 0 (which implies (N C) % 4 == 0)
    const bool whole = (((long long)g.PD * g.C) & 3) == 0;
    return mode == 0 ? vg_launch<0>(MRDIS_CNT_PATCHWARP, whole, bricks, patchwarp_tile_kernel<0, 4>, patchwarp_tile_kernel<0, 0>, br, t, ld_table, pol, out, mask, g, 0, B,
                                    (hipStream_t)stream)
                     : vg_launch<1>(MRDIS_CNT_PATCHWARP, whole, bricks, patchwarp_tile_kernel<1, 0>, patchwarp_tile_kernel<1, 0>, br, t, ld_table, pol, out, nullptr, g, K, B,
                                    (hipStream_t)stream);
}
