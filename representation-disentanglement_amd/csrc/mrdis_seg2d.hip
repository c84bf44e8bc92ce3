// Whole-subject tumour segmentation by the 2-D model (segment.segment_volumes): the output decoder's logits of a batch of consecutive centre
// slices become label planes of one volume per missing-contrast pattern ("set"), and the planes become the store's (H, W, D) volumes.  The
// label rule is this package's own convention: the reference assembles no volume and never fuses for M > 1.
//   mrdis_seg2d_label_planes   planes[s][s0 + r][h][w] = label of pixel (h, w) of sample r of set s          one launch per batch, all sets
//        one view:   argmax_c y_c over the logits themselves, the lowest c on a tie
//        two views:  p_c = 0.5 (softmax(y^0)_c + softmax(y^1)_c), each softmax exp(y_c - max) / sum in fp32 (accurate expf, IEEE division, the
//                    sum in increasing c); argmax_c p_c, the lowest c on a tie.  View v is read at the pixel mirrored per flips[v]: it is the
//                    prediction of a flipped input, un-flipped here
//        class c is written as label c, a 3 as 4 with `relabel`
//   mrdis_seg2d_finish         out[s][h][w][d] = planes[s][d][h][w]                                             one launch per subject, all sets
// The torch composition (flip, softmax, mean, argmax, relabel, cast, slice store per pattern; permute + contiguous) makes five to nine passes per
// pattern and launches per pattern; here a batch costs one read of the logits and one store of a byte per pixel, whatever the number of sets.
// No atomics and every output byte has one owner: two runs give the same bits.
//
// label_planes: a workgroup owns SL_PIX consecutive pixels of one (set, sample); a lane takes pixel j * SL_THREADS + lane of them, j = 0 .. 3, so
// every load instruction of a wave covers 64 consecutive pixels -- 1 KB of one 16-byte load per lane when C == 4 and the view is 16-byte
// aligned, else C 4-byte loads per lane over 256 C contiguous bytes (a W flip walks the same bytes downwards) -- and every store instruction
// writes 64 consecutive bytes of a plane row.  The four pixels of a lane are independent: up to eight 16-byte loads in flight per lane.  The
// kernel is a byte mover: 16 n_views bytes read per byte written (C = 4); the softmax of a view is C accurate expf and C divisions.  Workgroup ids are
// laid out tile-fastest and remapped per XCD (mrdis_xcd_remap), so the tiles whose output rows meet in one 128-byte line mostly share an L2.
//
// finish transposes through LDS like synth_finish_kernel: a workgroup takes SF2_TP consecutive pixels and up to SF2_DC planes, reads plane by
// plane (64 contiguous bytes per wave), parks the bytes in an LDS tile (row stride SF2_TP + 4 bytes = 17 words: the column reads of 32 lanes fall on
// 32 different banks), and streams the tile out along (H, W, D): with D <= SF2_DC (BraTS: 155) the SF2_TP pixels' D-runs are ONE contiguous run
// of SF2_TP D bytes whatever D % 4 is; a deeper volume goes in chunks of SF2_DC planes.
#include "mrdis_common.h"

namespace {
constexpr int SL_THREADS = 256;
constexpr int SL_PER = 4;                    // pixels per lane
constexpr int SL_PIX = SL_THREADS * SL_PER;  // pixels per workgroup
constexpr int SF2_THREADS = 256;
constexpr int SF2_TP = 64;                   // pixels per finish tile
constexpr int SF2_DC = 160;                  // planes per finish tile: 160 x 68 bytes = 10.6 KB of LDS
constexpr int SF2_RS = SF2_TP + 4;           // row stride of the tile, bytes

struct Seg2dViews { const float* p[MRDIS_SEG2D_MAX_SETS * MRDIS_SEG2D_MAX_VIEWS]; };
struct Seg2dGeom { int B, H, W, D, s0, n_sets, n_views, flip0, flip1, relabel, ntiles; long long HW; };

template <int C, bool VEC>
__device__ __forceinline__ void seg2d_load(const float* __restrict__ q, float (&y)[C]) {
    if constexpr (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(q);
        y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) y[c] = q[c];
    }
}

// y becomes softmax(y): exp(y_c - max) / sum, the sum in increasing c
template <int C>
__device__ __forceinline__ void seg2d_softmax(float (&y)[C]) {
    float m = y[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, y[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { y[c] = expf(y[c] - m); sum += y[c]; }
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = y[c] / sum;
}

// grid: n_sets * B * ntiles workgroups; logical id = (set * B + sample) * ntiles + tile
template <int C, bool VEC>
__global__ __launch_bounds__(SL_THREADS) void seg2d_label_kernel(Seg2dViews views, unsigned char* __restrict__ planes, Seg2dGeom g) {
    const int lid = mrdis_xcd_remap((int)blockIdx.x, g.n_sets * g.B * g.ntiles);
    const int q = lid / g.ntiles, tile = lid - q * g.ntiles;
    const int s = q / g.B, r = q - s * g.B;
    unsigned char* out = planes + ((long long)s * g.D + g.s0 + r) * g.HW;
    const float* v0 = views.p[s * g.n_views];
    const float* v1 = views.p[s * g.n_views + g.n_views - 1];       // the same view when there is one
    const long long base = (long long)r * g.HW;
#pragma unroll
    for (int j = 0; j < SL_PER; ++j) {
        const long long p = (long long)tile * SL_PIX + j * SL_THREADS + threadIdx.x;
        if (p >= g.HW) break;
        const int h = (int)(p / g.W), w = (int)(p - (long long)h * g.W);
        const int h0 = g.flip0 == 1 ? g.H - 1 - h : h, w0 = g.flip0 == 2 ? g.W - 1 - w : w;
        float y[C];
        seg2d_load<C, VEC>(v0 + (base + (long long)h0 * g.W + w0) * C, y);
        if (g.n_views == 2) {                                        // wave-uniform
            const int h1 = g.flip1 == 1 ? g.H - 1 - h : h, w1 = g.flip1 == 2 ? g.W - 1 - w : w;
            float z[C];
            seg2d_load<C, VEC>(v1 + (base + (long long)h1 * g.W + w1) * C, z);
            seg2d_softmax<C>(y);
            seg2d_softmax<C>(z);
#pragma unroll
            for (int c = 0; c < C; ++c) y[c] = 0.5f * (y[c] + z[c]);
        }
        int best = 0;
        float top = y[0];
#pragma unroll
        for (int c = 1; c < C; ++c)
            if (y[c] > top) { top = y[c]; best = c; }               // strictly above: the lowest c keeps a tie
        if (g.relabel && best == 3) best = 4;
        out[p] = (unsigned char)best;
    }
}

// grid: n_sets * ntiles_p * nchunk workgroups; logical id = (set * ntiles_p + pixel tile) * nchunk + chunk of SF2_DC planes
__global__ __launch_bounds__(SF2_THREADS) void seg2d_finish_kernel(const unsigned char* __restrict__ planes, unsigned char* __restrict__ out, int D,
                                                                   long long HW, int ntiles_p, int nchunk, int nblk) {
    __shared__ unsigned char tile[SF2_DC * SF2_RS];
    const int lid = mrdis_xcd_remap((int)blockIdx.x, nblk);
    const int q = lid / nchunk, ch = lid - q * nchunk;
    const int s = q / ntiles_p, tp = q - s * ntiles_p;
    const long long p0 = (long long)tp * SF2_TP;
    const int d0 = ch * SF2_DC;
    const int dn = min(SF2_DC, D - d0);
    const int pn = (int)min((long long)SF2_TP, HW - p0);
    const unsigned char* src = planes + (long long)s * D * HW;
    unsigned char* dst = out + (long long)s * D * HW;
    const int tx = threadIdx.x & (SF2_TP - 1), ty = threadIdx.x / SF2_TP;
    if (tx < pn) {
        for (int dd = ty; dd < dn; dd += SF2_THREADS / SF2_TP) tile[dd * SF2_RS + tx] = src[(long long)(d0 + dd) * HW + p0 + tx];
    }
    __syncthreads();
    // out[(p0 + py) * D + d0 + dd]: consecutive threads along dd, then py
    const int n = pn * dn;
    for (int i = threadIdx.x; i < n; i += SF2_THREADS) {
        const int py = i / dn, dd = i - py * dn;
        dst[(p0 + py) * D + d0 + dd] = tile[dd * SF2_RS + py];
    }
}

template <int C>
void launch_seg2d_label(const Seg2dViews& vs, bool vec, unsigned char* planes, const Seg2dGeom& g, unsigned nblk, hipStream_t s) {
    if constexpr (C == 4) {
        if (vec) {
            MRDIS_LAUNCH((seg2d_label_kernel<4, true>), dim3(nblk), dim3(SL_THREADS), 0, s, vs, planes, g);
            return;
        }
    }
    MRDIS_LAUNCH((seg2d_label_kernel<C, false>), dim3(nblk), dim3(SL_THREADS), 0, s, vs, planes, g);
}
}  // namespace

extern "C" int mrdis_seg2d_label_planes(const float* const* views, int n_sets, int n_views, const int* flips, unsigned char* planes, int B, int C,
                                        int H, int W, int D, int s0, int relabel, void* stream) {
    if (n_sets < 1 || n_sets > MRDIS_SEG2D_MAX_SETS || n_views < 1 || n_views > MRDIS_SEG2D_MAX_VIEWS || C < 2 || C > 4) return MRDIS_EINVAL;
    if (B < 1 || H < 1 || W < 1 || D < 1 || s0 < 0 || (long long)s0 + B > D || (long long)H * W >= (1LL << 31)) return MRDIS_EINVAL;
    if (!views || !flips || !planes) return MRDIS_EINVAL;
    for (int v = 0; v < n_views; ++v)
        if (flips[v] < 0 || flips[v] > 2) return MRDIS_EINVAL;
    Seg2dViews vs;
    bool vec = C == 4;
    const int n = n_sets * n_views;
    for (int k = 0; k < MRDIS_SEG2D_MAX_SETS * MRDIS_SEG2D_MAX_VIEWS; ++k) {
        vs.p[k] = views[k < n ? k : 0];
        if (!vs.p[k]) return MRDIS_EINVAL;
        if ((((uintptr_t)vs.p[k]) & 3) != 0) return MRDIS_EALIGN;
        if ((((uintptr_t)vs.p[k]) & 15) != 0) vec = false;
    }
    Seg2dGeom g;
    g.B = B; g.H = H; g.W = W; g.D = D; g.s0 = s0; g.n_sets = n_sets; g.n_views = n_views; g.flip0 = flips[0]; g.flip1 = flips[n_views - 1];
    g.relabel = relabel ? 1 : 0; g.HW = (long long)H * W;
    const long long ntiles = (g.HW + SL_PIX - 1) / SL_PIX;
    const long long nblk = ntiles * B * n_sets;
    if (nblk >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    g.ntiles = (int)ntiles;
    hipStream_t s = (hipStream_t)stream;
    mrdis_count(MRDIS_CNT_SEG2DLABELS);
    switch (C) {
        case 2: launch_seg2d_label<2>(vs, vec, planes, g, (unsigned)nblk, s); break;
        case 3: launch_seg2d_label<3>(vs, vec, planes, g, (unsigned)nblk, s); break;
        default: launch_seg2d_label<4>(vs, vec, planes, g, (unsigned)nblk, s); break;
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_seg2d_finish(const unsigned char* planes, unsigned char* out, int n_sets, int D, int H, int W, void* stream) {
    if (!planes || !out || n_sets < 1 || D < 1 || H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return MRDIS_EINVAL;
    const long long HW = (long long)H * W;
    const int nchunk = mrdis_cdiv(D, SF2_DC);
    const long long ntiles_p = (HW + SF2_TP - 1) / SF2_TP;
    const long long nblk = ntiles_p * nchunk * n_sets;
    if (nblk >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    mrdis_count(MRDIS_CNT_SEG2DFINISH);
    MRDIS_LAUNCH(seg2d_finish_kernel, dim3((unsigned)nblk), dim3(SF2_THREADS), 0, (hipStream_t)stream, planes, out, D, HW, (int)ntiles_p, nchunk,
                 (int)nblk);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
