// Whole-subject synthesis of missing contrasts (synth.synthesize_volumes): per-voxel assembly of the input decoders' slice blocks into a volume.
//
// A decode of the 2-D model predicts the C = 2b + 1 slices centred on s, once per present source contrast.  The volume of a target contrast takes
// either the centre channel of every sample (`block: centre`) or the mean of EVERY prediction of a plane (`block: mean`: channel k - s + b of each
// sample with |k - s| <= b), averaged over the sources.  The rule is this package's own convention: the reference ships no such path.
//   mrdis_synth_accum    acc[k] += sum over (sample r ascending, its one channel c = k - s0 - r + b in [c_lo, c_hi], source ascending) of src[r][c];
//                        cnt[k] += number of those values                              one launch per batch of consecutive centres and target
//   mrdis_synth_finish   vol[d] = acc[d] / (float)cnt[d]  (IEEE fp32 division; `fill` where cnt[d] == 0), in place in (D, H, W) and transposed
//                        into the store's (H, W, D)                                      one launch per target
// The torch composition (index the channels, stack, mean, index_add_, divide, where, permute + contiguous) makes seven passes and several
// temporaries of the batch's size; here a batch costs one read of the channels it needs and one read-modify-write of the planes it covers.
//
// Accumulation is a GATHER: a workgroup owns one plane k of the covered range and a tile of pixels, a thread four consecutive pixels of it (one where H W % 4 != 0), and
// adds its contributions in the fixed order above.  Within a launch exactly one thread owns an acc element and there are no atomics, so batches add
// in launch order and two runs give the same bits.  Access: the sources are channels-last, so the channel a plane needs sits at a stride of C
// floats from pixel to pixel -- inherent to the decoders' layout.  A wave's 4-byte loads of one (sample, channel, source) therefore touch C times
// the lines they use; in mean mode the planes k - b .. k + b use the other channels of the very same lines, so the workgroup ids are laid out
// plane-fastest inside a tile and remapped per XCD (mrdis_xcd_remap): the 2b + 1 workgroups that share a line mostly run on one XCD, close in
// time, and the line comes from that L2.  In centre mode one channel in C is used and the rest of each line is fetched for nothing.  acc itself is
// read and written 16 bytes per lane where H W % 4 == 0 (aligned planes), else 4 bytes per lane.
//
// Finish transposes through LDS: a workgroup takes SF_TP consecutive pixels and up to SF_DC planes, reads acc plane by plane (128 contiguous bytes
// per half wave), writes the quotient back in place, parks it in an LDS tile (row stride SF_TP + 1 words: both phases conflict-free), and then
// streams the tile out along the (H, W, D) order: with D <= SF_DC (BraTS: 155) the SF_TP pixels' D-runs are ONE contiguous run of SF_TP D floats,
// whatever D % 4 is, so the ragged depth costs nothing; a deeper volume goes in chunks of SF_DC planes (runs of 640 bytes).
#include "mrdis_common.h"

namespace {
constexpr int SA_THREADS = 256;
constexpr int SF_THREADS = 256;
constexpr int SF_TP = 32;                    // pixels per finish tile
constexpr int SF_DC = 160;                   // planes per finish tile: 160 x 33 words = 21 KB of LDS

struct SynthSrc { const float* p[MRDIS_SYNTH_MAX_SRC]; };
struct SynthGeom { int B, C, D, s0, b, c_lo, c_hi, k0, nplanes, ntiles, n_src; long long HW; };

// grid: nplanes * ntiles workgroups; logical id = tile * nplanes + (k - k0)
template <int VEC>
__global__ __launch_bounds__(SA_THREADS) void synth_accum_kernel(SynthSrc src, float* __restrict__ acc, int* __restrict__ cnt, SynthGeom g) {
    const int lid = mrdis_xcd_remap((int)blockIdx.x, g.nplanes * g.ntiles);
    const int tile = lid / g.nplanes;
    const int k = g.k0 + (lid - tile * g.nplanes);
    if (k < 0 || k >= g.D) return;                                   // a plane the batch predicts but the volume does not have
    // sample r (centre s0 + r) predicts plane k with its channel c = k - s0 - r + b; c in [c_lo, c_hi]
    const int kk = k - g.s0 + g.b;
    const int r_lo = max(0, kk - g.c_hi), r_hi = min(g.B - 1, kk - g.c_lo);
    if (r_lo > r_hi) return;
    if (tile == 0 && threadIdx.x == 0) cnt[k] += (r_hi - r_lo + 1) * g.n_src;
    const long long p = ((long long)tile * SA_THREADS + threadIdx.x) * VEC;
    if (p >= g.HW) return;
    float* dst = acc + (long long)k * g.HW + p;
    float a[VEC];
    if constexpr (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(dst);
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    } else {
        a[0] = *dst;
    }
    for (int r = r_lo; r <= r_hi; ++r) {
        const long long off = ((long long)r * g.HW + p) * g.C + (kk - r);
#pragma unroll
        for (int j = 0; j < MRDIS_SYNTH_MAX_SRC; ++j) {
            if (j < g.n_src) {                                       // wave-uniform
                const float* q = src.p[j] + off;
#pragma unroll
                for (int v = 0; v < VEC; ++v) a[v] += q[(long long)v * g.C];
            }
        }
    }
    if constexpr (VEC == 4) {
        f32x4 v;
        v.x = a[0]; v.y = a[1]; v.z = a[2]; v.w = a[3];
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        *dst = a[0];
    }
}

// grid: ntiles_p * nchunk workgroups; workgroup = (pixel tile, chunk of SF_DC planes)
__global__ __launch_bounds__(SF_THREADS) void synth_finish_kernel(float* __restrict__ acc, const int* __restrict__ cnt, float* __restrict__ out,
                                                                  int D, long long HW, int nchunk, float fill) {
    __shared__ float tile[SF_DC][SF_TP + 1];
    const int tp = (int)blockIdx.x / nchunk, ch = (int)blockIdx.x - tp * nchunk;
    const long long p0 = (long long)tp * SF_TP;
    const int d0 = ch * SF_DC;
    const int dn = min(SF_DC, D - d0);
    const int pn = (int)min((long long)SF_TP, HW - p0);
    const int tx = threadIdx.x & (SF_TP - 1), ty = threadIdx.x / SF_TP;
    if (tx < pn) {
        for (int dd = ty; dd < dn; dd += SF_THREADS / SF_TP) {
            float* a = acc + (long long)(d0 + dd) * HW + p0 + tx;
            const int c = cnt[d0 + dd];
            const float v = c > 0 ? *a / (float)c : fill;            // IEEE division; the count converts exactly (< 2^24)
            *a = v;
            tile[dd][tx] = v;
        }
    }
    __syncthreads();
    // out[(p0 + py) * D + d0 + dd]: consecutive threads along dd, then py
    const int n = pn * dn;
    for (int i = threadIdx.x; i < n; i += SF_THREADS) {
        const int py = i / dn, dd = i - py * dn;
        out[(p0 + py) * D + d0 + dd] = tile[dd][py];
    }
}
}  // namespace

extern "C" int mrdis_synth_accum(const float* const* srcs, int n_src, float* acc, int* cnt, int B, int C, int H, int W, int D, int s0, int c_lo,
                                 int c_hi, void* stream) {
    if (!srcs || !acc || !cnt || n_src < 1 || n_src > MRDIS_SYNTH_MAX_SRC || B < 1 || C < 1 || (C & 1) == 0 || H < 1 || W < 1 || D < 1) return MRDIS_EINVAL;
    if (c_lo < 0 || c_hi < c_lo || c_hi >= C) return MRDIS_EINVAL;
    if ((long long)H * W >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    SynthSrc ss;
    for (int j = 0; j < MRDIS_SYNTH_MAX_SRC; ++j) {
        ss.p[j] = srcs[j < n_src ? j : 0];
        if (!ss.p[j]) return MRDIS_EINVAL;
        if ((((uintptr_t)ss.p[j]) & 3) != 0) return MRDIS_EALIGN;
    }
    if ((((uintptr_t)acc) & 3) != 0 || (((uintptr_t)cnt) & 3) != 0) return MRDIS_EALIGN;
    SynthGeom g;
    g.B = B; g.C = C; g.D = D; g.s0 = s0; g.b = (C - 1) / 2; g.c_lo = c_lo; g.c_hi = c_hi; g.n_src = n_src; g.HW = (long long)H * W;
    g.k0 = s0 + c_lo - g.b;                                          // first and number of planes this batch predicts
    g.nplanes = B + (c_hi - c_lo);
    const bool vec = (g.HW & 3) == 0 && (((uintptr_t)acc) & 15) == 0;
    const long long per = (long long)SA_THREADS * (vec ? 4 : 1);
    const long long ntiles = (g.HW + per - 1) / per;
    if (ntiles * g.nplanes >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    g.ntiles = (int)ntiles;
    hipStream_t s = (hipStream_t)stream;
    mrdis_count(MRDIS_CNT_SYNTHACCUM);
    if (vec) MRDIS_LAUNCH(synth_accum_kernel<4>, dim3(g.nplanes * g.ntiles), dim3(SA_THREADS), 0, s, ss, acc, cnt, g);
    else MRDIS_LAUNCH(synth_accum_kernel<1>, dim3(g.nplanes * g.ntiles), dim3(SA_THREADS), 0, s, ss, acc, cnt, g);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_synth_finish(float* acc, const int* cnt, float* out, int D, int H, int W, float fill, void* stream) {
    if (!acc || !cnt || !out || D < 1 || H < 1 || W < 1) return MRDIS_EINVAL;
    if ((((uintptr_t)acc) | ((uintptr_t)cnt) | ((uintptr_t)out)) & 3) return MRDIS_EALIGN;
    const long long HW = (long long)H * W;
    const int nchunk = mrdis_cdiv(D, SF_DC);
    const long long nblk = ((HW + SF_TP - 1) / SF_TP) * nchunk;
    if (nblk >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    mrdis_count(MRDIS_CNT_SYNTHFINISH);
    MRDIS_LAUNCH(synth_finish_kernel, dim3((unsigned)nblk), dim3(SF_THREADS), 0, (hipStream_t)stream, acc, cnt, out, D, HW, nchunk, fill);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
