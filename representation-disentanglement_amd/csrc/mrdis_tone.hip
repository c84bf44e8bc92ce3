// Intensity augmentation of the gathered 3-D training patches: Gaussian blur, contrast, gamma and additive noise, behind mrdis_patch_gather /
// mrdis_patch_warp.  THIS PACKAGE'S CONVENTIONS -- the reference has no such augmentation.  Three entry points, in the order a batch takes
// them: mrdis_patch_blur (x -> y), mrdis_patch_stats (y -> stats), mrdis_patch_tone (y in place).  The rules are stated in include/mrdis.h.
//
// x / y: (B, PH, PW, PD, M) dense fp32, contrast fastest.  A voxel is background iff its value equals -10.0f exactly; background voxels leave
// every kernel as -10 and enter no sum.  Every per-batch value comes from the table block at word `col` of a row (tone3d.pack_tone), so the
// calls replay from a captured graph.
//
// Blur.  A normalised convolution: the 9-tap chains of N = m ? x : 0 and D = m along d, then w, then h, y = N / D on tissue.  A tap outside
// the patch and a background tap both contribute nothing, and fmaf(g, 0, acc) == acc exactly (acc is never -0: the chain starts from +0), so
// the kernels zero-fill instead of skipping: the same bits as the chain over the inside taps only.
//   M == 4 form, two launches (x and y 16-byte aligned): a voxel's four contrasts move as one f32x4, the taps of the four contrasts as five
//     f32x4 read from block-uniform table words.
//       tone_blur_dw4_kernel   one (b, h) plane strip per workgroup: the 16 x 32 (w, d) tile with its 4-voxel halo is staged in LDS (24 x 40
//                              f32x4), the d pass writes N1 / D1 for the 24 x 32 rows the w pass needs into LDS, the w pass writes N2 / D2 to
//                              the workspace.  40 KB of LDS: four workgroups per CU.
//       tone_blur_h4_kernel    a thread owns one (w, d) column of a 32-plane h segment and marches along h with the nine (N2, D2) pairs of its
//                              window in registers: every workspace word is read once (1.25 times with the segment halo), x once, y written once.
//     A whole halo tile of the three passes does not fit LDS at a useful size (8 x 8 x 16 outputs need 16 x 16 x 24 x 16 B of x and 16 x 16 x 16
//     x 32 B of N1 / D1, 229 KB, at six times the reads), so only the two passes that share the plane are fused.
//   generic form, three launches (every other M, a base that is only 4-byte aligned, and every shape under debug_volgen): tone_blur_axis_kernel,
//     one thread per float and pass, through two workspace pairs.  The same chains in the same order: the same bits as the M == 4 form.
// Stats.  Two launches: per-block partials (min, max, count, float64 sum: lanes, then waves, in a fixed tree), then one wave per (b, m) over
//   the partials in a fixed order.  No atomics: two runs give the same bits.
// Tone.  One launch, element-wise and in place; the noise is Philox4x32-10 on (flat voxel index, contrast) under the row's seed, so it does not
//   depend on the launch geometry.
#include "mrdis_common.h"

namespace {
constexpr int TN_R = 4;                       // tap radius
constexpr float TN_BG = -10.f;                // the background marker
constexpr int TN_BLUR = MRDIS_TONE_BLUR, TN_CONTRAST = MRDIS_TONE_CONTRAST, TN_GAMMA = MRDIS_TONE_GAMMA, TN_INVERT = MRDIS_TONE_INVERT, TN_NOISE = MRDIS_TONE_NOISE;
constexpr int TN_TONE_BITS = TN_CONTRAST | TN_GAMMA | TN_NOISE;
constexpr unsigned TN_Z_SCALE = 0x3addb446u;  // the fp32 nearest to 349520^-1/2: the standard deviation of 2 S - 4080, S a sum of 16 uniform bytes
constexpr int TN_BW = 16, TN_BD = 32;         // the (w, d) tile of tone_blur_dw4_kernel
constexpr int TN_HSEG = 32;                   // planes per h segment of tone_blur_h4_kernel
constexpr int TN_STAT_BLOCKS = 256;           // most partial blocks per sample of the statistics

// the block of a row: word 0 the seed, then per contrast ten 32-bit halves: flags, g0 .. g4, f, gamma, std, 0
__device__ __forceinline__ const unsigned* tn_block(const unsigned long long* table, int ld, int col, int b) {
    return reinterpret_cast<const unsigned*>(table + (long long)b * ld + col);
}
__device__ __forceinline__ unsigned tn_flags(const unsigned* blk, int m) { return blk[2 + 10 * m]; }
__device__ __forceinline__ float tn_word(const unsigned* blk, int m, int k) { return __uint_as_float(blk[2 + 10 * m + k]); }
// whether any contrast of the row has one of `bits`
__device__ __forceinline__ bool tn_row_has(const unsigned* blk, int M, unsigned bits) {
    unsigned any = 0;
    for (int m = 0; m < M; ++m) any |= tn_flags(blk, m);
    return (any & bits) != 0;
}

__device__ __forceinline__ f32x4 tn_fma4(f32x4 a, f32x4 b, f32x4 c) {
    f32x4 r;
    r.x = __builtin_fmaf(a.x, b.x, c.x); r.y = __builtin_fmaf(a.y, b.y, c.y); r.z = __builtin_fmaf(a.z, b.z, c.z); r.w = __builtin_fmaf(a.w, b.w, c.w);
    return r;
}
__device__ __forceinline__ f32x4 tn_tissue4(f32x4 x) {          // m as 1 / 0
    f32x4 r;
    r.x = x.x != TN_BG ? 1.f : 0.f; r.y = x.y != TN_BG ? 1.f : 0.f; r.z = x.z != TN_BG ? 1.f : 0.f; r.w = x.w != TN_BG ? 1.f : 0.f;
    return r;
}
__device__ __forceinline__ f32x4 tn_masked4(f32x4 x) {          // m ? x : 0
    f32x4 r;
    r.x = x.x != TN_BG ? x.x : 0.f; r.y = x.y != TN_BG ? x.y : 0.f; r.z = x.z != TN_BG ? x.z : 0.f; r.w = x.w != TN_BG ? x.w : 0.f;
    return r;
}
// the taps of the four contrasts, g[t] one f32x4; a contrast without the blur flag gets zeros (its sums are never read)
struct TnTaps4 { f32x4 g[TN_R + 1]; };
__device__ __forceinline__ TnTaps4 tn_taps4(const unsigned* blk) {
    TnTaps4 tp;
#pragma unroll
    for (int t = 0; t <= TN_R; ++t) {
        float v[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = (tn_flags(blk, m) & TN_BLUR) ? tn_word(blk, m, 1 + t) : 0.f;
        tp.g[t] = f32x4{v[0], v[1], v[2], v[3]};
    }
    return tp;
}

// ---------------------------------------------------------------------------------------------- blur, M == 4
// grid (tiles of a plane x PH, B), 256 threads.  ws: N2 then D2, each B N f32x4.
__global__ __launch_bounds__(256) void tone_blur_dw4_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ ws, const unsigned long long* __restrict__ table,
                                                            int ld, int col, int PH, int PW, int PD, int nbw, int nbd, long long total) {
    __shared__ f32x4 xs[TN_BW + 2 * TN_R][TN_BD + 2 * TN_R];
    __shared__ f32x4 n1[TN_BW + 2 * TN_R][TN_BD], d1[TN_BW + 2 * TN_R][TN_BD];
    const int b = blockIdx.y, tid = threadIdx.x;
    const unsigned* blk = tn_block(table, ld, col, b);
    if (!tn_row_has(blk, 4, TN_BLUR)) return;                   // uniform: the h pass copies the row
    const int per = nbw * nbd, h = blockIdx.x / per, rem = blockIdx.x - h * per;
    const int w0 = (rem / nbd) * TN_BW, d0 = (rem % nbd) * TN_BD;
    const TnTaps4 tp = tn_taps4(blk);
    const long long plane = ((long long)b * PH + h) * PW;
    const f32x4 bg = {TN_BG, TN_BG, TN_BG, TN_BG};
    for (int q = tid; q < (TN_BW + 2 * TN_R) * (TN_BD + 2 * TN_R); q += 256) {
        const int r = q / (TN_BD + 2 * TN_R), c = q - r * (TN_BD + 2 * TN_R);
        const int w = w0 - TN_R + r, d = d0 - TN_R + c;
        xs[r][c] = (w >= 0 && w < PW && d >= 0 && d < PD) ? x[(plane + w) * PD + d] : bg;       // outside the patch: contributes nothing
    }
    __syncthreads();
    for (int q = tid; q < (TN_BW + 2 * TN_R) * TN_BD; q += 256) {
        const int r = q / TN_BD, c = q - r * TN_BD;
        f32x4 an = {0.f, 0.f, 0.f, 0.f}, ad = an;
#pragma unroll
        for (int t = -TN_R; t <= TN_R; ++t) {
            const f32x4 v = xs[r][c + TN_R + t], g = tp.g[t < 0 ? -t : t];
            an = tn_fma4(g, tn_masked4(v), an);
            ad = tn_fma4(g, tn_tissue4(v), ad);
        }
        n1[r][c] = an; d1[r][c] = ad;
    }
    __syncthreads();
    for (int q = tid; q < TN_BW * TN_BD; q += 256) {
        const int r = q / TN_BD, c = q - r * TN_BD;
        const int w = w0 + r, d = d0 + c;
        if (w >= PW || d >= PD) continue;
        f32x4 an = {0.f, 0.f, 0.f, 0.f}, ad = an;
#pragma unroll
        for (int t = -TN_R; t <= TN_R; ++t) {
            const f32x4 g = tp.g[t < 0 ? -t : t];
            an = tn_fma4(g, n1[r + TN_R + t][c], an);
            ad = tn_fma4(g, d1[r + TN_R + t][c], ad);
        }
        const long long p = (plane + w) * PD + d;
        ws[p] = an; ws[total + p] = ad;
    }
}

// grid (columns / 256 x h segments, B), 256 threads: thread = one (w, d) column of one segment
__global__ __launch_bounds__(256) void tone_blur_h4_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ y, const f32x4* __restrict__ ws,
                                                           const unsigned long long* __restrict__ table, int ld, int col, int PH, int cols, int ncb, long long total) {
    const int b = blockIdx.y;
    const int seg = blockIdx.x / ncb, q = (blockIdx.x - seg * ncb) * 256 + threadIdx.x;
    if (q >= cols) return;
    const unsigned* blk = tn_block(table, ld, col, b);
    const int h0 = seg * TN_HSEG, h1 = h0 + TN_HSEG < PH ? h0 + TN_HSEG : PH;
    const long long base = (long long)b * PH * cols + q;
    if (!tn_row_has(blk, 4, TN_BLUR)) {                         // uniform: y = x
        for (int h = h0; h < h1; ++h) y[base + (long long)h * cols] = x[base + (long long)h * cols];
        return;
    }
    const TnTaps4 tp = tn_taps4(blk);
    bool on[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) on[m] = tn_flags(blk, m) & TN_BLUR;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 wn[2 * TN_R + 1], wd[2 * TN_R + 1];                   // the window: planes h - 4 .. h + 4
#pragma unroll
    for (int t = 0; t < 2 * TN_R; ++t) {
        const int hh = h0 - TN_R + t;
        const bool in = hh >= 0 && hh < PH;
        wn[t + 1] = in ? ws[base + (long long)hh * cols] : zero;
        wd[t + 1] = in ? ws[total + base + (long long)hh * cols] : zero;
    }
    for (int h = h0; h < h1; ++h) {
#pragma unroll
        for (int t = 0; t < 2 * TN_R; ++t) { wn[t] = wn[t + 1]; wd[t] = wd[t + 1]; }
        const int hh = h + TN_R;
        wn[2 * TN_R] = hh < PH ? ws[base + (long long)hh * cols] : zero;
        wd[2 * TN_R] = hh < PH ? ws[total + base + (long long)hh * cols] : zero;
        const f32x4 xv = x[base + (long long)h * cols];
        f32x4 an = zero, ad = zero;
#pragma unroll
        for (int t = -TN_R; t <= TN_R; ++t) {
            const f32x4 g = tp.g[t < 0 ? -t : t];
            an = tn_fma4(g, wn[t + TN_R], an);
            ad = tn_fma4(g, wd[t + TN_R], ad);
        }
        f32x4 o;
        o.x = (on[0] && xv.x != TN_BG) ? an.x / ad.x : xv.x;
        o.y = (on[1] && xv.y != TN_BG) ? an.y / ad.y : xv.y;
        o.z = (on[2] && xv.z != TN_BG) ? an.z / ad.z : xv.z;
        o.w = (on[3] && xv.w != TN_BG) ? an.w / ad.w : xv.w;
        y[base + (long long)h * cols] = o;
    }
}

// ---------------------------------------------------------------------------------------------- blur, any M
// One pass along one axis, one thread per float.  stage 0: x -> (N, D) along d; stage 1: (N, D) -> (N, D) along w; stage 2: (N, D) along h and
// the quotient -> y (an unflagged contrast or row: y = x).  grid (x, B), grid-stride over the N M floats of a sample.
__global__ __launch_bounds__(256) void tone_blur_axis_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ nin,
                                                             const float* __restrict__ din, float* __restrict__ nout, float* __restrict__ dout,
                                                             const unsigned long long* __restrict__ table, int ld, int col, int M, int PH, int PW, int PD, int stage) {
    const int b = blockIdx.y;
    const unsigned* blk = tn_block(table, ld, col, b);
    const bool row_on = tn_row_has(blk, M, TN_BLUR);
    if (!row_on && stage < 2) return;
    const long long per = (long long)PH * PW * PD * M, off = (long long)b * per;
    const int n = stage == 0 ? PD : (stage == 1 ? PW : PH);                     // the extent and the element stride of the pass's axis
    const long long st = stage == 0 ? M : (stage == 1 ? (long long)PD * M : (long long)PW * PD * M);
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < per; e += gridDim.x * 256LL) {
        const int p = (int)(e / M), m = (int)(e - (long long)p * M);
        const bool on = row_on && (tn_flags(blk, m) & TN_BLUR);
        if (!on) {
            if (stage == 2) y[off + e] = x[off + e];
            continue;
        }
        const int k = p % PD, j = (p / PD) % PW, i = p / PD / PW;
        const int a = stage == 0 ? k : (stage == 1 ? j : i);
        float an = 0.f, ad = 0.f;
#pragma unroll
        for (int t = -TN_R; t <= TN_R; ++t) {
            if (a + t < 0 || a + t >= n) continue;
            const float g = tn_word(blk, m, 1 + (t < 0 ? -t : t));
            const long long s = off + e + t * st;
            float vn, vd;
            if (stage == 0) { const float v = x[s]; vd = v != TN_BG ? 1.f : 0.f; vn = v != TN_BG ? v : 0.f; }
            else { vn = nin[s]; vd = din[s]; }
            an = __builtin_fmaf(g, vn, an);
            ad = __builtin_fmaf(g, vd, ad);
        }
        if (stage < 2) { nout[off + e] = an; dout[off + e] = ad; }
        else { const float v = x[off + e]; y[off + e] = v != TN_BG ? an / ad : v; }
    }
}

// ---------------------------------------------------------------------------------------------- statistics
struct TnAcc { float lo, hi; double sum; int n; };
__device__ __forceinline__ void tn_acc_add(TnAcc& a, float v) {
    if (v != TN_BG) { a.lo = fminf(a.lo, v); a.hi = fmaxf(a.hi, v); a.sum += (double)v; a.n += 1; }
}
__device__ __forceinline__ void tn_acc_merge(TnAcc& a, float lo, float hi, double sum, int n) {
    a.lo = fminf(a.lo, lo); a.hi = fmaxf(a.hi, hi); a.sum += sum; a.n += n;
}
__device__ __forceinline__ TnAcc tn_wave_acc(TnAcc a) {         // a fixed tree over the 64 lanes; lane 0 holds the result
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        tn_acc_merge(a, __shfl_down(a.lo, o, 64), __shfl_down(a.hi, o, 64), __shfl_down(a.sum, o, 64), __shfl_down(a.n, o, 64));
    return a;
}

// V = 4: M == 4, grid (nblk, B), a voxel's contrasts as one f32x4; V = 1: grid (M nblk, B), blockIdx.x = m nblk + block.  256 threads.
// partials, indexed [(b M + m) nblk + block]: psum (double), then plo, phi (float), pn (int)
template <int V>
__global__ __launch_bounds__(256) void tone_stats_part_kernel(const float* __restrict__ x, double* __restrict__ psum, float* __restrict__ plo,
                                                              float* __restrict__ phi, int* __restrict__ pn, int M, int N, int nblk) {
    __shared__ float slo[4][V], shi[4][V];
    __shared__ double ssum[4][V];
    __shared__ int sn[4][V];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    TnAcc a[V];
#pragma unroll
    for (int v = 0; v < V; ++v) a[v] = TnAcc{__builtin_inff(), -__builtin_inff(), 0.0, 0};
    const int b = blockIdx.y, m = V == 4 ? 0 : blockIdx.x / nblk, bk = blockIdx.x - m * nblk;
    if (V == 4) {
        const f32x4* src = reinterpret_cast<const f32x4*>(x) + (long long)b * N;
        for (int p = bk * 256 + tid; p < N; p += nblk * 256) {
            const f32x4 v = src[p];
            tn_acc_add(a[0], v.x); tn_acc_add(a[V > 1 ? 1 : 0], v.y); tn_acc_add(a[V > 2 ? 2 : 0], v.z); tn_acc_add(a[V > 3 ? 3 : 0], v.w);
        }
    } else {
        const float* src = x + (long long)b * N * M + m;
        for (int p = bk * 256 + tid; p < N; p += nblk * 256) tn_acc_add(a[0], src[(long long)p * M]);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        a[v] = tn_wave_acc(a[v]);
        if (lane == 0) { slo[wave][v] = a[v].lo; shi[wave][v] = a[v].hi; ssum[wave][v] = a[v].sum; sn[wave][v] = a[v].n; }
    }
    __syncthreads();
    if (tid < V) {
        TnAcc r = TnAcc{slo[0][tid], shi[0][tid], ssum[0][tid], sn[0][tid]};
        for (int w = 1; w < 4; ++w) tn_acc_merge(r, slo[w][tid], shi[w][tid], ssum[w][tid], sn[w][tid]);
        const long long o = ((long long)b * M + m + tid) * nblk + bk;
        psum[o] = r.sum; plo[o] = r.lo; phi[o] = r.hi; pn[o] = r.n;
    }
}

// grid (B M), 64 threads: lane l takes the partials l, l + 64, .. in order, then the lane tree
__global__ __launch_bounds__(64) void tone_stats_finish_kernel(const double* __restrict__ psum, const float* __restrict__ plo, const float* __restrict__ phi,
                                                               const int* __restrict__ pn, unsigned* __restrict__ stats, int nblk) {
    const long long o = (long long)blockIdx.x * nblk;
    TnAcc a = TnAcc{__builtin_inff(), -__builtin_inff(), 0.0, 0};
    for (int k = threadIdx.x; k < nblk; k += 64) tn_acc_merge(a, plo[o + k], phi[o + k], psum[o + k], pn[o + k]);
    a = tn_wave_acc(a);
    if (threadIdx.x == 0) {
        unsigned* s = stats + 4LL * blockIdx.x;
        const bool any = a.n > 0;
        s[0] = __float_as_uint(any ? a.lo : 0.f);
        s[1] = __float_as_uint(any ? a.hi : 0.f);
        s[2] = __float_as_uint(any ? (float)(a.sum / (double)a.n) : 0.f);
        s[3] = (unsigned)a.n;
    }
}

// ---------------------------------------------------------------------------------------------- tone
// Philox4x32-10 on the counter (p, m, 0, 0) under the key (k0, k1) -> the sum of the 16 bytes of the four output words
__device__ __forceinline__ unsigned tn_philox_bytes(unsigned p, unsigned m, unsigned k0, unsigned k1) {
    unsigned c0 = p, c1 = m, c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    unsigned s = 0;
    const unsigned w[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int i = 0; i < 4; ++i) s += (w[i] & 255u) + ((w[i] >> 8) & 255u) + ((w[i] >> 16) & 255u) + (w[i] >> 24);
    return s;
}

struct TnTone { unsigned flags; float f, gamma, std, lo, hi, mean; };
__device__ __forceinline__ TnTone tn_tone_params(const unsigned* blk, const unsigned* stats, int b, int M, int m) {
    TnTone t;
    t.flags = tn_flags(blk, m); t.f = tn_word(blk, m, 6); t.gamma = tn_word(blk, m, 7); t.std = tn_word(blk, m, 8);
    const unsigned* s = stats + 4LL * ((long long)b * M + m);
    t.lo = __uint_as_float(s[0]); t.hi = __uint_as_float(s[1]); t.mean = __uint_as_float(s[2]);
    return t;
}
__device__ __forceinline__ float tn_tone(float v, const TnTone& t, unsigned p, unsigned m, unsigned k0, unsigned k1) {
#pragma clang fp contract(off)              // every statement rounds once; the fused steps are the explicit fmaf calls
    if (v == TN_BG || !(t.flags & TN_TONE_BITS)) return v;
    if (t.flags & TN_CONTRAST) {
        const float d = v - t.mean;
        v = fminf(fmaxf(__builtin_fmaf(d, t.f, t.mean), t.lo), t.hi);
    }
    if ((t.flags & TN_GAMMA) && t.hi > t.lo) {
        const float rg = t.hi - t.lo;
        const float d = v - t.lo;
        float u = fminf(fmaxf(d / rg, 0.f), 1.f);
        if (t.flags & TN_INVERT) u = 1.f - u;
        u = powf(u, t.gamma);
        if (t.flags & TN_INVERT) u = 1.f - u;
        v = __builtin_fmaf(u, rg, t.lo);
    }
    if (t.flags & TN_NOISE) {
        const int s2 = 2 * (int)tn_philox_bytes(p, m, k0, k1) - 4080;
        const float z = (float)s2 * __uint_as_float(TN_Z_SCALE);
        v = __builtin_fmaf(t.std, z, v);
    }
    return v;
}

// V = 4: M == 4, a voxel per thread; V = 1: a float per thread.  grid (x, B), grid-stride.
template <int V>
__global__ __launch_bounds__(256) void tone_apply_kernel(float* __restrict__ x, const unsigned* __restrict__ stats, const unsigned long long* __restrict__ table,
                                                         int ld, int col, int M, int N) {
    const int b = blockIdx.y;
    const unsigned* blk = tn_block(table, ld, col, b);
    if (!tn_row_has(blk, M, TN_TONE_BITS)) return;              // uniform: the row stays as it is, bit for bit
    const unsigned k0 = blk[0], k1 = blk[1];
    if (V == 4) {
        TnTone t[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) t[m] = tn_tone_params(blk, stats, b, 4, m);
        f32x4* row = reinterpret_cast<f32x4*>(x) + (long long)b * N;
        for (int p = blockIdx.x * 256 + threadIdx.x; p < N; p += gridDim.x * 256) {
            f32x4 v = row[p];
            v.x = tn_tone(v.x, t[0], (unsigned)p, 0u, k0, k1); v.y = tn_tone(v.y, t[1], (unsigned)p, 1u, k0, k1);
            v.z = tn_tone(v.z, t[2], (unsigned)p, 2u, k0, k1); v.w = tn_tone(v.w, t[3], (unsigned)p, 3u, k0, k1);
            row[p] = v;
        }
    } else {
        const long long per = (long long)N * M;
        float* row = x + (long long)b * per;
        for (long long e = blockIdx.x * 256LL + threadIdx.x; e < per; e += gridDim.x * 256LL) {
            const int p = (int)(e / M), m = (int)(e - (long long)p * M);
            const TnTone t = tn_tone_params(blk, stats, b, M, m);
            if (!(t.flags & TN_TONE_BITS)) continue;
            row[e] = tn_tone(row[e], t, (unsigned)p, (unsigned)m, k0, k1);
        }
    }
}

// ---------------------------------------------------------------------------------------------- host
// the checks every entry point shares; N = PH PW PD on success
int tn_check(const void* x, int B, int M, int PH, int PW, int PD, long long* N) {
    if (!x || B < 1 || M < 1 || M > 64 || PH < 1 || PW < 1 || PD < 1) return MRDIS_EINVAL;
    *N = (long long)PH * PW * PD;
    if (B > 65535 || *N >= (1LL << 31)) return MRDIS_EUNSUPPORTED;
    if (((uintptr_t)x) & 3) return MRDIS_EALIGN;
    return MRDIS_OK;
}
int tn_check_table(const void* table, int ld_table, int col, int M) {
    if (!table || col < 0 || (long long)ld_table < (long long)col + 1 + 5LL * M) return MRDIS_EINVAL;
    if (((uintptr_t)table) & 7) return MRDIS_EALIGN;
    return MRDIS_OK;
}
// the M == 4 kernels: four contrasts, 16-byte aligned bases, and not under debug_volgen
bool tn_vec4(int M, const void* a, const void* b) {
    return M == 4 && !mrdis_opt(MRDIS_OPT_VOLGEN) && ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
}
unsigned tn_grid(long long work) { long long g = (work + 255) / 256; return (unsigned)(g > 4096 ? 4096 : g); }
int tn_stat_blocks(long long N) { const long long g = (N + 255) / 256; return (int)(g > TN_STAT_BLOCKS ? TN_STAT_BLOCKS : g); }
}  // namespace

// two (N, D) pairs of the generic form; the M == 4 form uses the first
extern "C" size_t mrdis_patch_blur_workspace(int B, int M, int PH, int PW, int PD) {
    if (B < 1 || M < 1 || PH < 1 || PW < 1 || PD < 1) return 0;
    return (size_t)4 * sizeof(float) * (size_t)B * (size_t)M * (size_t)PH * (size_t)PW * (size_t)PD;
}

extern "C" int mrdis_patch_blur(const float* x, float* y, const void* table, int ld_table, int col, int B, int M, int PH, int PW, int PD,
                                void* workspace, size_t workspace_bytes, void* stream) {
    long long N;
    int rc = tn_check(x, B, M, PH, PW, PD, &N);
    if (rc != MRDIS_OK) return rc;
    if (!y || x == y || !workspace) return MRDIS_EINVAL;
    if ((rc = tn_check_table(table, ld_table, col, M)) != MRDIS_OK) return rc;
    if ((((uintptr_t)y) & 3) || (((uintptr_t)workspace) & 15)) return MRDIS_EALIGN;
    if (workspace_bytes < mrdis_patch_blur_workspace(B, M, PH, PW, PD)) return MRDIS_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long* t = reinterpret_cast<const unsigned long long*>(table);
    const long long total = (long long)B * N * M;               // floats of x
    mrdis_count(MRDIS_CNT_PATCHBLUR);
    if (tn_vec4(M, x, y)) {
        const int nbw = mrdis_cdiv(PW, TN_BW), nbd = mrdis_cdiv(PD, TN_BD);
        const long long tiles = (long long)nbw * nbd * PH;
        const int cols = PW * PD, ncb = mrdis_cdiv(cols, 256);
        const long long hblocks = (long long)ncb * mrdis_cdiv(PH, TN_HSEG);
        // (both grids are at most N < 2^31 workgroups wide)
        f32x4* ws = reinterpret_cast<f32x4*>(workspace);
        MRDIS_LAUNCH(tone_blur_dw4_kernel, dim3((unsigned)tiles, B), dim3(256), 0, s, reinterpret_cast<const f32x4*>(x), ws, t, ld_table, col, PH, PW, PD, nbw, nbd,
                     (long long)B * N);
        MRDIS_CHECK_LAUNCH();
        MRDIS_LAUNCH(tone_blur_h4_kernel, dim3((unsigned)hblocks, B), dim3(256), 0, s, reinterpret_cast<const f32x4*>(x), reinterpret_cast<f32x4*>(y), ws, t, ld_table,
                     col, PH, cols, ncb, (long long)B * N);
        MRDIS_CHECK_LAUNCH();
        return MRDIS_OK;
    }
    float* w = reinterpret_cast<float*>(workspace);
    float *na = w, *da = w + total, *nb = w + 2 * total, *db = w + 3 * total;
    const dim3 grid(tn_grid(N * M), B);
    MRDIS_LAUNCH(tone_blur_axis_kernel, grid, dim3(256), 0, s, x, y, (const float*)nullptr, (const float*)nullptr, na, da, t, ld_table, col, M, PH, PW, PD, 0);
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(tone_blur_axis_kernel, grid, dim3(256), 0, s, x, y, (const float*)na, (const float*)da, nb, db, t, ld_table, col, M, PH, PW, PD, 1);
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(tone_blur_axis_kernel, grid, dim3(256), 0, s, x, y, (const float*)nb, (const float*)db, (float*)nullptr, (float*)nullptr, t, ld_table, col, M, PH, PW, PD, 2);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" size_t mrdis_patch_stats_workspace(int B, int M, int PH, int PW, int PD) {
    if (B < 1 || M < 1 || PH < 1 || PW < 1 || PD < 1) return 0;
    return (size_t)20 * (size_t)B * (size_t)M * (size_t)tn_stat_blocks((long long)PH * PW * PD);
}

extern "C" int mrdis_patch_stats(const float* x, void* stats, int B, int M, int PH, int PW, int PD, void* workspace, size_t workspace_bytes, void* stream) {
    long long N;
    const int rc = tn_check(x, B, M, PH, PW, PD, &N);
    if (rc != MRDIS_OK) return rc;
    if (!stats || !workspace) return MRDIS_EINVAL;
    if ((((uintptr_t)stats) & 3) || (((uintptr_t)workspace) & 15)) return MRDIS_EALIGN;
    if (workspace_bytes < mrdis_patch_stats_workspace(B, M, PH, PW, PD)) return MRDIS_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = tn_stat_blocks(N);
    const long long parts = (long long)B * M * nblk;
    double* psum = reinterpret_cast<double*>(workspace);
    float* plo = reinterpret_cast<float*>(psum + parts);
    float* phi = plo + parts;
    int* pn = reinterpret_cast<int*>(phi + parts);
    mrdis_count(MRDIS_CNT_PATCHSTATS);
    if (tn_vec4(M, x, x)) {
        MRDIS_LAUNCH(tone_stats_part_kernel<4>, dim3(nblk, B), dim3(256), 0, s, x, psum, plo, phi, pn, M, (int)N, nblk);
    } else {
        MRDIS_LAUNCH(tone_stats_part_kernel<1>, dim3(nblk * M, B), dim3(256), 0, s, x, psum, plo, phi, pn, M, (int)N, nblk);
    }
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(tone_stats_finish_kernel, dim3(B * M), dim3(64), 0, s, (const double*)psum, (const float*)plo, (const float*)phi, (const int*)pn,
                 reinterpret_cast<unsigned*>(stats), nblk);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_patch_tone(float* x, const void* stats, const void* table, int ld_table, int col, int B, int M, int PH, int PW, int PD, void* stream) {
    long long N;
    int rc = tn_check(x, B, M, PH, PW, PD, &N);
    if (rc != MRDIS_OK) return rc;
    if (!stats) return MRDIS_EINVAL;
    if ((rc = tn_check_table(table, ld_table, col, M)) != MRDIS_OK) return rc;
    if (((uintptr_t)stats) & 3) return MRDIS_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long* t = reinterpret_cast<const unsigned long long*>(table);
    const unsigned* st = reinterpret_cast<const unsigned*>(stats);
    mrdis_count(MRDIS_CNT_PATCHTONE);
    if (tn_vec4(M, x, x)) MRDIS_LAUNCH(tone_apply_kernel<4>, dim3(tn_grid(N), B), dim3(256), 0, s, x, st, t, ld_table, col, M, (int)N);
    else MRDIS_LAUNCH(tone_apply_kernel<1>, dim3(tn_grid(N * M), B), dim3(256), 0, s, x, st, t, ld_table, col, M, (int)N);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
