// Kernels of the `others` variants of the reference (config.yaml:67-70):
//
//  * mod_enc_s: the modality encoder's first CondConv layer reads cat([x_i, s_i], 1) (model.py:2374).  The conv2d_2src kernels take
//    the two sources as they are -- x (N,H,W,Cx) and s (N,H,W,Cs), each an NHWC view with its own pixel stride -- so the
//    concatenation is never written.  The filter is the mixed one of the layer, w_tck [T][Cx+Cs][Co] / w_tkc [T][Co][Cx+Cs]
//    (input channel ci < Cx reads x, ci >= Cx reads s), exactly the filter of the concatenated layer.
//      forward:          y = lrelu?(bias + sum_{tap, ci} in[ci] * w)              one thread per output pixel, filter in LDS
//      data gradient:    dx / ds = sum_{tap, co} dy * w_tkc                        one thread per input pixel (dx may be NULL)
//      weight gradient:  dw = sum_{pixels} in * dy, dbias = sum dy                 64-pixel row tiles staged in LDS, one job per
//                        (tap, ci) and one for the bias, each held by several threads that split the tile's pixels; per-workgroup
//                        slabs summed in a fixed order (mrdis_launch_slab_reduce)
//    fp32 FMA throughout.  Geometry: T = kh * kw <= 9, Cx + Cs <= 32, Co <= 16, stride <= 2 (the reference's layer: 3x3, stride 2,
//    pad 1, 7 + 4 -> 16).
//  * ana_dec_act (model.py:3145-3153): softplus (torch's beta = 1, threshold = 20) and the channel softmax without the mask
//    channel, forward and backward.
//
// Launch counter families "conv2src" (the three conv entry points, reduce included) and "ana_act" (the activations).
#include "mrdis_common.h"

namespace {

constexpr int C2_CO = 16;          // output channels held per thread (Co <= 16, zero-padded)
constexpr int C2_TW = 64;          // output pixels of a weight-gradient row tile
constexpr int C2_MAX_T = 9, C2_MAX_CI = 32;
constexpr int C2_WG_MAX = 512;     // weight-gradient workgroup: up to 512 / JP copies of the (tap, ci) + bias jobs
constexpr int C2_WG_BLOCKS = 1024; // weight-gradient workgroups (= slabs) at most

inline int ew_grid(long long n, int threads) { long long b = (n + threads - 1) / threads; if (b > 8192) b = 8192; if (b < 1) b = 1; return (int)b; }

struct C2Geom {
    const float* x; const float* s; int ldx, lds, Cx, Cs;
    int N, H, W, Ho, Wo, Co, kh, kw, stride, pad;
};

// ---------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void conv2src_fwd_kernel(C2Geom g, const float* __restrict__ w_tck, const float* __restrict__ bias,
                                                          float* __restrict__ y, int ldy, int lrelu) {
    __shared__ float wl[C2_MAX_T * C2_MAX_CI * C2_CO];
    __shared__ float bl[C2_CO];
    const int Ci = g.Cx + g.Cs, T = g.kh * g.kw;
    for (int i = threadIdx.x; i < T * Ci * C2_CO; i += blockDim.x) {
        const int co = i % C2_CO, tc = i / C2_CO;
        wl[i] = co < g.Co ? w_tck[(long long)tc * g.Co + co] : 0.f;
    }
    if (threadIdx.x < C2_CO) bl[threadIdx.x] = (bias != nullptr && (int)threadIdx.x < g.Co) ? bias[threadIdx.x] : 0.f;
    __syncthreads();
    const long long P = (long long)g.N * g.Ho * g.Wo;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        const int ow = (int)(p % g.Wo);
        const long long nh = p / g.Wo;
        const int oh = (int)(nh % g.Ho), n = (int)(nh / g.Ho);
        float acc[C2_CO];
#pragma unroll
        for (int co = 0; co < C2_CO; ++co) acc[co] = 0.f;
        for (int r = 0; r < g.kh; ++r) {
            const int ih = oh * g.stride - g.pad + r;
            if (ih < 0 || ih >= g.H) continue;
            for (int c = 0; c < g.kw; ++c) {
                const int iw = ow * g.stride - g.pad + c;
                if (iw < 0 || iw >= g.W) continue;
                const long long q = ((long long)n * g.H + ih) * g.W + iw;
                const float* wt = wl + (r * g.kw + c) * Ci * C2_CO;
                const float* xp = g.x + q * g.ldx;
                for (int ci = 0; ci < g.Cx; ++ci) {
                    const float v = xp[ci];
#pragma unroll
                    for (int co = 0; co < C2_CO; ++co) acc[co] = fmaf(v, wt[ci * C2_CO + co], acc[co]);
                }
                const float* sp = g.s + q * g.lds;
                wt += g.Cx * C2_CO;
                for (int ci = 0; ci < g.Cs; ++ci) {
                    const float v = sp[ci];
#pragma unroll
                    for (int co = 0; co < C2_CO; ++co) acc[co] = fmaf(v, wt[ci * C2_CO + co], acc[co]);
                }
            }
        }
        float* yp = y + p * ldy;
#pragma unroll
        for (int co = 0; co < C2_CO; ++co) {
            if (co < g.Co) {
                float v = acc[co] + bl[co];
                if (lrelu) v = v > 0.f ? v : 0.2f * v;
                yp[co] = v;
            }
        }
    }
}

// ---------------------------------------------------------------- data gradient
template <int CIP>
__global__ __launch_bounds__(256) void conv2src_dgrad_kernel(C2Geom g, const float* __restrict__ dy, int lddy, const float* __restrict__ w_tkc,
                                                            float* __restrict__ dx, int lddx, float* __restrict__ ds, int ldds) {
    __shared__ float wl[C2_MAX_T * C2_CO * CIP];
    const int Ci = g.Cx + g.Cs, T = g.kh * g.kw;
    for (int i = threadIdx.x; i < T * C2_CO * CIP; i += blockDim.x) {
        const int ci = i % CIP, tco = i / CIP, co = tco % C2_CO, t = tco / C2_CO;
        wl[i] = (ci < Ci && co < g.Co) ? w_tkc[((long long)t * g.Co + co) * Ci + ci] : 0.f;
    }
    __syncthreads();
    const long long P = (long long)g.N * g.H * g.W;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < P; q += (long long)gridDim.x * blockDim.x) {
        const int iw = (int)(q % g.W);
        const long long nh = q / g.W;
        const int ih = (int)(nh % g.H), n = (int)(nh / g.H);
        float acc[CIP];
#pragma unroll
        for (int ci = 0; ci < CIP; ++ci) acc[ci] = 0.f;
        for (int r = 0; r < g.kh; ++r) {
            const int th = ih + g.pad - r;                 // = oh * stride
            if (th < 0 || th % g.stride) continue;
            const int oh = th / g.stride;
            if (oh >= g.Ho) continue;
            for (int c = 0; c < g.kw; ++c) {
                const int tw = iw + g.pad - c;
                if (tw < 0 || tw % g.stride) continue;
                const int ow = tw / g.stride;
                if (ow >= g.Wo) continue;
                const float* dp = dy + (((long long)n * g.Ho + oh) * g.Wo + ow) * lddy;
                const float* wt = wl + (r * g.kw + c) * C2_CO * CIP;
                for (int co = 0; co < g.Co; ++co) {
                    const float d = dp[co];
#pragma unroll
                    for (int ci = 0; ci < CIP; ++ci) acc[ci] = fmaf(d, wt[co * CIP + ci], acc[ci]);
                }
            }
        }
#pragma unroll
        for (int ci = 0; ci < CIP; ++ci) {
            if (ci < g.Cx) { if (dx != nullptr) dx[q * lddx + ci] = acc[ci]; }
            else if (ci < Ci) ds[q * ldds + (ci - g.Cx)] = acc[ci];
        }
    }
}

// ---------------------------------------------------------------- weight gradient
// Tile = C2_TW consecutive output pixels of one output row.  LDS: the kh input rows x ((C2_TW - 1) * stride + kw) columns x Ci
// channels the tile reads (zero outside the image), then the tile's dy (C2_TW x 16, zero beyond Co / the row's end).  Job j < T * Ci
// is (tap, ci) = (j / Ci, j % Ci) with Co accumulators, job T * Ci the bias.  The jobs are padded to JP (a multiple of 64) and the
// workgroup holds GROUPS = blockDim / JP copies of them: copy g takes pixels g, g + GROUPS, ... of every tile (a wave is one copy, so it
// reads the same dy row: an LDS broadcast).  At the end copies 1.. hand their sums to copy 0 through LDS, added in copy order.
// Workgroup b takes tiles b, b + G, ...; its sums go to slab b.
__global__ __launch_bounds__(C2_WG_MAX) void conv2src_wgrad_kernel(C2Geom g, const float* __restrict__ dy, int lddy, float* __restrict__ slab,
                                                                  float* __restrict__ bslab, int tiles_per_row, int JP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* patch = reinterpret_cast<float*>(smem_raw);
    const int Ci = g.Cx + g.Cs, T = g.kh * g.kw;
    const int PW = (C2_TW - 1) * g.stride + g.kw;
    const int patch_n = g.kh * PW * Ci;
    float* dyl = patch + patch_n;
    const long long tiles = (long long)g.N * g.Ho * tiles_per_row;
    const int GROUPS = blockDim.x / JP;
    const int j = threadIdx.x % JP, grp = threadIdx.x / JP;
    const int jt = j / Ci, jc = j % Ci;
    const int jr = jt / g.kw, jw = jt % g.kw;
    float acc[C2_CO];
#pragma unroll
    for (int co = 0; co < C2_CO; ++co) acc[co] = 0.f;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int seg = (int)(tile % tiles_per_row);
        const long long nh = tile / tiles_per_row;
        const int oh = (int)(nh % g.Ho), n = (int)(nh / g.Ho);
        const int ow0 = seg * C2_TW;
        const int ih0 = oh * g.stride - g.pad, iw0 = ow0 * g.stride - g.pad;
        __syncthreads();                                   // the previous tile's readers are done
        for (int i = threadIdx.x; i < patch_n; i += blockDim.x) {
            const int ci = i % Ci, rc = i / Ci, c = rc % PW, r = rc / PW;
            const int ih = ih0 + r, iw = iw0 + c;
            float v = 0.f;
            if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) {
                const long long q = ((long long)n * g.H + ih) * g.W + iw;
                v = ci < g.Cx ? g.x[q * g.ldx + ci] : g.s[q * g.lds + (ci - g.Cx)];
            }
            patch[i] = v;
        }
        for (int i = threadIdx.x; i < C2_TW * C2_CO; i += blockDim.x) {
            const int co = i % C2_CO, t = i / C2_CO, ow = ow0 + t;
            dyl[i] = (co < g.Co && ow < g.Wo) ? dy[(((long long)n * g.Ho + oh) * g.Wo + ow) * lddy + co] : 0.f;
        }
        __syncthreads();
        if (j < T * Ci) {
            const float* pp = patch + (jr * PW + jw) * Ci + jc;
            for (int t = grp; t < C2_TW; t += GROUPS) {
                const float v = pp[t * g.stride * Ci];
#pragma unroll
                for (int co = 0; co < C2_CO; ++co) acc[co] = fmaf(v, dyl[t * C2_CO + co], acc[co]);
            }
        } else if (j == T * Ci) {
            for (int t = grp; t < C2_TW; t += GROUPS) {
#pragma unroll
                for (int co = 0; co < C2_CO; ++co) acc[co] += dyl[t * C2_CO + co];
            }
        }
    }
    if (GROUPS > 1) {                                      // copies 1.. -> LDS (over the last tile's staging), copy 0 adds them in order
        float* red = patch;
        __syncthreads();
        if (grp > 0 && j <= T * Ci) {
#pragma unroll
            for (int co = 0; co < C2_CO; ++co) red[((grp - 1) * JP + j) * C2_CO + co] = acc[co];
        }
        __syncthreads();
        if (grp == 0 && j <= T * Ci) {
            for (int q = 1; q < GROUPS; ++q) {
#pragma unroll
                for (int co = 0; co < C2_CO; ++co) acc[co] += red[((q - 1) * JP + j) * C2_CO + co];
            }
        }
    }
    if (grp != 0) return;
    const int total = T * Ci * g.Co;
    if (j < T * Ci) {
        float* sp = slab + (long long)blockIdx.x * total + (long long)j * g.Co;       // [tap][ci][co] = w_tck order
#pragma unroll
        for (int co = 0; co < C2_CO; ++co) if (co < g.Co) sp[co] = acc[co];
    } else if (j == T * Ci) {
        float* bp = bslab + (long long)blockIdx.x * g.Co;
#pragma unroll
        for (int co = 0; co < C2_CO; ++co) if (co < g.Co) bp[co] = acc[co];
    }
}

int c2_check(const C2Geom& g) {
    if (!g.x || !g.s || g.N < 1 || g.H < 1 || g.W < 1 || g.Cx < 1 || g.Cs < 1 || g.Co < 1 || g.kh < 1 || g.kw < 1 || g.stride < 1 || g.pad < 0)
        return MRDIS_EINVAL;
    if (g.ldx < g.Cx || g.lds < g.Cs) return MRDIS_EINVAL;
    if (g.kh * g.kw > C2_MAX_T || g.Cx + g.Cs > C2_MAX_CI || g.Co > C2_CO || g.stride > 2) return MRDIS_EUNSUPPORTED;
    if (g.Ho < 1 || g.Wo < 1) return MRDIS_EINVAL;
    return MRDIS_OK;
}

C2Geom c2_geom(const float* x, int ldx, int Cx, const float* s, int lds_, int Cs, int N, int H, int W, int Co, int kh, int kw, int stride, int pad) {
    C2Geom g{};
    g.x = x; g.s = s; g.ldx = ldx; g.lds = lds_; g.Cx = Cx; g.Cs = Cs; g.N = N; g.H = H; g.W = W; g.Co = Co;
    g.kh = kh; g.kw = kw; g.stride = stride < 1 ? 1 : stride; g.pad = pad;
    g.Ho = (H + 2 * pad - kh) / g.stride + 1; g.Wo = (W + 2 * pad - kw) / g.stride + 1;
    if (H + 2 * pad < kh || W + 2 * pad < kw) g.Ho = g.Wo = 0;
    return g;
}

int c2_wgrad_blocks(const C2Geom& g) {
    const long long tiles = (long long)g.N * g.Ho * mrdis_cdiv(g.Wo, C2_TW);
    return (int)(tiles < C2_WG_BLOCKS ? tiles : C2_WG_BLOCKS);
}

// ---------------------------------------------------------------- anatomy activations
__global__ void softplus_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, long long P, int C) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < P * C; i += (long long)gridDim.x * blockDim.x) {
        const long long p = i / C; const int c = (int)(i % C);
        const float v = x[p * ldx + c];
        y[p * ldy + c] = v > 20.f ? v : log1pf(expf(v));           // F.softplus(beta=1, threshold=20)
    }
}
__global__ void softplus_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx, float* __restrict__ dx, int lddx,
                                    long long P, int C) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < P * C; i += (long long)gridDim.x * blockDim.x) {
        const long long p = i / C; const int c = (int)(i % C);
        const float v = x[p * ldx + c], d = dy[p * lddy + c];
        const float z = expf(v);
        dx[p * lddx + c] = v > 20.f ? d : d * z / (z + 1.f);        // torch's softplus_backward
    }
}
constexpr int SMX_MAXC = 8;
__global__ void softmax_fwd_kernel(const float* __restrict__ s, int lds_, float* __restrict__ out, int ldo, long long P, int C) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        float l[SMX_MAXC];
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < SMX_MAXC; ++c) if (c < C) { l[c] = s[p * lds_ + c]; mx = fmaxf(mx, l[c]); }
        float den = 0.f;
#pragma unroll
        for (int c = 0; c < SMX_MAXC; ++c) if (c < C) { l[c] = expf(l[c] - mx); den += l[c]; }
        const float inv = 1.f / den;
#pragma unroll
        for (int c = 0; c < SMX_MAXC; ++c) if (c < C) out[p * ldo + c] = l[c] * inv;
    }
}
__global__ void softmax_bwd_kernel(const float* __restrict__ dout, int lddo, const float* __restrict__ out, int ldo, float* __restrict__ ds, int ldds,
                                   long long P, int C) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        float o[SMX_MAXC], d[SMX_MAXC];
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < SMX_MAXC; ++c) if (c < C) { o[c] = out[p * ldo + c]; d[c] = dout[p * lddo + c]; dot += o[c] * d[c]; }
#pragma unroll
        for (int c = 0; c < SMX_MAXC; ++c) if (c < C) ds[p * ldds + c] = o[c] * (d[c] - dot);
    }
}

}  // namespace

extern "C" int mrdis_conv2d_2src_fwd(const float* x, int ldx, int Cx, const float* s, int lds_, int Cs, const float* w_tck, const float* bias,
                                     float* y, int ldy, int N, int H, int W, int Co, int kh, int kw, int stride, int pad, int lrelu, void* stream) {
    const C2Geom g = c2_geom(x, ldx, Cx, s, lds_, Cs, N, H, W, Co, kh, kw, stride, pad);
    const int rc = c2_check(g);
    if (rc != MRDIS_OK) return rc;
    if (!w_tck || !y || ldy < Co) return MRDIS_EINVAL;
    mrdis_count(MRDIS_CNT_CONV2SRC);
    MRDIS_LAUNCH(conv2src_fwd_kernel, dim3(ew_grid((long long)N * g.Ho * g.Wo, 256)), dim3(256), 0, (hipStream_t)stream, g, w_tck, bias, y, ldy, lrelu);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_conv2d_2src_bwd_data(const float* dy, int lddy, const float* w_tkc, float* dx, int lddx, int Cx, float* ds, int ldds, int Cs,
                                          int N, int H, int W, int Co, int kh, int kw, int stride, int pad, void* stream) {
    // (x and s are not read: any non-null pointer satisfies the shared geometry check)
    C2Geom g = c2_geom(dy, Cx, Cx, dy, Cs, Cs, N, H, W, Co, kh, kw, stride, pad);
    const int rc = c2_check(g);
    if (rc != MRDIS_OK) return rc;
    if (!dy || !w_tkc || !ds || lddy < Co || ldds < Cs || (dx != nullptr && lddx < Cx)) return MRDIS_EINVAL;
    g.x = g.s = nullptr;
    mrdis_count(MRDIS_CNT_CONV2SRC);
    const dim3 grid(ew_grid((long long)N * H * W, 256));
    if (Cx + Cs <= 16) MRDIS_LAUNCH((conv2src_dgrad_kernel<16>), grid, dim3(256), 0, (hipStream_t)stream, g, dy, lddy, w_tkc, dx, lddx, ds, ldds);
    else MRDIS_LAUNCH((conv2src_dgrad_kernel<32>), grid, dim3(256), 0, (hipStream_t)stream, g, dy, lddy, w_tkc, dx, lddx, ds, ldds);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" size_t mrdis_conv2d_2src_bwd_weight_workspace(int N, int H, int W, int Cx, int Cs, int Co, int kh, int kw, int stride, int pad) {
    const float one = 0.f;
    const C2Geom g = c2_geom(&one, Cx, Cx, &one, Cs, Cs, N, H, W, Co, kh, kw, stride, pad);
    if (c2_check(g) != MRDIS_OK) return 0;
    const size_t G = (size_t)c2_wgrad_blocks(g);
    return sizeof(float) * G * ((size_t)kh * kw * (Cx + Cs) * Co + Co);
}

extern "C" int mrdis_conv2d_2src_bwd_weight(const float* x, int ldx, int Cx, const float* s, int lds_, int Cs, const float* dy, int lddy,
                                            float* dw_tck, float* dbias, int accumulate_bias, void* workspace, size_t workspace_bytes,
                                            int N, int H, int W, int Co, int kh, int kw, int stride, int pad, void* stream) {
    const C2Geom g = c2_geom(x, ldx, Cx, s, lds_, Cs, N, H, W, Co, kh, kw, stride, pad);
    const int rc = c2_check(g);
    if (rc != MRDIS_OK) return rc;
    if (!dy || !dw_tck || !workspace || lddy < Co) return MRDIS_EINVAL;
    if (((uintptr_t)workspace & 15) != 0) return MRDIS_EALIGN;
    const int G = c2_wgrad_blocks(g);
    const int Ci = Cx + Cs, total = kh * kw * Ci * Co;
    if (workspace_bytes < sizeof(float) * (size_t)G * ((size_t)total + Co)) return MRDIS_EWORKSPACE;
    float* slab = (float*)workspace;
    float* bslab = slab + (size_t)G * total;
    const int jobs = kh * kw * Ci + 1;
    const int JP = ((jobs + 63) / 64) * 64;                     // <= 320 (T <= 9, Ci <= 32)
    const int groups = C2_WG_MAX / JP;                          // >= 1
    const size_t stage = (size_t)kh * ((C2_TW - 1) * g.stride + kw) * Ci + (size_t)C2_TW * C2_CO;
    const size_t red = (size_t)(groups - 1) * JP * C2_CO;
    const size_t lds = sizeof(float) * (stage > red ? stage : red);
    mrdis_count(MRDIS_CNT_CONV2SRC);
    MRDIS_LAUNCH(conv2src_wgrad_kernel, dim3(G), dim3(groups * JP), lds, (hipStream_t)stream, g, dy, lddy, slab, bslab, mrdis_cdiv(g.Wo, C2_TW), JP);
    MRDIS_CHECK_LAUNCH();
    return mrdis_launch_slab_reduce(slab, dw_tck, total, Co, G, bslab, dbias, accumulate_bias, (hipStream_t)stream);
}

extern "C" int mrdis_softplus_fwd(const float* x, int ldx, float* y, int ldy, long long P, int C, void* stream) {
    if (!x || !y || P < 1 || C < 1 || ldx < C || ldy < C) return MRDIS_EINVAL;
    mrdis_count(MRDIS_CNT_ANA_ACT);
    MRDIS_LAUNCH(softplus_fwd_kernel, dim3(ew_grid(P * C, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, P, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
extern "C" int mrdis_softplus_bwd(const float* dy, int lddy, const float* x, int ldx, float* dx, int lddx, long long P, int C, void* stream) {
    if (!dy || !x || !dx || P < 1 || C < 1 || lddy < C || ldx < C || lddx < C) return MRDIS_EINVAL;
    mrdis_count(MRDIS_CNT_ANA_ACT);
    MRDIS_LAUNCH(softplus_bwd_kernel, dim3(ew_grid(P * C, 256)), dim3(256), 0, (hipStream_t)stream, dy, lddy, x, ldx, dx, lddx, P, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
extern "C" int mrdis_softmax_fwd(const float* s, int lds_, float* out, int ldo, long long P, int C, void* stream) {
    if (!s || !out || P < 1 || C < 1 || lds_ < C || ldo < C) return MRDIS_EINVAL;
    if (C > SMX_MAXC) return MRDIS_EUNSUPPORTED;
    mrdis_count(MRDIS_CNT_ANA_ACT);
    MRDIS_LAUNCH(softmax_fwd_kernel, dim3(ew_grid(P, 256)), dim3(256), 0, (hipStream_t)stream, s, lds_, out, ldo, P, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
extern "C" int mrdis_softmax_bwd(const float* dout, int lddo, const float* out, int ldo, float* ds, int ldds, long long P, int C, void* stream) {
    if (!dout || !out || !ds || P < 1 || C < 1 || lddo < C || ldo < C || ldds < C) return MRDIS_EINVAL;
    if (C > SMX_MAXC) return MRDIS_EUNSUPPORTED;
    mrdis_count(MRDIS_CNT_ANA_ACT);
    MRDIS_LAUNCH(softmax_bwd_kernel, dim3(ew_grid(P, 256)), dim3(256), 0, (hipStream_t)stream, dout, lddo, out, ldo, ds, ldds, P, C);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
