// Kernels of the latent-code options of the reference's loss block (config.yaml:36, 54, 60-61):
//
//  * lambda_kl / is_distri_z: the masked KL term of the modality code, forward and backward, in ONE launch each way
//    (the reference's loss is ~20 ATen ops per direction).  M per-contrast (B, Z) blocks of mu and log-variance, each read
//    through its own device pointer (a host array of M pointers) with a row stride; an optional prior (pmu, plv) of M rows
//    (row i of contrast i, broadcast over the batch when ldp_b = 0, one row per sample otherwise); an (M, B) weight table
//    that carries the mask and the reference's normalisation (computed on the host, so a graph replay redraws it):
//      standard      kl = 0.5 * (exp(lv) + mu^2 - 1 - lv)                                   (model.py:3343-3353)
//      two-Gaussian  kl = 0.5 * (-1 + (plv - lv) + (exp(lv) + (mu - pmu)^2) / exp(plv))     (model.py:3362-3382)
//      loss = sum_{i, b} weight[i][b] * sum_z kl
//    The forward pass is one workgroup with a fixed summation order (bit-identical on every launch and graph replay).  The
//    backward pass reads the upstream gradient from a device scalar (never a host float: a replayed graph would freeze it),
//    writes dmu / dlv element-wise and, for a broadcast prior, dpmu / dplv summed over the batch in a fixed order.
//  * s_compact_method 'mean': F.avg_pool2d(s, k) then view(B, -1) (model.py:3453-3456).  The input is an NHWC view with a row
//    stride; the output is the compact vector in the NCHW order of the pooled map (c, oh, ow), written directly.  Floor
//    semantics: rows / columns at or beyond k * (H // k) are not read and their gradient is exactly 0.
//
// Launch counter families "kl" and "avgpool".
#include "mrdis_common.h"

namespace {

constexpr int KL_THREADS = 256;

inline int lat_grid(long long n, int threads) { long long b = (n + threads - 1) / threads; if (b > 8192) b = 8192; if (b < 1) b = 1; return (int)b; }

struct KLArgs {
    const float* mu[MRDIS_KL_MAXM];
    const float* lv[MRDIS_KL_MAXM];
    float* dmu[MRDIS_KL_MAXM];
    float* dlv[MRDIS_KL_MAXM];
    int ldmu, ldlv, lddmu, lddlv;
    const float* pmu; const float* plv; long long ldp_m; int ldp_b;
    const float* weight;
    int M, B, Z;
};

__device__ __forceinline__ float kl_term(float mu, float lv, float pm, float plv, bool two) {
    if (!two) return 0.5f * (expf(lv) + mu * mu - 1.f - lv);
    const float d = mu - pm;
    return 0.5f * (-1.f + (plv - lv) + (expf(lv) + d * d) / expf(plv));
}

// one workgroup: thread t sums the elements t, t + 256, ... (contrast-major, then sample, then z); the partial sums meet in a fixed tree
__global__ __launch_bounds__(KL_THREADS) void kl_fwd_kernel(KLArgs a, float* __restrict__ loss) {
    __shared__ double red[KL_THREADS];
    const bool two = a.pmu != nullptr;
    const long long per = (long long)a.B * a.Z, n = (long long)a.M * per;
    double s = 0.0;
    for (long long e = threadIdx.x; e < n; e += KL_THREADS) {
        const int i = (int)(e / per);
        const long long r = e - i * per;
        const int b = (int)(r / a.Z), z = (int)(r - (long long)b * a.Z);
        const float w = a.weight[(long long)i * a.B + b];
        const float mu = a.mu[i][(long long)b * a.ldmu + z], lv = a.lv[i][(long long)b * a.ldlv + z];
        float pm = 0.f, plv = 0.f;
        if (two) {
            const long long p = i * a.ldp_m + (long long)b * a.ldp_b + z;
            pm = a.pmu[p]; plv = a.plv[p];
        }
        s += (double)(w * kl_term(mu, lv, pm, plv, two));
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = KL_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)red[0];
}

// blocks [0, eblocks): one thread per (i, b, z) element -> dmu, dlv (and the per-row prior gradient when ldp_b > 0);
// the blocks behind them: one thread per (i, z) of a broadcast prior -> dpmu, dplv summed over b = 0 .. B-1 in order
__global__ __launch_bounds__(KL_THREADS) void kl_bwd_kernel(KLArgs a, const float* __restrict__ dloss, float* __restrict__ dpmu,
                                                            float* __restrict__ dplv, int eblocks) {
    const bool two = a.pmu != nullptr;
    const float g = dloss[0];
    const long long per = (long long)a.B * a.Z, n = (long long)a.M * per;
    if ((int)blockIdx.x < eblocks) {
        for (long long e = blockIdx.x * (long long)KL_THREADS + threadIdx.x; e < n; e += (long long)eblocks * KL_THREADS) {
            const int i = (int)(e / per);
            const long long r = e - i * per;
            const int b = (int)(r / a.Z), z = (int)(r - (long long)b * a.Z);
            const float gw = g * a.weight[(long long)i * a.B + b];
            const float mu = a.mu[i][(long long)b * a.ldmu + z], lv = a.lv[i][(long long)b * a.ldlv + z];
            float dm, dl;
            if (!two) {
                dm = gw * mu;
                dl = gw * 0.5f * (expf(lv) - 1.f);
            } else {
                const long long p = i * a.ldp_m + (long long)b * a.ldp_b + z;
                const float d = mu - a.pmu[p], ep = expf(a.plv[p]), el = expf(lv);
                dm = gw * d / ep;
                dl = gw * 0.5f * (-1.f + el / ep);
                if (a.ldp_b != 0 && dpmu != nullptr) {
                    dpmu[e] = -dm;
                    dplv[e] = gw * 0.5f * (1.f - (el + d * d) / ep);
                }
            }
            a.dmu[i][(long long)b * a.lddmu + z] = dm;
            a.dlv[i][(long long)b * a.lddlv + z] = dl;
        }
        return;
    }
    if (!two || a.ldp_b != 0 || dpmu == nullptr) return;
    for (long long t = (blockIdx.x - eblocks) * (long long)KL_THREADS + threadIdx.x; t < (long long)a.M * a.Z; t += (long long)(gridDim.x - eblocks) * KL_THREADS) {
        const int i = (int)(t / a.Z), z = (int)(t - (long long)i * a.Z);
        const float pm = a.pmu[i * a.ldp_m + z], ep = expf(a.plv[i * a.ldp_m + z]);
        double sm = 0.0, sl = 0.0;
        for (int b = 0; b < a.B; ++b) {
            const float gw = g * a.weight[(long long)i * a.B + b];
            const float mu = a.mu[i][(long long)b * a.ldmu + z], el = expf(a.lv[i][(long long)b * a.ldlv + z]);
            const float d = mu - pm;
            sm += (double)(-(gw * d / ep));
            sl += (double)(gw * 0.5f * (1.f - (el + d * d) / ep));
        }
        dpmu[t] = (float)sm;
        dplv[t] = (float)sl;
    }
}

// ---------------------------------------------------------------- k x k mean pooling, compact-vector output
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int N, int H, int W, int C,
                                                         int k, int Ho, int Wo) {
    const long long total = (long long)N * Ho * Wo * C;
    const float div = (float)(k * k);
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C); long long r = idx / C;
        const int wo = (int)(r % Wo); r /= Wo;
        const int ho = (int)(r % Ho); const int n = (int)(r / Ho);
        float s = 0.f;
        for (int i = 0; i < k; ++i) {
            const float* row = x + ((long long)n * H * W + (long long)(ho * k + i) * W + wo * k) * ldx + c;
            for (int j = 0; j < k; ++j) s += row[(long long)j * ldx];                 // ATen's scan order: window rows, then columns
        }
        y[(long long)n * C * Ho * Wo + ((long long)c * Ho + ho) * Wo + wo] = s / div;
    }
}

__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int lddx, int N, int H, int W, int C,
                                                         int k, int Ho, int Wo) {
    // one thread per element of dx, every element written (no memset in front: graph replay)
    const long long total = (long long)N * H * W * C;
    const float div = (float)(k * k);
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C); long long r = idx / C;
        const int w = (int)(r % W); r /= W;
        const int h = (int)(r % H); const int n = (int)(r / H);
        const int ho = h / k, wo = w / k;
        float v = 0.f;
        if (ho < Ho && wo < Wo) v = dy[(long long)n * C * Ho * Wo + ((long long)c * Ho + ho) * Wo + wo] / div;
        dx[((long long)n * H * W + (long long)h * W + w) * lddx + c] = v;
    }
}

int kl_args(KLArgs& a, const float* const* mu, const float* const* lv, int ldmu, int ldlv, const float* pmu, const float* plv, long long ldp_m,
            int ldp_b, const float* weight, int M, int B, int Z) {
    if (!mu || !lv || !weight || M < 1 || B < 1 || Z < 1 || ldmu < Z || ldlv < Z) return MRDIS_EINVAL;
    if (M > MRDIS_KL_MAXM) return MRDIS_EUNSUPPORTED;
    if ((pmu == nullptr) != (plv == nullptr)) return MRDIS_EINVAL;
    if (pmu != nullptr && (ldp_b < 0 || ldp_m < 0 || (ldp_b != 0 && ldp_b < Z))) return MRDIS_EINVAL;
    a = KLArgs{};
    for (int i = 0; i < M; ++i) {
        if (!mu[i] || !lv[i]) return MRDIS_EINVAL;
        a.mu[i] = mu[i]; a.lv[i] = lv[i];
    }
    a.ldmu = ldmu; a.ldlv = ldlv;
    a.pmu = pmu; a.plv = plv; a.ldp_m = ldp_m; a.ldp_b = ldp_b;
    a.weight = weight; a.M = M; a.B = B; a.Z = Z;
    return MRDIS_OK;
}

}  // namespace

extern "C" int mrdis_kl_fwd(const float* const* mu, const float* const* lv, int ldmu, int ldlv, const float* pmu, const float* plv, long long ldp_m,
                            int ldp_b, const float* weight, float* loss, int M, int B, int Z, void* stream) {
    KLArgs a;
    const int rc = kl_args(a, mu, lv, ldmu, ldlv, pmu, plv, ldp_m, ldp_b, weight, M, B, Z);
    if (rc != MRDIS_OK) return rc;
    if (!loss) return MRDIS_EINVAL;
    mrdis_count(MRDIS_CNT_KL);
    MRDIS_LAUNCH(kl_fwd_kernel, dim3(1), dim3(KL_THREADS), 0, (hipStream_t)stream, a, loss);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_kl_bwd(const float* dloss, const float* const* mu, const float* const* lv, int ldmu, int ldlv, const float* pmu, const float* plv,
                            long long ldp_m, int ldp_b, const float* weight, float* const* dmu, float* const* dlv, int lddmu, int lddlv,
                            float* dpmu, float* dplv, int M, int B, int Z, void* stream) {
    KLArgs a;
    const int rc = kl_args(a, mu, lv, ldmu, ldlv, pmu, plv, ldp_m, ldp_b, weight, M, B, Z);
    if (rc != MRDIS_OK) return rc;
    if (!dloss || !dmu || !dlv || lddmu < Z || lddlv < Z || (dpmu == nullptr) != (dplv == nullptr)) return MRDIS_EINVAL;
    if (dpmu != nullptr && pmu == nullptr) return MRDIS_EINVAL;
    for (int i = 0; i < M; ++i) {
        if (!dmu[i] || !dlv[i]) return MRDIS_EINVAL;
        a.dmu[i] = dmu[i]; a.dlv[i] = dlv[i];
    }
    a.lddmu = lddmu; a.lddlv = lddlv;
    const long long n = (long long)M * B * Z;
    const int eblocks = lat_grid(n, KL_THREADS);
    const int pblocks = (dpmu != nullptr && ldp_b == 0) ? lat_grid((long long)M * Z, KL_THREADS) : 0;
    mrdis_count(MRDIS_CNT_KL);
    MRDIS_LAUNCH(kl_bwd_kernel, dim3(eblocks + pblocks), dim3(KL_THREADS), 0, (hipStream_t)stream, a, dloss, dpmu, dplv, eblocks);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_avgpool_fwd(const float* x, int ldx, float* y, int N, int H, int W, int C, int k, void* stream) {
    if (!x || !y || N < 1 || C < 1 || k < 1 || H < k || W < k || ldx < C) return MRDIS_EINVAL;
    const int Ho = H / k, Wo = W / k;
    mrdis_count(MRDIS_CNT_AVGPOOL);
    MRDIS_LAUNCH(avgpool_fwd_kernel, dim3(lat_grid((long long)N * Ho * Wo * C, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, N, H, W, C, k, Ho, Wo);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" int mrdis_avgpool_bwd(const float* dy, float* dx, int lddx, int N, int H, int W, int C, int k, void* stream) {
    if (!dy || !dx || N < 1 || C < 1 || k < 1 || H < k || W < k || lddx < C) return MRDIS_EINVAL;
    const int Ho = H / k, Wo = W / k;
    mrdis_count(MRDIS_CNT_AVGPOOL);
    MRDIS_LAUNCH(avgpool_bwd_kernel, dim3(lat_grid((long long)N * H * W * C, 256)), dim3(256), 0, (hipStream_t)stream, dy, dx, lddx, N, H, W, C, k, Ho, Wo);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
