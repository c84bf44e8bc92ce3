// Min-plus pass of the squared Euclidean distance transform, out[i] = min_j (g[j] + (i - j)^2), two ways on gfx950 (csrc/mrdis_surfdist.hip uses
// the first):
//   brute     every (i, j) pair over an LDS-resident line, four outputs per thread and sweep (the library's edt_minplus_kernel, TD = 64)
//   envelope  the lower envelope of parabolas in Meijster's integer form: per column one forward scan that keeps a stack of parabolas (s) and
//             of the positions where each takes over (t), then one backward scan that reads the minimum off the stack.  O(n) work per column,
//             but a serial walk with a data-dependent inner loop and one integer division per step; one lane per column, stack in LDS.
// Data: L tiles of n x 64 int32 (a line of n by 64 consecutive d, as a workgroup of the library sees it), 70 % "no feature" (2^30), the rest
// squared distances up to 150^2; every eighth tile has no feature at all.  Both kernels read and write the same bytes; the outputs must agree.
// hipcc --offload-arch=gfx950 -O3 -o edt_envelope edt_envelope.hip && ./edt_envelope [n = 240] [L = 17280]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

constexpr unsigned FAR = 1u << 30;
constexpr int TD = 64;

__global__ __launch_bounds__(256) void brute(const unsigned* __restrict__ in, unsigned* __restrict__ out, int n) {
    extern __shared__ unsigned tile[];                               // [n][TD]
    const unsigned* src = in + (size_t)blockIdx.x * n * TD;
    unsigned* dst = out + (size_t)blockIdx.x * n * TD;
    for (int idx = threadIdx.x; idx < n * TD; idx += 256) tile[idx] = src[idx];
    __syncthreads();
    const int dd = threadIdx.x & 63, ig = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int i0 = ig * 4; i0 < n; i0 += 16) {
        unsigned acc[4] = {FAR, FAR, FAR, FAR};
        for (int j = 0; j < n; ++j) {
            const unsigned gj = tile[j * TD + dd];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int di = i0 + t - j;
                acc[t] = min(acc[t], gj + (unsigned)(di * di));
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (i0 + t < n) dst[(i0 + t) * TD + dd] = min(acc[t], FAR);
    }
}

// one wave per tile, lane = column.  LDS: g [n][64] int32, s and t [n][64] uint16.
__global__ __launch_bounds__(64) void envelope(const unsigned* __restrict__ in, unsigned* __restrict__ out, int n) {
    extern __shared__ unsigned tile[];
    unsigned short* sv = reinterpret_cast<unsigned short*>(tile + n * TD);
    unsigned short* tv = sv + n * TD;
    const unsigned* src = in + (size_t)blockIdx.x * n * TD;
    unsigned* dst = out + (size_t)blockIdx.x * n * TD;
    const int dd = threadIdx.x;
    for (int j = 0; j < n; ++j) tile[j * TD + dd] = src[j * TD + dd];
    auto f = [&](int x, int i) { const int di = x - i; return tile[i * TD + dd] + (unsigned)(di * di); };
    int q = 0;
    sv[dd] = 0; tv[dd] = 0;
    for (int u = 1; u < n; ++u) {
        while (q >= 0) {
            const int tq = tv[q * TD + dd], sq = sv[q * TD + dd];
            if (f(tq, sq) > f(tq, u)) --q; else break;
        }
        if (q < 0) {
            q = 0; sv[dd] = (unsigned short)u;                       // (t[0] stays 0)
        } else {
            const int i = sv[q * TD + dd];
            const unsigned num = (unsigned)(u * u - i * i) + tile[u * TD + dd] - tile[i * TD + dd];      // >= 0: parabola i is not above u at t[q]
            const unsigned w = 1u + num / (unsigned)(2 * (u - i));
            if (w < (unsigned)n) { ++q; sv[q * TD + dd] = (unsigned short)u; tv[q * TD + dd] = (unsigned short)w; }
        }
    }
    for (int u = n - 1; u >= 0; --u) {
        dst[u * TD + dd] = min(f(u, sv[q * TD + dd]), FAR);
        if (u == tv[q * TD + dd]) --q;
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 240;
    const int L = argc > 2 ? atoi(argv[2]) : 17280;                  // 6 sources x 4 samples x 240 lines x 3 d tiles
    if (n < 1 || n > 300 || L < 1 || L > 40000) { printf("n in 1 .. 300, L in 1 .. 40000\n"); return 1; }
    const size_t count = (size_t)L * n * TD;
    std::vector<unsigned> h(count);
    unsigned long long st = 88172645463325252ull;
    for (size_t k = 0; k < count; ++k) {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        const bool empty_tile = (k / ((size_t)n * TD)) % 8 == 7;
        h[k] = (empty_tile || (st >> 33) % 10 < 7) ? FAR : (unsigned)((st >> 40) % 22501);
    }
    unsigned *din, *da, *db;
    CK(hipMalloc(&din, count * 4)); CK(hipMalloc(&da, count * 4)); CK(hipMalloc(&db, count * 4));
    CK(hipMemcpy(din, h.data(), count * 4, hipMemcpyHostToDevice));
    const size_t lds_b = (size_t)n * TD * 4, lds_e = (size_t)n * TD * 8;
    CK(hipFuncSetAttribute((const void*)brute, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    CK(hipFuncSetAttribute((const void*)envelope, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_e));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int rep = 0; rep < 3; ++rep) {                              // alternating windows
        float ms;
        CK(hipEventRecord(e0));
        for (int k = 0; k < 3; ++k) hipLaunchKernelGGL(brute, dim3(L), dim3(256), lds_b, 0, din, da, n);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        printf("window %d: brute %.1f us", rep, ms * 1e3 / 3);
        CK(hipEventRecord(e0));
        for (int k = 0; k < 3; ++k) hipLaunchKernelGGL(envelope, dim3(L), dim3(64), lds_e, 0, din, db, n);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        printf("   envelope %.1f us   (n %d, %d tiles of %d x %d, %.0f MB read + written per call)\n", ms * 1e3 / 3, n, L, n, TD, count * 8 / 1e6);
    }
    CK(hipGetLastError());
    std::vector<unsigned> a(count), b(count);
    CK(hipMemcpy(a.data(), da, count * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), db, count * 4, hipMemcpyDeviceToHost));
    size_t differ = 0, far = 0;
    for (size_t k = 0; k < count; ++k) { differ += a[k] != b[k]; far += a[k] == FAR; }
    printf("outputs that differ: %zu of %zu (%zu are 2^30: tiles without a feature)\n", differ, count, far);
    return differ != 0;
}
