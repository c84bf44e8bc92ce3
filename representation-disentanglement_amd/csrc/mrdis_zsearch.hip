// Batched cosine top-1 over an fp32 gallery with label exclusion: the nearest-neighbour modality-code search of the
// missing-contrast evaluation (reference: model.py:3396-3415 compute_nearest_neighbour_z_by_s / compute_cosine, called per
// query row from main_missing.py:414-426).
//
//   norm(x) = max(sqrt(sum x^2 + 1e-8), 1e-8)          cos(g, q) = sum g*q / (norm(g) * norm(q))
//   out[q]  = argmax over gallery rows n with gallery_label[n] != query_label[q] of cos(g_n, q); equal cos: smaller n
//             (torch.argmax's first occurrence); every row excluded: idx = -1, cos = -inf.
//
// One launch reads the gallery once for all Q <= 64 queries.  Workgroup = 4 waves; a TILE is 128 gallery rows, 32 per wave
// (two 16-row MFMA tiles).  Per 64-wide D-chunk the workgroup stages the query block (Q padded to 16 QT rows) in LDS; each wave
// holds its gallery rows in registers (loaded one chunk ahead) and runs v_mfma_f32_16x16x4_f32 with the gallery as A
// (row = lane & 15, k-slot = lane >> 4) and the queries as B.  A lane loads a float4 of its row at k = 16t + 4h and feeds its
// four components to four MFMA k-steps; the query lane of the same k-slot reads the same k from LDS, so every product meets
// its partner (the k order inside the dot differs from a sequential chain, never between launches).  Gallery norms are summed
// in the same pass from the same registers.  Each row's dot and norm are computed by one wave in a fixed order whatever the
// grid, so out_cos is bit-identical across runs and grid sizes.
//
// Cross-workgroup reduction: every workgroup writes its per-query best (cos, idx) to the workspace, then takes a ticket; the
// last to arrive reduces the partials (lexicographic max of (cos, -idx): associative and exact) and sets the ticket back to 0,
// so the library issues no memset: the caller zeroes the ticket word once when it allocates the workspace.
#include "mrdis_common.h"
#include <climits>

namespace {

constexpr int ZS_THREADS = 256;
constexpr int ZS_WAVES = 4;
constexpr int ZS_RT = 2;                         // 16-row MFMA tiles per wave
constexpr int ZS_TILE = ZS_WAVES * ZS_RT * 16;   // gallery rows per workgroup tile
constexpr int ZS_KC = 64;                        // D-chunk
constexpr int ZS_LDQ = ZS_KC + 4;                // LDS row stride of the staged query chunk (floats): rows start 4 banks apart
constexpr int ZS_MAXQ = 64;
constexpr int ZS_MAX_GRID = 2048;
constexpr size_t ZS_HEAD = 64;                   // ticket word, padded

__device__ __forceinline__ bool zs_better(float c, int n, float bc, int bn) { return c > bc || (c == bc && n < bn); }

template <bool VEC>
__device__ __forceinline__ float4 zs_load4(const float* __restrict__ row, int k, int D) {
    if (VEC) {
        if (k < D) return *reinterpret_cast<const float4*>(row + k);      // D % 4 == 0: k < D covers k + 3
        return make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 v;
    v.x = k < D ? row[k] : 0.f;
    v.y = k + 1 < D ? row[k + 1] : 0.f;
    v.z = k + 2 < D ? row[k + 2] : 0.f;
    v.w = k + 3 < D ? row[k + 3] : 0.f;
    return v;
}

__device__ __forceinline__ float zs_comp(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

template <int QT, bool VEC>
__global__ __launch_bounds__(ZS_THREADS) void zsearch_kernel(const float* __restrict__ G, long long ldg, const int* __restrict__ glab, int N, int D,
                                                             const float* __restrict__ Qm, const int* __restrict__ qlab, int Q,
                                                             int* __restrict__ out_idx, float* __restrict__ out_cos,
                                                             unsigned* ticket, float* part_cos, int* part_idx) {
    __shared__ __attribute__((aligned(16))) float s_q[QT * 16 * ZS_LDQ];
    __shared__ float s_qnorm[ZS_MAXQ];
    __shared__ int s_qlab[ZS_MAXQ];
    __shared__ float s_bc[ZS_WAVES][QT * 16];
    __shared__ int s_bi[ZS_WAVES][QT * 16];
    __shared__ int s_last;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;

    if (tid < Q) s_qlab[tid] = qlab[tid];       // (query norms: summed from the staged chunks, below)

    float best_c[QT];
    int best_i[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) { best_c[qt] = -INFINITY; best_i[qt] = INT_MAX; }

    const int nchunks = (D + ZS_KC - 1) / ZS_KC;
    const int ntiles = (N + ZS_TILE - 1) / ZS_TILE;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int row0 = tile * ZS_TILE + wave * (ZS_RT * 16);
        const float* grow[ZS_RT];
        bool gok[ZS_RT];
#pragma unroll
        for (int rt = 0; rt < ZS_RT; ++rt) {
            const int n = row0 + rt * 16 + r16;
            gok[rt] = n < N;
            grow[rt] = G + (size_t)(gok[rt] ? n : 0) * (size_t)ldg;
        }
        f32x4 acc[QT][ZS_RT];
        float gss[ZS_RT];
#pragma unroll
        for (int rt = 0; rt < ZS_RT; ++rt) {
            gss[rt] = 0.f;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) acc[qt][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float4 gnext[ZS_RT][4], qnext[QT];
        auto load_chunk = [&](int kb) {
#pragma unroll
            for (int rt = 0; rt < ZS_RT; ++rt)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    gnext[rt][t] = gok[rt] ? zs_load4<VEC>(grow[rt], kb + 16 * t + 4 * h, D) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < QT; ++j) {           // staging share of this thread: query row (tid >> 4) + 16 j, float4 column tid & 15
                const int q = (tid >> 4) + 16 * j;
                qnext[j] = q < Q ? zs_load4<VEC>(Qm + (size_t)q * D, kb + 4 * (tid & 15), D) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        float qss[QT];                               // sum of squares of this thread's staging share of query rows (tid >> 4) + 16 j
#pragma unroll
        for (int j = 0; j < QT; ++j) qss[j] = 0.f;
        load_chunk(0);
        for (int c = 0; c < nchunks; ++c) {
            float4 g[ZS_RT][4];
#pragma unroll
            for (int rt = 0; rt < ZS_RT; ++rt)
#pragma unroll
                for (int t = 0; t < 4; ++t) g[rt][t] = gnext[rt][t];
            __syncthreads();                         // every wave is done with the previous chunk's queries
#pragma unroll
            for (int j = 0; j < QT; ++j) {
                *reinterpret_cast<float4*>(&s_q[((tid >> 4) + 16 * j) * ZS_LDQ + 4 * (tid & 15)]) = qnext[j];
                qss[j] = fmaf(qnext[j].x, qnext[j].x, qss[j]); qss[j] = fmaf(qnext[j].y, qnext[j].y, qss[j]);
                qss[j] = fmaf(qnext[j].z, qnext[j].z, qss[j]); qss[j] = fmaf(qnext[j].w, qnext[j].w, qss[j]);
            }
            __syncthreads();
            if (c + 1 < nchunks) load_chunk((c + 1) * ZS_KC);
#pragma unroll
            for (int rt = 0; rt < ZS_RT; ++rt)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    gss[rt] = fmaf(g[rt][t].x, g[rt][t].x, gss[rt]); gss[rt] = fmaf(g[rt][t].y, g[rt][t].y, gss[rt]);
                    gss[rt] = fmaf(g[rt][t].z, g[rt][t].z, gss[rt]); gss[rt] = fmaf(g[rt][t].w, g[rt][t].w, gss[rt]);
                }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float4 b[QT];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) b[qt] = *reinterpret_cast<const float4*>(&s_q[(qt * 16 + r16) * ZS_LDQ + 16 * t + 4 * h]);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int rt = 0; rt < ZS_RT; ++rt)
#pragma unroll
                        for (int qt = 0; qt < QT; ++qt)
                            acc[qt][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(zs_comp(g[rt][t], s), zs_comp(b[qt], s), acc[qt][rt], 0, 0, 0);
            }
        }
        // query norms: the 16 staging threads of a row (one 16-lane group of a wave) combine their sums in a fixed tree; recomputed per tile, same value
#pragma unroll
        for (int j = 0; j < QT; ++j) {
            float ss = qss[j];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) ss += __shfl_xor(ss, o, 64);
            const int q = (tid >> 4) + 16 * j;
            if ((tid & 15) == 0 && q < Q) s_qnorm[q] = fmaxf(sqrtf(ss + 1e-8f), 1e-8f);
        }
        __syncthreads();
        // epilogue of the tile: C[i][j] (i = gallery row 4 (lane >> 4) + reg, j = query lane & 15) -> cosine, exclusion, running best
#pragma unroll
        for (int rt = 0; rt < ZS_RT; ++rt) {
            float ss = gss[rt];
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);            // every k-slot lane of row r16 now holds its full sum, same order everywhere
            const float gn_own = fmaxf(sqrtf(ss + 1e-8f), 1e-8f);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 4 * h + r;
                const float gn = __shfl(gn_own, i, 64);
                const int n = row0 + rt * 16 + i;
                const int lab = n < N ? glab[n] : 0;
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    const int q = qt * 16 + r16;
                    if (n < N && q < Q && lab != s_qlab[q]) {
                        const float cs = acc[qt][rt][r] / (gn * s_qnorm[q]);
                        if (zs_better(cs, n, best_c[qt], best_i[qt])) { best_c[qt] = cs; best_i[qt] = n; }
                    }
                }
            }
        }
    }
    // lanes of one query (same lane & 15) -> one best per wave -> one per workgroup
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float oc = __shfl_xor(best_c[qt], o, 64);
            const int oi = __shfl_xor(best_i[qt], o, 64);
            if (zs_better(oc, oi, best_c[qt], best_i[qt])) { best_c[qt] = oc; best_i[qt] = oi; }
        }
        if (h == 0) { s_bc[wave][qt * 16 + r16] = best_c[qt]; s_bi[wave][qt * 16 + r16] = best_i[qt]; }
    }
    __syncthreads();
    if (tid < Q) {
        float bc = s_bc[0][tid];
        int bi = s_bi[0][tid];
        for (int w = 1; w < ZS_WAVES; ++w)
            if (zs_better(s_bc[w][tid], s_bi[w][tid], bc, bi)) { bc = s_bc[w][tid]; bi = s_bi[w][tid]; }
        const size_t o = (size_t)blockIdx.x * Q + tid;
        __hip_atomic_store(reinterpret_cast<unsigned*>(part_cos) + o, __float_as_uint(bc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part_idx + o, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (tid < Q) {
        float bc = -INFINITY;
        int bi = INT_MAX;
        for (unsigned b = 0; b < gridDim.x; ++b) {
            const size_t o = (size_t)b * Q + tid;
            const float c = __uint_as_float(__hip_atomic_load(reinterpret_cast<unsigned*>(part_cos) + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const int i = __hip_atomic_load(part_idx + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (zs_better(c, i, bc, bi)) { bc = c; bi = i; }
        }
        out_idx[tid] = bi == INT_MAX ? -1 : bi;
        out_cos[tid] = bi == INT_MAX ? -INFINITY : bc;
    }
    if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // ready for the next launch
}

int zs_grid(int N) {
    const int ntiles = mrdis_cdiv(N, ZS_TILE);
    long long g = mrdis_opt(MRDIS_OPT_ZS_GRID);
    if (g <= 0) g = 1024;
    if (g > ZS_MAX_GRID) g = ZS_MAX_GRID;
    return (int)(g < ntiles ? g : ntiles);
}

template <int QT>
void zs_launch(bool vec, int grid, hipStream_t s, const float* G, long long ldg, const int* glab, int N, int D, const float* Qm, const int* qlab, int Q,
               int* out_idx, float* out_cos, unsigned* ticket, float* pc, int* pi) {
    if (vec)
        MRDIS_LAUNCH((zsearch_kernel<QT, true>), dim3(grid), dim3(ZS_THREADS), 0, s, G, ldg, glab, N, D, Qm, qlab, Q, out_idx, out_cos, ticket, pc, pi);
    else
        MRDIS_LAUNCH((zsearch_kernel<QT, false>), dim3(grid), dim3(ZS_THREADS), 0, s, G, ldg, glab, N, D, Qm, qlab, Q, out_idx, out_cos, ticket, pc, pi);
}

}  // namespace

extern "C" size_t mrdis_cosine_top1_workspace(int N, int D, int Q) {
    if (N < 1 || D < 1 || Q < 1 || Q > ZS_MAXQ) return 0;
    const int g = ZS_MAX_GRID < mrdis_cdiv(N, ZS_TILE) ? ZS_MAX_GRID : mrdis_cdiv(N, ZS_TILE);
    return ZS_HEAD + (size_t)2 * sizeof(float) * (size_t)g * (size_t)Q;
}

extern "C" int mrdis_cosine_top1(const float* gallery, long long ldg, const int* gallery_label, int N, int D,
                                 const float* query, const int* query_label, int Q,
                                 int* out_idx, float* out_cos, void* workspace, size_t workspace_bytes, void* stream) {
    if (!gallery || !gallery_label || !query || !query_label || !out_idx || !out_cos || !workspace) return MRDIS_EINVAL;
    if (N < 1 || D < 1 || Q < 1 || Q > ZS_MAXQ || ldg < D) return MRDIS_EINVAL;
    if (workspace_bytes < mrdis_cosine_top1_workspace(N, D, Q)) return MRDIS_EWORKSPACE;
    if ((((uintptr_t)workspace) & 15) != 0) return MRDIS_EALIGN;
    const bool vec = (D & 3) == 0 && (ldg & 3) == 0 && (((uintptr_t)gallery) & 15) == 0 && (((uintptr_t)query) & 15) == 0;
    const int grid = zs_grid(N);
    unsigned* ticket = reinterpret_cast<unsigned*>(workspace);
    float* pc = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + ZS_HEAD);
    int* pi = reinterpret_cast<int*>(pc + (size_t)grid * Q);
    hipStream_t s = (hipStream_t)stream;
    mrdis_count(MRDIS_CNT_ZSEARCH);
    const int QT = (Q + 15) / 16;
    switch (QT) {
        case 1: zs_launch<1>(vec, grid, s, gallery, ldg, gallery_label, N, D, query, query_label, Q, out_idx, out_cos, ticket, pc, pi); break;
        case 2: zs_launch<2>(vec, grid, s, gallery, ldg, gallery_label, N, D, query, query_label, Q, out_idx, out_cos, ticket, pc, pi); break;
        case 3: zs_launch<3>(vec, grid, s, gallery, ldg, gallery_label, N, D, query, query_label, Q, out_idx, out_cos, ticket, pc, pi); break;
        default: zs_launch<4>(vec, grid, s, gallery, ldg, gallery_label, N, D, query, query_label, Q, out_idx, out_cos, ticket, pc, pi); break;
    }
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
