// Connected components of label volumes and the clean-up rules built on them (postproc.components3d / postproc.clean_labels).  Integer
// arithmetic only: exact, and the same bits from run to run.  Volumes are (B, H, W, D) uint8 with D contiguous, as mrdis_seg_label_volume
// writes its labels.  A voxel is FOREGROUND iff its label l is at most 7 and bit l of fg_mask is set; every other voxel is background and is
// never joined to anything.  Connectivity 6 / 18 / 26; components never cross a sample and never wrap from the end of a line, row or plane
// into the next (every neighbour is addressed by its coordinates, which are checked against H, W, D).
//
//   mrdis_cc_label   comp[v] = the smallest in-sample flat index (h W + w) D + d of v's component (-1 on background),
//                    size[v] = the component's voxel count where comp[v] == v, 0 elsewhere.  THREE launches, whatever B, shape and content:
//     1 cc_local_kernel     a workgroup owns a tile of 4 x 4 x 64 voxels (a wave = one run of 64 contiguous bytes).  Union-find over the
//                           tile in LDS, then every voxel stores the GLOBAL index of its tile-local root into comp (the parent forest) and
//                           0 into size.  Local and global indices are both lexicographic in (h, w, d), so the smallest local index of a
//                           set is also its smallest global one: a parent never exceeds its child, in LDS and in memory alike.
//     2 cc_merge_kernel     the same tiling; a voxel on a tile face unions itself with each foreground FORWARD neighbour (3 / 9 / 13 of the
//                           6 / 18 / 26 offsets: the other half is the same pair seen from the other side) that lies in another tile.
//     3 cc_compress_kernel  comp[v] = root of v, and size[root] += the voxels of the wave that share that root (one atomicAdd per distinct
//                           root and wave).
//   mrdis_cc_clean   the three rules of postproc.clean_labels on (labels, comp, size): FOUR launches (clear, scan the roots, apply the
//                    keep rule, apply the enhancing-tumour rule), whatever the arguments.
//
// No workgroup ever waits for another: there is no grid barrier, no cooperative launch, no flag and no spin on a word another workgroup
// writes.  The only cross-workgroup primitive is the lock-free union (cc_union): find both roots, atomicMin the LARGER root's parent to the
// smaller; if the atomic returns anything but that root, somebody else re-parented it first and the walk continues from the value returned.
// Every iteration replaces an index by a strictly smaller one (a parent is never above its child, and the returned value is below the
// root it replaced), indices are bounded below by 0, so every loop ends by construction, whatever any other workgroup does or does not do.
//
// Visibility.  The per-XCD L2s are not coherent for plain loads within a launch, and a CU's L1 is never refreshed by another CU's stores.
// During the merge every parent is read with an agent-scope atomic load (L1 bypassed) and written only by atomicMin; what DECIDES a union is
// the value atomicMin returns, which is the word's true content at the L2 / memory that serialises the atomics.  A stale parent can only be
// an EARLIER parent of the same voxel, i.e. an index that was an ancestor then and, since links are only ever redirected to members of the
// same set with smaller index after their old target was united with the new one, still belongs to the same final component: it may lengthen
// a walk, it never decides a result.  Final comp values are produced by launch 3, after the kernel boundary behind the last union.  Launch 3
// compresses in place: a concurrent reader sees either the old parent or the final root of a voxel, both ancestors (relaxed agent-scope
// atomics both ways: no torn or register-cached word); roots (comp[v] == v) are never rewritten.  size is zeroed by launch 1 and only
// added to by launch 3; mrdis_cc_clean reads comp, size and its own counters only across kernel boundaries.
#include "mrdis_common.h"

namespace {
constexpr int CC_THREADS = 256;
constexpr int CC_TH = 4, CC_TW = 4, CC_TD = 64;                  // the tile: CC_TD is the wave, (CC_TH, CC_TW) the wave index and the voxel of a thread
constexpr int CC_TILE = CC_TH * CC_TW * CC_TD;
constexpr int CC_VPT = CC_TILE / CC_THREADS;                     // voxels per thread = CC_TH: thread t owns (lh = k, lw = t / 64, ld = t % 64)
constexpr int CC_MAX_BLOCKS = 2048;                              // 256 CUs x 8 workgroups, for the grid-stride passes
constexpr int CC_MAX_EXTENT = 1024;
static_assert(CC_TD == 64 && CC_TW * CC_TD == CC_THREADS && CC_VPT == CC_TH, "thread <-> voxel mapping of the tile kernels");

// forward half of the 26 offsets (dh, dw, dd), lexicographically positive: 3 faces, then 6 edges, then 4 corners
__constant__ signed char cc_fwd[13][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0},
                                          {0, 1, -1}, {0, 1, 1}, {1, 0, -1}, {1, 0, 1}, {1, -1, 0}, {1, 1, 0},
                                          {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};

struct CcGeom {
    int H, W, D;
    int tw, td;             // tiles along W and D
    int nfwd;               // 3 | 9 | 13
    unsigned fg;            // bit l: label l is foreground
    long long P;            // voxels per sample
};

// ---- union-find over int parents, p[x] <= x, a root has p[x] == x.  SCOPE: workgroup for LDS, agent for memory.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* p, int x) {
    for (;;) {
        const int q = __hip_atomic_load(p + x, __ATOMIC_RELAXED, SCOPE);
        if (q >= x) return x;                                    // q == x: a root (q > x never happens)
        x = q;                                                   // strictly smaller
    }
}
template <int SCOPE>
__device__ __forceinline__ void cc_union(int* p, int a, int b) {
    for (;;) {
        a = cc_find<SCOPE>(p, a);
        b = cc_find<SCOPE>(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }            // a: the larger root
        const int old = atomicMin(p + a, b);
        if (old == a) return;                                    // a was still a root and now hangs below b
        a = old;                                                 // somebody re-parented a to old < a first: unite old and b instead
    }
}

__device__ __forceinline__ void cc_tile_origin(const CcGeom& g, int& h0, int& w0, int& d0) {
    const int t = blockIdx.x;
    const int per_h = g.tw * g.td;
    const int th = t / per_h, r = t - th * per_h;
    const int tw = r / g.td;
    h0 = th * CC_TH; w0 = tw * CC_TW; d0 = (r - tw * g.td) * CC_TD;
}

// grid (tiles, B).  comp <- the parent forest of the tile-local components (global indices), size <- 0
__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const unsigned char* __restrict__ labels, int* __restrict__ comp, int* __restrict__ size,
                                                              CcGeom g) {
    __shared__ int lp[CC_TILE];
    int h0, w0, d0;
    cc_tile_origin(g, h0, w0, d0);
    const long long base = (long long)blockIdx.y * g.P;
    const int lw = threadIdx.x >> 6, ld = threadIdx.x & 63;
    const int w = w0 + lw, d = d0 + ld;
    bool in[CC_VPT], fg[CC_VPT];
#pragma unroll
    for (int k = 0; k < CC_VPT; ++k) {
        const int h = h0 + k;
        in[k] = h < g.H && w < g.W && d < g.D;
        unsigned l = 255u;
        if (in[k]) l = labels[base + ((long long)h * g.W + w) * g.D + d];
        fg[k] = l <= 7u && ((g.fg >> l) & 1u) != 0u;
        const int li = k * CC_THREADS + threadIdx.x;
        lp[li] = fg[k] ? li : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_VPT; ++k) {
        if (!fg[k]) continue;
        const int li = k * CC_THREADS + threadIdx.x;
        for (int o = 0; o < g.nfwd; ++o) {
            const int nh = k + cc_fwd[o][0], nw = lw + cc_fwd[o][1], nd = ld + cc_fwd[o][2];
            if (nh >= CC_TH || nw < 0 || nw >= CC_TW || nd < 0 || nd >= CC_TD) continue;      // another tile: cc_merge_kernel
            const int ni = (nh * CC_TW + nw) * CC_TD + nd;
            if (lp[ni] < 0) continue;                            // background (or beyond the volume); the sign never changes
            cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, li, ni);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_VPT; ++k) {
        if (!in[k]) continue;
        const long long v = base + ((long long)(h0 + k) * g.W + w) * g.D + d;
        int root = -1;
        if (fg[k]) {
            const int r = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, k * CC_THREADS + threadIdx.x);
            root = ((h0 + (r >> 8)) * g.W + (w0 + ((r >> 6) & 3))) * g.D + (d0 + (r & 63));
        }
        comp[v] = root;
        size[v] = 0;
    }
}

// grid (tiles, B).  Unions across tile faces; par is comp of the launch before.
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(int* par, CcGeom g) {
    int h0, w0, d0;
    cc_tile_origin(g, h0, w0, d0);
    int* p = par + (long long)blockIdx.y * g.P;
    const int lw = threadIdx.x >> 6, ld = threadIdx.x & 63;
    const int w = w0 + lw, d = d0 + ld;
    if (w >= g.W || d >= g.D) return;
#pragma unroll
    for (int k = 0; k < CC_VPT; ++k) {
        const int h = h0 + k;
        if (h >= g.H) break;
        if (k != CC_TH - 1 && lw != 0 && lw != CC_TW - 1 && ld != 0 && ld != CC_TD - 1) continue;      // no forward neighbour outside the tile
        const int v = (h * g.W + w) * g.D + d;
        if (__hip_atomic_load(p + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
        for (int o = 0; o < g.nfwd; ++o) {
            const int nh = h + cc_fwd[o][0], nw = w + cc_fwd[o][1], nd = d + cc_fwd[o][2];
            if (nh >= g.H || nw < 0 || nw >= g.W || nd < 0 || nd >= g.D) continue;              // beyond the sample: nothing to join, nothing wraps
            if (nh < h0 + CC_TH && nw >= w0 && nw < w0 + CC_TW && nd >= d0 && nd < d0 + CC_TD) continue;      // this tile: done in LDS
            const int n = (nh * g.W + nw) * g.D + nd;
            if (__hip_atomic_load(p + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
            cc_union<__HIP_MEMORY_SCOPE_AGENT>(p, v, n);
        }
    }
}

// grid (gx, B), grid-stride.  comp[v] <- root(v) in place, size[root] += count
__global__ __launch_bounds__(CC_THREADS) void cc_compress_kernel(int* comp, int* size, long long P) {
    int* p = comp + (long long)blockIdx.y * P;
    int* sz = size + (long long)blockIdx.y * P;
    const int lane = threadIdx.x & 63;
    for (long long i0 = (long long)blockIdx.x * CC_THREADS; i0 < P; i0 += (long long)gridDim.x * CC_THREADS) {      // (the trip count is uniform over the workgroup)
        const long long v = i0 + threadIdx.x;
        int root = -1;
        if (v < P) {
            const int q = __hip_atomic_load(p + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (q >= 0) {
                root = cc_find<__HIP_MEMORY_SCOPE_AGENT>(p, q);
                if (root != q) __hip_atomic_store(p + v, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        unsigned long long todo = __builtin_amdgcn_ballot_w64(root >= 0);
        while (todo != 0ull) {                                   // one add per distinct root of the wave
            const int leader = __builtin_ctzll(todo);
            const int r = __shfl(root, leader, 64);
            const unsigned long long same = __builtin_amdgcn_ballot_w64(root == r);
            if (lane == leader) atomicAdd(sz + r, (int)__builtin_popcountll(same));
            todo &= ~same;
        }
    }
}

// ---------------------------------------------------------------------------------------------- clean
constexpr int CC_NSTAT = 6;          // components, kept, foreground, removed, n of the ET rule, replaced

__device__ __forceinline__ int cc_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// sum over the workgroup of N per-thread counts, then one atomicAdd per non-zero count; red: [CC_THREADS / 64][N]
template <int N>
__device__ __forceinline__ void cc_block_add(const int (&cnt)[N], int (*red)[N], int* dst, const int (&col)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int v = cc_wave_sum(cnt[i]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        const int v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (v != 0) atomicAdd(dst + col[threadIdx.x], v);
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_clear_kernel(int* __restrict__ stats, unsigned long long* __restrict__ best, int B) {
    const int i = blockIdx.x * CC_THREADS + threadIdx.x;
    if (i < B * CC_NSTAT) stats[i] = 0;
    if (i < B) best[i] = 0ull;
}

// the largest component of a sample, a size tie going to the smaller root: the maximum of (size << 32) | (2^31 - 1 - root); 0 = no component
__device__ __forceinline__ unsigned long long cc_key(int sz, int root) { return ((unsigned long long)(unsigned)sz << 32) | (unsigned)(0x7fffffff - root); }

// grid (gx, B): stats[0] += roots, stats[2] += foreground voxels, best = max key over the roots
__global__ __launch_bounds__(CC_THREADS) void cc_scan_kernel(const int* __restrict__ comp, const int* __restrict__ size, int* __restrict__ stats,
                                                             unsigned long long* __restrict__ best, long long P) {
    __shared__ int red[CC_THREADS / 64][2];
    __shared__ unsigned long long kred[CC_THREADS / 64];
    const int b = blockIdx.y;
    const int* c = comp + (long long)b * P;
    const int* s = size + (long long)b * P;
    int cnt[2] = {0, 0};
    unsigned long long key = 0ull;
    for (long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x; v < P; v += (long long)gridDim.x * CC_THREADS) {
        const int r = c[v];
        if (r < 0) continue;
        cnt[1] += 1;
        if ((long long)r == v) {
            cnt[0] += 1;
            const unsigned long long k = cc_key(s[v], r);
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k = __shfl_down(key, o, 64);
        key = k > key ? k : key;
    }
    if ((threadIdx.x & 63) == 0) kred[threadIdx.x >> 6] = key;
    const int col[2] = {0, 2};
    cc_block_add<2>(cnt, red, stats + b * CC_NSTAT, col);         // (its barrier also covers kred)
    if (threadIdx.x == 0) {
        unsigned long long k = kred[0];
#pragma unroll
        for (int i = 1; i < CC_THREADS / 64; ++i) k = kred[i] > k ? kred[i] : k;
        if (k != 0ull) atomicMax(best + b, k);
    }
}

struct CcClean { int min_voxels, keep_largest, et_label, et_min_voxels, et_replace; };

// grid (gx, B): the keep rule.  out <- labels, 0 on the voxels of components that are not kept; stats[1] += kept roots, [3] += removed voxels,
// [4] += voxels whose label is now et_label
__global__ __launch_bounds__(CC_THREADS) void cc_keep_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ comp,
                                                             const int* __restrict__ size, const unsigned long long* __restrict__ best,
                                                             unsigned char* __restrict__ out, int* __restrict__ stats, long long P, CcClean a) {
    __shared__ int red[CC_THREADS / 64][3];
    const int b = blockIdx.y;
    const long long base = (long long)b * P;
    const int* c = comp + base;
    const int* s = size + base;
    const unsigned long long k = best[b];
    const int best_root = k != 0ull ? 0x7fffffff - (int)(unsigned)(k & 0xffffffffull) : -1;
    int cnt[3] = {0, 0, 0};
    for (long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x; v < P; v += (long long)gridDim.x * CC_THREADS) {
        unsigned char l = labels[base + v];
        const int r = c[v];
        if (r >= 0) {
            const bool kept = s[r] >= a.min_voxels && (a.keep_largest == 0 || r == best_root);
            if (kept) { cnt[0] += (long long)r == v ? 1 : 0; }
            else { l = 0; cnt[1] += 1; }
        }
        cnt[2] += (int)l == a.et_label ? 1 : 0;
        out[base + v] = l;
    }
    const int col[3] = {1, 3, 4};
    cc_block_add<3>(cnt, red, stats + b * CC_NSTAT, col);
}

// grid (gx, B): the ET rule on `out`, decided by n = stats[4] of the launch before
__global__ __launch_bounds__(CC_THREADS) void cc_et_kernel(unsigned char* __restrict__ out, int* __restrict__ stats, long long P, CcClean a) {
    const int b = blockIdx.y;
    const int n = stats[b * CC_NSTAT + 4];
    if (a.et_min_voxels <= 0 || n <= 0 || n >= a.et_min_voxels) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[b * CC_NSTAT + 5] = 1;
    unsigned char* o = out + (long long)b * P;
    for (long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x; v < P; v += (long long)gridDim.x * CC_THREADS)
        if ((int)o[v] == a.et_label) o[v] = (unsigned char)a.et_replace;
}

bool cc_geometry_ok(int B, int H, int W, int D) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || D < 1 || H > CC_MAX_EXTENT || W > CC_MAX_EXTENT || D > CC_MAX_EXTENT) return false;
    return (long long)H * W * D < (1LL << 31);
}
unsigned cc_stride_blocks(long long P, int B) {
    long long nb = (P + CC_THREADS - 1) / CC_THREADS, cap = CC_MAX_BLOCKS / B;
    if (cap < 1) cap = 1;
    return (unsigned)(nb > cap ? cap : nb);
}
}  // namespace

extern "C" int mrdis_cc_label(const unsigned char* labels, int fg_mask, int connectivity, int* comp, int* size, int B, int H, int W, int D,
                              void* stream) {
    if (!cc_geometry_ok(B, H, W, D)) return MRDIS_EUNSUPPORTED;
    if (!labels || !comp || !size || fg_mask < 2 || fg_mask > 255 || (fg_mask & 1) != 0) return MRDIS_EINVAL;
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return MRDIS_EINVAL;
    if (((((uintptr_t)comp) | ((uintptr_t)size)) & 3) != 0) return MRDIS_EALIGN;
    CcGeom g;
    g.H = H; g.W = W; g.D = D; g.P = (long long)H * W * D;
    g.tw = mrdis_cdiv(W, CC_TW); g.td = mrdis_cdiv(D, CC_TD);
    g.nfwd = connectivity == 6 ? 3 : connectivity == 18 ? 9 : 13;
    g.fg = (unsigned)fg_mask;
    const unsigned tiles = (unsigned)mrdis_cdiv(H, CC_TH) * (unsigned)g.tw * (unsigned)g.td;
    hipStream_t s = (hipStream_t)stream;
    mrdis_count(MRDIS_CNT_CCLABEL);
    MRDIS_LAUNCH(cc_local_kernel, dim3(tiles, B), dim3(CC_THREADS), 0, s, labels, comp, size, g);
    MRDIS_CHECK_LAUNCH();
    mrdis_count(MRDIS_CNT_CCLABEL);
    MRDIS_LAUNCH(cc_merge_kernel, dim3(tiles, B), dim3(CC_THREADS), 0, s, comp, g);
    MRDIS_CHECK_LAUNCH();
    mrdis_count(MRDIS_CNT_CCLABEL);
    MRDIS_LAUNCH(cc_compress_kernel, dim3(cc_stride_blocks(g.P, B), B), dim3(CC_THREADS), 0, s, comp, size, g.P);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}

extern "C" size_t mrdis_cc_clean_workspace(int B) { return B >= 1 && B <= 65535 ? (size_t)B * 8 : 0; }

extern "C" int mrdis_cc_clean(const unsigned char* labels, const int* comp, const int* size, int min_voxels, int keep_largest, int et_label,
                              int et_min_voxels, int et_replace, unsigned char* out, int* stats, void* workspace, size_t workspace_bytes, int B,
                              int H, int W, int D, void* stream) {
    if (!cc_geometry_ok(B, H, W, D)) return MRDIS_EUNSUPPORTED;
    if (!labels || !comp || !size || !out || !stats || !workspace) return MRDIS_EINVAL;
    if (min_voxels < 0 || et_min_voxels < 0 || (keep_largest != 0 && keep_largest != 1) || et_label < 0 || et_label > 7 || et_replace < 0 ||
        et_replace > 7)
        return MRDIS_EINVAL;
    if (workspace_bytes < mrdis_cc_clean_workspace(B)) return MRDIS_EWORKSPACE;
    if (((((uintptr_t)comp) | ((uintptr_t)size) | ((uintptr_t)stats)) & 3) != 0 || (((uintptr_t)workspace) & 7) != 0) return MRDIS_EALIGN;
    const long long P = (long long)H * W * D;
    unsigned long long* best = reinterpret_cast<unsigned long long*>(workspace);
    CcClean a;
    a.min_voxels = min_voxels; a.keep_largest = keep_largest; a.et_label = et_label; a.et_min_voxels = et_min_voxels; a.et_replace = et_replace;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cc_stride_blocks(P, B), B);
    mrdis_count(MRDIS_CNT_CCCLEAN);
    MRDIS_LAUNCH(cc_clear_kernel, dim3(mrdis_cdiv((long long)B * CC_NSTAT, CC_THREADS)), dim3(CC_THREADS), 0, s, stats, best, B);
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(cc_scan_kernel, grid, dim3(CC_THREADS), 0, s, comp, size, stats, best, P);
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(cc_keep_kernel, grid, dim3(CC_THREADS), 0, s, labels, comp, size, (const unsigned long long*)best, out, stats, P, a);
    MRDIS_CHECK_LAUNCH();
    MRDIS_LAUNCH(cc_et_kernel, grid, dim3(CC_THREADS), 0, s, out, stats, P, a);
    MRDIS_CHECK_LAUNCH();
    return MRDIS_OK;
}
