// What the two batch gathers of the 3-D store share (mrdis_volgather.hip: the reference's depth crop; mrdis_patch.hip: random patches):
// the per-element rules of an item -- T_b, the label rule, the region channels -- the shape of the LDS tile and its store phase.
// The rules are documented where they were first written, in the header comment of mrdis_volgather.hip.
#pragma once
#include "mrdis_common.h"

constexpr int VG_TILE_FLOATS = 8192;        // 32 KB tile: P = 1024 positions at C <= 8, 512 at C <= 16, 256 at C <= 32
constexpr int VG_MAXC_TILE = 32;
constexpr int VG_LDS_FLOATS = VG_TILE_FLOATS + VG_MAXC_TILE * 4;

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

// positions per tile and the row stride of the [C][S] LDS tile: a lane's four reads of the store phase sit 4 S apart per neighbouring lane at
// C = 8 (S % 8 == 4 puts the two rows on opposite halves of the 32 banks) and at C = 16 (S % 8 == 2: four rows, 8 banks apart); C = 4 reads
// whole rows and needs none
static inline void vg_tile_shape(int C, int* P, int* S) {
    int p = VG_TILE_FLOATS / C / 256 * 256; if (p > 1024) p = 1024;
    *P = p;
    *S = p + ((C % 16) == 0 ? 2 : (C % 8) == 0 ? 4 : (C % 4) == 0 ? 0 : 1);
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
