// Device-side primitives shared by the kernels of libmrdis_hip (gfx950 only), each defined ONCE: vector types, buffer descriptors, LDS-DMA copies,
// the half-wave pairing of bf16 stores, bf16 <-> fp32 loads / stores, the sigmoid and the three-term bf16 split.  A new kernel uses these instead of a copy under
// a prefix of its own; what is local to one kernel (tile constants, its body) stays in that kernel's file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ------------------------------------------------------------------ vector types
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte access at 4-byte alignment
typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32u1 __attribute__((aligned(1)));                        // a 4-byte access at any alignment (global memory: one dword instruction)

// ------------------------------------------------------------------ buffer descriptors
// Word 3 of a gfx950 raw buffer descriptor: DATA_FORMAT = 32 bit (bits 15..18 = 4), no stride, no swizzle; an access whose byte offset is not below
// `bytes` (word 2) reads zeros / is dropped -- what the kernels use for zero padding, ragged tiles and tails.
constexpr int MRDIS_BUFFER_RSRC_WORD3 = 0x00020000;
// build it from wave-uniform values only (cdna_hip_programming.md T20)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mrdis_buffer_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, (int)bytes, MRDIS_BUFFER_RSRC_WORD3);
}
// bytes of an N x H x W NHWC view of C channels (elem bytes each) whose pixels are ld elements apart: up to the last pixel's last channel
__device__ __forceinline__ unsigned mrdis_nhwc_bytes(int N, int H, int W, int ld, int C, int elem) {
    return (unsigned)((long long)elem * ((long long)(N * H) * W - 1) * ld + (long long)elem * C);
}

// ------------------------------------------------------------------ LDS-DMA copies (16 bytes per lane, straight from memory into LDS)
// Written as inline assembly: through the builtin hipcc puts `s_waitcnt vmcnt(0)` in front of EVERY later LDS read of the kernel (it cannot tell which
// LDS bytes the copy lands on); inline assembly is invisible to its wait-count pass, so the caller waits for its own copies (vmcnt) before the barrier
// that publishes them.  M0 (the wave's LDS base of the copy, lane l lands at m0v + 16 l) is the compiler's: saved, written and restored inside the one
// statement that reads it.  m0v and src / rs are wave-uniform.
__device__ __forceinline__ void mrdis_lds_dma16(unsigned m0v, unsigned voff, const void* src) {         // lane: 16 bytes at src + voff
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "s"(m0v), "v"(voff), "s"(src) : "memory");
}
__device__ __forceinline__ void mrdis_buffer_lds_dma16(unsigned m0v, unsigned voff, const __amdgpu_buffer_rsrc_t& rs) {   // the same through a descriptor
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(m0v), "s"(rs) : "memory");
}
// the builtin form (the compiler tracks it with vmcnt and waits before the LDS reads): lane l lands at lds + 16 l, lds wave-uniform
__device__ __forceinline__ void mrdis_lds_copy16(const void* src, void* lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}

// ------------------------------------------------------------------ small helpers
// an index the compiler may not fold into the addresses computed from it (keeps a pipeline stage's LDS bases in one register + immediate offsets)
__device__ __forceinline__ int mrdis_opaque(int idx) { asm volatile("" : "+v"(idx)); return idx; }

// The two half-waves of a lane pair (e, half) hold the cout groups 8 q + 4 half .. + 3 of one position: two 8-byte pieces per 8 couts.  Swapping
// group q of the upper half with group q + 1 of the lower half (v_permlane32_swap, one instruction per dword) leaves every lane with 8
// CONSECUTIVE couts -- half 0: 8 q .. 8 q + 7, half 1: 8 (q + 1) .. 8 (q + 1) + 7 -- i.e. one 16-byte store per lane where there were two 8-byte
// stores: half as many write requests of twice the size reach L2 (tools/micro/store_pattern.hip).
__device__ __forceinline__ u32x4 mrdis_pair8(u32x2 gq, u32x2 gq1) {
    const auto s0 = __builtin_amdgcn_permlane32_swap(gq[0], gq1[0], false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(gq[1], gq1[1], false, false);
    return u32x4{s0[0], s1[0], s0[1], s1[1]};
}

// activations are stored as fp32 or bf16, the arithmetic is fp32 either way: convert on load / store (bf16 stores round to nearest even)
__device__ __forceinline__ float4 mrdis_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 mrdis_ld4(const __bf16* p) {
    const bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
    return make_float4((float)t[0], (float)t[1], (float)t[2], (float)t[3]);
}
__device__ __forceinline__ void mrdis_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void mrdis_st4(__bf16* p, float4 v) {
    bf16x4 t; t[0] = (__bf16)v.x; t[1] = (__bf16)v.y; t[2] = (__bf16)v.z; t[3] = (__bf16)v.w;
    *reinterpret_cast<bf16x4*>(p) = t;
}
__device__ __forceinline__ float mrdis_ld1(const float* p) { return *p; }
__device__ __forceinline__ float mrdis_ld1(const __bf16* p) { return (float)*p; }

// the fp32 sigmoid torch computes: accurate expf and an IEEE division.  The objective, the segmentation counts and the sliding-window accumulation
// (mrdis_loss3d.hip, mrdis_segvol.hip) must agree on which side of 0.5 a probability falls, so they share this one.
__device__ __forceinline__ float mrdis_sigmoid(float u) { return 1.f / (1.f + expf(-u)); }

// ------------------------------------------------------------------ region membership of a label value
// lut: eight nibbles built on the host, bit r of nibble l = label l belongs to region r.  A predicted label above 7 and a ground-truth value that
// is NaN, negative, above 7 or non-integral belong to no region.  mrdis_surfdist.hip (surfaces, counts) and mrdis_lesion.hip (planes) share it.
__device__ __forceinline__ unsigned mrdis_region_nib(unsigned char l, unsigned lut) { return l <= 7 ? (lut >> (4 * l)) & 15u : 0u; }
__device__ __forceinline__ unsigned mrdis_region_nib(float t, unsigned lut) {
    if (!(t >= 0.f && t <= 7.f)) return 0u;                         // NaN, negative, above 7: no region
    const int l = (int)t;
    return t == (float)l ? (lut >> (4 * l)) & 15u : 0u;             // non-integral: no region
}

// ------------------------------------------------------------------ three-term bf16 split
// v = h + m + l, each term the bf16 rounding (to nearest even) of what the terms before it left: 3 x 8 mantissa bits.  With both operands of a
// product split this way, the six products of order <= 2 (h h, m h, h m, l h, h l, m m) on the bf16 matrix pipe are fp32-equivalent: what is
// dropped is below 2^-23 of the product.  This is the arithmetic of every split6 kernel.
__device__ __forceinline__ void mrdis_split3(float v, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)v; const float r1 = v - (float)h; m = (__bf16)r1; l = (__bf16)(r1 - (float)m);
}
// the terms into element c of three bf16 vectors (V = bf16x4 | bf16x8); h and m are placed before l is formed.  Same values as the scalar form, another
// statement order: the compiler schedules the two differently, so a kernel that was tuned with one keeps calling that one.
template <typename V>
__device__ __forceinline__ void mrdis_split3(float v, V& h, V& m, V& l, int c) {
    const __bf16 h_ = (__bf16)v; const float r1 = v - (float)h_; const __bf16 m_ = (__bf16)r1;
    h[c] = h_; m[c] = m_; l[c] = (__bf16)(r1 - (float)m_);
}
// four values (one 16-byte load) -> their three bf16x4 terms
__device__ __forceinline__ void mrdis_split3(const float (&v)[4], bf16x4& h, bf16x4& m, bf16x4& l) {
#pragma unroll
    for (int c = 0; c < 4; ++c) mrdis_split3(v[c], h, m, l, c);
}
// the same for 8 values, converted in pairs (v_cvt_pk_bf16_f32 rounds two values per instruction), packed two bf16 per dword
__device__ __forceinline__ void mrdis_split3x8(const float* v, u32x4& h, u32x4& m, u32x4& l) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const f32x2 a = {v[2 * k], v[2 * k + 1]};
        const bf16x2 hh = __builtin_convertvector(a, bf16x2);
        const f32x2 r1 = a - __builtin_convertvector(hh, f32x2);
        const bf16x2 mm = __builtin_convertvector(r1, bf16x2);
        const f32x2 r2 = r1 - __builtin_convertvector(mm, f32x2);
        const bf16x2 ll = __builtin_convertvector(r2, bf16x2);
        h[k] = __builtin_bit_cast(unsigned, hh); m[k] = __builtin_bit_cast(unsigned, mm); l[k] = __builtin_bit_cast(unsigned, ll);
    }
}
