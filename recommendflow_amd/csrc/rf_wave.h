// rf_wave.h — the MFMA fragment types and the wave-level (64 lanes) reductions shared by the kernels: one definition each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// 4 fp32 -> 4 bf16 (round to nearest even) as one 8-byte store; two of them -> one MFMA operand
__device__ __forceinline__ uint2 bf16_pack4(f32x4 v) {
    bf16x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = (__bf16)v[e];
    return __builtin_bit_cast(uint2, h);
}
__device__ __forceinline__ bf16x8 bf16_join(uint2 lo, uint2 hi) {
    return __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
}

// Sum / max over the four 16-lane rows (lane >> 4) of one column, lanes l, l ^ 16, l ^ 32, l ^ 48: the same value in
// all four, as rows (0 + 1) + (2 + 3)
__device__ __forceinline__ float rows4_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float rows4_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}

// Sum over each 16-lane row of the wave, result in every lane of the row, by DPP (four VALU operations, where a shuffle
// tree is four LDS round trips): quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror. Lane 0's value
// is bit-identical to the xor butterfly (offsets 1, 2, 4, 8): every step adds the same two partial sums, only commuted.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    return v;
}

// Sum / max over the whole wave, the same value in every lane. The two sums add in different orders, so a call site
// keeps the one it has.
// xor butterfly, offsets 32, 16, 8, 4, 2, 1: NOT the same bits as wave_sum_row16_first
__device__ __forceinline__ float wave_sum_butterfly(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max_butterfly(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// the 16-lane rows by DPP first, then rows (0 + 1) + (2 + 3): NOT the same bits as wave_sum_butterfly
__device__ __forceinline__ float wave_sum_row16_first(float v) { return rows4_sum(row16_sum(v)); }
