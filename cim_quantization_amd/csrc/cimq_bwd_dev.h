// cimq_bwd_dev.h -- device helpers shared by the state-word backward kernels (cimq_v7.hip, cimq_fused.hip,
// cimq_c1.hip, cimq_gx5.hip, cimq_gw5.hip, cimq_r6.hip): pass-bit masks, uniform-register copies, DPP lane
// shifts, ctx slice words.
#pragma once
#include "cimq_device.h"

#ifndef CIMQ_FOLD_XB
#define CIMQ_FOLD_XB 1  // the grad_x folds' elements per thread and round (cimq_v7 / cimq_fused)
#endif

namespace cimq {

// pass-bit masks of the state word: all j of slice k / all k of slice j
__host__ __device__ constexpr uint32_t pass_mask_k(int k, int nba) {
  uint32_t m = 0;
  for (int j = 0; j < nba; ++j) m |= 1u << (3 * (k * nba + j));
  return m;
}
__host__ __device__ constexpr uint32_t pass_mask_j(int j, int nbw, int nba) {
  uint32_t m = 0;
  for (int k = 0; k < nbw; ++k) m |= 1u << (3 * (k * nba + j));
  return m;
}

// The state words a v7 slice-pair shape reads (host: StateFmt, v7_plan), named per shape -- the pair count alone
// does not tell the 16 pairs of w4a4 from plane words:
//   V7W_32      one uint32, bits 3*kj + {0 pass, 1 code != 0, 2 code < 0}, kj = k*nba + j            (w2a2, w3a3)
//   V7W_32X2    a uint2 of two such words: .x weight slices 0-1 (kj 0..7), .y slices 2-3 (kj - 8)   (w4a4)
//   V7W_PLANES  three 64-bit planes, bit kj each                                                     (w8a8)
enum V7Words { V7W_32, V7W_32X2, V7W_PLANES };
template <int NBW, int NBA> struct V7WordsOf;
template <> struct V7WordsOf<2, 2> { static constexpr V7Words fmt = V7W_32; };
template <> struct V7WordsOf<3, 3> { static constexpr V7Words fmt = V7W_32; };
template <> struct V7WordsOf<4, 4> { static constexpr V7Words fmt = V7W_32X2; };
template <> struct V7WordsOf<8, 8> { static constexpr V7Words fmt = V7W_PLANES; };

// uniform (scalar-register) copies of values every lane computed identically
__device__ inline float sgpr_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ inline uint64_t sgpr_u64(uint64_t v) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}

// lane l <- lane l+1 / l-1 of the same 16-lane row (0 past the row's end)
__device__ inline float dpp_from_next(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x101, 0xF, 0xF, true));
}
__device__ inline float dpp_from_prev(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true));
}

// ctx slice bytes of one input element: NBP = 4 (uint32) or 8 (uint2) bytes, slice j in byte j
__device__ inline uint32_t xbyte(uint32_t w, int j) { return (w >> (8 * j)) & 0xFFu; }
__device__ inline uint32_t xbyte(uint2 w, int j) { return (j < 4 ? (w.x >> (8 * j)) : (w.y >> (8 * (j - 4)))) & 0xFFu; }
template <typename XW>
__device__ inline XW xzero();
template <>
__device__ inline uint32_t xzero<uint32_t>() { return 0u; }
template <>
__device__ inline uint2 xzero<uint2>() { return make_uint2(0u, 0u); }
// n consecutive elements from a 16-B aligned source by 16-B loads
template <int N>
__device__ inline void xload(const uint32_t* src, uint32_t* d) {
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const uint4 t = reinterpret_cast<const uint4*>(src)[q];
    d[4 * q] = t.x; d[4 * q + 1] = t.y; d[4 * q + 2] = t.z; d[4 * q + 3] = t.w;
  }
}
template <int N>
__device__ inline void xload(const uint2* src, uint2* d) {
#pragma unroll
  for (int q = 0; q < N / 2; ++q) {
    const uint4 t = reinterpret_cast<const uint4*>(src)[q];
    d[2 * q] = make_uint2(t.x, t.y); d[2 * q + 1] = make_uint2(t.z, t.w);
  }
}

}  // namespace cimq
