// cimq_ideal_dev.h -- device helpers the ideal-ADC kernels share (cimq_ideal.hip, cimq_ideal_wide.hip).
#pragma once
#include "cimq_device.h"

namespace cimq {

__device__ inline float ideal_code(float v, float s, float qn, float qp) {
  return rintf(fminf(fmaxf(v / s, qn), qp));  // (a non-finite v is outside the contract)
}

// the block's sum in every thread: a wave butterfly, then the waves' sums added in wave order (red: one float a wave)
__device__ inline float ideal_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float s = red[0];
  for (int i = 1; i < nw; ++i) s += red[i];
  return s;
}

}  // namespace cimq
