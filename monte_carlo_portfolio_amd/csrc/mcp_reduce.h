// mcp_reduce.h -- the fixed-order wave and workgroup reductions every kernel file shares (gfx950, 64-lane waves).
//
// A wave reduction is the xor butterfly at distances 32, 16, ..., 1: every lane ends with the same value, formed in the same order on
// every run.  mcp_device.h includes this file, so the path kernels see these functions; a file that needs nothing else includes it alone.
#pragma once
#include <hip/hip_runtime.h>

namespace mcp {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float wave_minf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// fixed-order sum of one double per thread over a 256-thread workgroup -> every thread
__device__ __forceinline__ double block_sum(double v, double* scratch /* [4] LDS */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

}  // namespace mcp
