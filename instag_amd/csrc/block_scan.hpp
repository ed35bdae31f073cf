// Prefix sums of one value per thread, for the per-frame scans of the JPEG encoder and decoder (mjpeg.hip,
// jpeg_decode.hip): a wave's by shuffles, a workgroup's through one LDS word per wave.
#pragma once
#include "common.hpp"

namespace instag {

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive scan of the values of one workgroup's thread each; -> the sum of all.  `s_wave`: THREADS / 64 words of LDS,
// free again when the call returns.  Every thread of the workgroup calls it.
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* s_wave, uint32_t& exclusive) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = (uint32_t)wave_inclusive_sum((int)v, lane);
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < THREADS / 64; ++w) {
    const uint32_t t = s_wave[w];
    if (w < wave) before += t;
    all += t;
  }
  __syncthreads();
  exclusive = before + inc - v;
  return all;
}

// v[0..n) -> its exclusive prefix sums, in place, THREADS values at a time with a carried total; -> the sum of all.
// `s_wave` as above.  Every thread of the workgroup calls it; a thread sees the others' writes after a __syncthreads().
template <int THREADS>
__device__ __forceinline__ uint32_t carried_exclusive(uint32_t* v, uint32_t n, uint32_t* s_wave) {
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += THREADS) {
    const uint32_t i = base + threadIdx.x;
    uint32_t ex;
    const uint32_t all = block_exclusive<THREADS>(i < n ? v[i] : 0, s_wave, ex);
    if (i < n) v[i] = carry + ex;
    carry += all;
  }
  return carry;
}

}  // namespace instag
