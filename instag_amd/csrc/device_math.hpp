// Stateless device routines shared by the kernels: the scalar activations, full-wave (64-lane) reductions, the
// 256-thread block sum and the per-Gaussian activations of the "deform + activate" kernels.  Everything is inlined into
// the including file and therefore compiled with THAT file's flags (build.py SOURCES): the same helper contracts into
// fused multiply-adds in glue.hip and does not in pretrain.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace instag {

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float softplus(float x) { return x > 20.f ? x : log1pf(__expf(x)); }
__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }

// ---- full-wave xor butterflies, 32 down to 1: every lane ends up with the result, the additions in a fixed order ----
template <typename T>      // float, double, uint32_t, uint64_t
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

// Sum over a workgroup of 256 threads (four waves), returned to every thread; s_red: 4 floats of LDS.  The waves'
// sums are added as ((s0 + s1) + s2) + s3: callers that promise reproducible bits depend on this association.  There
// is no leading barrier: two uses of one s_red must be separated by a __syncthreads() at the call site, or a fast
// wave overwrites its slot while a slow one still reads the previous sum.
__device__ __forceinline__ float block_sum_256(float v, float* s_red) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_red[wave] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// ---- per-Gaussian activations on register arrays -----------------------------------------------------------------------
// upstream gradient that autograd may not have materialised
__device__ __forceinline__ float load_or_zero(const float* __restrict__ g, size_t i) { return g ? g[i] : 0.f; }

constexpr float QUAT_EPS = 1e-12f;       // torch.nn.functional.normalize's eps

// n2 = |q|^2 comes from the caller, accumulated (n2 += q[k] * q[k]) in the loop that forms q[k]: where the sum sits
// decides whether the compiler fuses or pairs its multiplications, and with that the kernels' result bits.
// y = q / max(|q|, eps) in reciprocal form: one division, four multiplications.  y, dq below: registers or memory
__device__ __forceinline__ void quat_normalize(const float (&q)[4], float n2, float* y) {
  const float inv = 1.0f / fmaxf(sqrtf(n2), QUAT_EPS);
#pragma unroll
  for (int k = 0; k < 4; ++k) y[k] = q[k] * inv;
}

// its backward:  dq = (g - y <g, y>) / |q| for |q| > eps, g / eps below
__device__ __forceinline__ void quat_normalize_backward(const float (&q)[4], float n2, const float (&g)[4],
                                                        float* dq) {
  const float nrm = sqrtf(n2);
  const float inv = 1.0f / fmaxf(nrm, QUAT_EPS);
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) dot += g[k] * q[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) dq[k] = nrm > QUAT_EPS ? (g[k] - q[k] * inv * dot * inv) * inv : g[k] * inv;
}

// d sigmoid(x) = s (1 - s)
__device__ __forceinline__ float sigmoid_backward(float g, float x) {
  const float s = sigmoid(x);
  return g * s * (1.f - s);
}

}  // namespace instag
