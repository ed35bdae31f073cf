// Device helpers of the tri-plane encoder (three identically configured 2-D, C = 1 grids over xy, yz, xz), shared by
// the encoder's own kernels (grid.hip) and the kernels that run the encode in front of a motion field's MLPs (mlp.hip).
// Everything here is inlined into the including file and so takes THAT file's flags (see the note in build.py): the
// two files build with the same ones, and the bilinear expression below must stay one statement in one place.
#pragma once

#include <cstdint>

#include "common.hpp"

namespace instag {
namespace {

struct LevelGeom {
  float scale;
  uint32_t resolution, hashmap_size;
};
__device__ __forceinline__ LevelGeom level_geom(const int32_t* __restrict__ offsets, uint32_t level, float S, uint32_t H) {
  LevelGeom g;
  g.hashmap_size = (uint32_t)(offsets[level + 1] - offsets[level]);
  g.scale = exp2f(level * S) * H - 1.0f;
  g.resolution = (uint32_t)ceilf(g.scale) + 1;
  return g;
}

constexpr uint32_t TP_MAX_L = 16;

struct TriPlaneArgs {
  const float* xyz;           // [N,3]
  const float* tables[3];     // each [T,1]
  const int32_t* offsets;     // [L+1], shared by the three planes
  uint32_t N, L, H;
  float S, bound;
  const float* shift;         // optional [N, shift_stride]: the point is xyz + shift_scale * shift[:, :3]
  uint32_t shift_stride;      //   (the universal field is evaluated at xyz + p_xyz, gaussian_renderer/__init__.py:196-197)
  float shift_scale;
};

__device__ __forceinline__ void tp_point(const TriPlaneArgs& a, uint32_t b, float p[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = a.xyz[3 * b + k];
  if (a.shift) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] += a.shift_scale * a.shift[(size_t)b * a.shift_stride + k];
  }
}

__device__ __forceinline__ void plane_coords(int plane, const float p[3], float x[2]) {
  // xy = (x,y), yz = (y,z), xz = (x,z)   (motion_net.py:244-247)
  x[0] = plane == 1 ? p[1] : p[0];
  x[1] = plane == 0 ? p[1] : p[2];
}

// per-level constants, computed once per workgroup (every level of a tri-plane table is dense: index = x + y*(res+1))
struct TpLevel { float scale; uint32_t stride, offset; };

__device__ __forceinline__ void tp_levels(const TriPlaneArgs& a, TpLevel* s_lv) {
  if (threadIdx.x < a.L) {
    const LevelGeom lg = level_geom(a.offsets, threadIdx.x, a.S, a.H);
    s_lv[threadIdx.x] = TpLevel{lg.scale, lg.resolution + 1, (uint32_t)a.offsets[threadIdx.x]};
  }
}

// table -> LDS with 16-byte loads, several in flight per thread (a scalar loop with a run-time trip count waits
// for every load in turn: ~1 us per iteration from L2)
template <int THREADS, bool ZERO_ACC>
__device__ __forceinline__ void tp_stage_table(float* __restrict__ s_tab, float* __restrict__ s_acc,
                                               const float* __restrict__ tab, uint32_t T) {
  if ((T & 3u) == 0 && (reinterpret_cast<uintptr_t>(tab) & 15) == 0) {
    const float4* src = reinterpret_cast<const float4*>(tab);
    float4* dst = reinterpret_cast<float4*>(s_tab);
    float4* acc = reinterpret_cast<float4*>(s_acc);
    const uint32_t n4 = T >> 2;
#pragma unroll 8
    for (uint32_t i = threadIdx.x; i < n4; i += THREADS) {
      dst[i] = src[i];
      if (ZERO_ACC) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  } else {
#pragma unroll 8
    for (uint32_t i = threadIdx.x; i < T; i += THREADS) {
      s_tab[i] = tab[i];
      if (ZERO_ACC) s_acc[i] = 0.f;
    }
  }
}

// Levels l4 .. l4+3 (clamped to L-1) of one plane at the plane's normalised coordinates (x0, x1): the four values of
// one 16-byte store of the feature row.  `tabp` is the plane's table, in LDS or in place.
__device__ __forceinline__ void tp_group4(const TpLevel* s_lv, const float* __restrict__ tabp, uint32_t L, uint32_t l4,
                                          float x0, float x1, bool oob, float v[4]) {
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t l = min(l4 + q, L - 1);
    const TpLevel lv = s_lv[l];
    const float px = x0 * lv.scale + 0.5f, py = x1 * lv.scale + 0.5f;
    const float flx = floorf(px), fly = floorf(py);
    const float fx = px - flx, fy = py - fly;
    // (out-of-range points read cell 0: the value is discarded)
    const float* tab = tabp + lv.offset + (oob ? 0u : (uint32_t)flx + (uint32_t)fly * lv.stride);
    const float v00 = tab[0], v10 = tab[1], v01 = tab[lv.stride], v11 = tab[lv.stride + 1];
    const float r = ((1.f - fx) * (1.f - fy)) * v00 + (fx * (1.f - fy)) * v10 + ((1.f - fx) * fy) * v01 + (fx * fy) * v11;
    v[q] = oob ? 0.f : r;
  }
}

}  // namespace
}  // namespace instag
