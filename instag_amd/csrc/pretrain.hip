// Identity-free pretraining of the universal motion field (pretrain_face.py:34-522): the per-Gaussian operators of its
// step that the adaptation stages do not have.
//
//  pretrain_deform  render_motion(personalized=True, align=False) (gaussian_renderer/__init__.py:200-235) together
//                   with every per-Gaussian term of the pretraining loss (pretrain_face.py, the lines after the
//                   render_motion call):
//                     means3D = xyz + (h_u[:, :3]*1e-2 + h_p[:, :3]*1e-2), scales = softplus(scaling + (h_u + h_p)[:, 8:11]),
//                     rotations = normalize(rotation + (h_u + h_p)[:, 3:7]), opacity = sigmoid(opacity_raw);
//                     1e-5 * mean|.| of the UMF's d_xyz, d_rot, d_scale AFTER the reference's in-place additions of the
//                     PMF's values, of the UMF's d_opa, and of the PMF's four outputs; and the contrast term
//                     sum_j mean_n relu(sum_c d_xyz_j * d_xyz_p) against the other identities' PMF heads h_j.
//                   One forward and one backward launch instead of ~20 elementwise launches each way plus the
//                   regulariser and contrast chains.
//  pretrain_mouth_deform  the mouth stage's counterpart (pretrain_mouth.py:34-358): render_motion_mouth_con(
//                   personalized=True, align=False) (gaussian_renderer/__init__.py:379-406) with the per-Gaussian terms of
//                   pretrain_mouth.py:231-276.  h [N,7], hs [N,1] = the mouth field's heads, h_p [N,7] = the PMF's head:
//                     d_xyz = ((h[:, :3] * (sx, sy, sz)) * sigmoid(hs)) * 2 + h_p[:, :3]*1e-2   (the reference adds the
//                     PMF's displacement IN PLACE, :387, so this combined value is what motion['d_xyz'] holds afterwards),
//                     means3D = xyz + d_xyz, scales = softplus(scaling), rotations = normalize(rotation) (d_rot is never
//                     applied), opacity = sigmoid(opacity_raw);
//                     1e-5 * mean|.| of the combined d_xyz, of h[:, 3:7], of h_p[:, :3]*1e-2 and of h_p[:, 3:7], and the
//                     contrast mean_n relu(sum_c (h_q[c]*1e-2) * (h_p[c]*1e-2)) against ONE partner's PMF head h_q.
//  window_mean      w * x[ch, r0:r1, c0:c1].mean() (the personalised attention map's lips term) appended to a row of
//                   partial sums, so the loss kernel reads all of the step's extra terms as one array.
#include <cstring>

#include "common.hpp"
#include "device_math.hpp"

namespace instag {
namespace {

constexpr int PB = 256;
constexpr int PRETRAIN_MAX_OTHERS = 15;
struct OtherHeads { const float* h[PRETRAIN_MAX_OTHERS]; };

// c_j = sum_c (h_j[c] * 1e-2) * (h_p[c] * 1e-2), evaluated like the reference: both displacements scaled, multiplied,
// the three products added left to right; no contraction into fused multiply-adds
__device__ __forceinline__ float contrast_dot(const float* __restrict__ hj, const float* p) {
  float acc = __fmul_rn(__fmul_rn(hj[0], 1e-2f), __fmul_rn(p[0], 1e-2f));
  acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(hj[1], 1e-2f), __fmul_rn(p[1], 1e-2f)));
  return __fadd_rn(acc, __fmul_rn(__fmul_rn(hj[2], 1e-2f), __fmul_rn(p[2], 1e-2f)));
}

__global__ void __launch_bounds__(PB)
pretrain_deform_forward_kernel(int N, const float* __restrict__ xyz, const float* __restrict__ scaling,
                               const float* __restrict__ rotation, const float* __restrict__ opacity,
                               const float* __restrict__ hu, const float* __restrict__ hp, OtherHeads oh, int n_others,
                               float* __restrict__ means3D, float* __restrict__ scales, float* __restrict__ rots,
                               float* __restrict__ opac, float* __restrict__ reg_partials) {
  __shared__ float s_red[PB / 64];
  const int r = blockIdx.x * PB + threadIdx.x;
  float reg = 0.f;
  if (r < N) {
    float u[11], p[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) { u[k] = hu[(size_t)r * 11 + k]; p[k] = hp[(size_t)r * 11 + k]; }
    float dx[3], ds[3], q[4], n2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dx[k] = __fadd_rn(__fmul_rn(u[k], 1e-2f), __fmul_rn(p[k], 1e-2f));
      ds[k] = u[8 + k] + p[8 + k];
      means3D[3 * r + k] = xyz[3 * r + k] + dx[k];
      scales[3 * r + k] = softplus(scaling[3 * r + k] + ds[k]);
    }
    float dr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dr[k] = u[3 + k] + p[3 + k];
      q[k] = rotation[4 * r + k] + dr[k];
      n2 += q[k] * q[k];
    }
    // this kernel DIVIDES by the clamped norm where quat_normalize multiplies by its reciprocal.  The two round
    // differently: keep the division, or the pretraining step's bits change
    const float den = fmaxf(sqrtf(n2), QUAT_EPS);
#pragma unroll
    for (int k = 0; k < 4; ++k) rots[4 * r + k] = q[k] / den;
    opac[r] = sigmoid(opacity[r]);
    if (reg_partials) {
      const float w3 = 1e-5f / (3.f * N), w4 = 1e-5f / (4.f * N), w1 = 1e-5f / (float)N;
      const float umf = w3 * (fabsf(dx[0]) + fabsf(dx[1]) + fabsf(dx[2])) + w4 * (fabsf(dr[0]) + fabsf(dr[1]) + fabsf(dr[2]) + fabsf(dr[3]))
          + w1 * fabsf(u[7]) + w3 * (fabsf(ds[0]) + fabsf(ds[1]) + fabsf(ds[2]));
      const float pmf = w3 * (fabsf(p[0] * 1e-2f) + fabsf(p[1] * 1e-2f) + fabsf(p[2] * 1e-2f))
          + w4 * (fabsf(p[3]) + fabsf(p[4]) + fabsf(p[5]) + fabsf(p[6])) + w1 * fabsf(p[7])
          + w3 * (fabsf(p[8]) + fabsf(p[9]) + fabsf(p[10]));
      float con = 0.f;
      for (int j = 0; j < n_others; ++j) con += fmaxf(contrast_dot(oh.h[j] + (size_t)r * 11, p), 0.f);
      reg = umf + pmf + con / (float)N;
    }
  }
  if (reg_partials) {
    reg = block_sum_256(reg, s_red);
    if (threadIdx.x == 0) reg_partials[blockIdx.x] = reg;
  }
}

__global__ void __launch_bounds__(PB)
pretrain_deform_backward_kernel(int N, const float* __restrict__ scaling, const float* __restrict__ rotation,
                                const float* __restrict__ opacity, const float* __restrict__ hu,
                                const float* __restrict__ hp, OtherHeads oh, int n_others,
                                const float* __restrict__ g_means, const float* __restrict__ g_scales,
                                const float* __restrict__ g_rots, const float* __restrict__ g_opac,
                                const float* __restrict__ g_reg, float* __restrict__ d_xyz,
                                float* __restrict__ d_scaling, float* __restrict__ d_rotation,
                                float* __restrict__ d_opacity, float* __restrict__ d_hu, float* __restrict__ d_hp) {
  const int r = blockIdx.x * PB + threadIdx.x;
  if (r >= N) return;
  float u[11], p[11], du[11], dp[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    u[k] = hu[(size_t)r * 11 + k]; p[k] = hp[(size_t)r * 11 + k];
    du[k] = 0.f; dp[k] = 0.f;
  }
  float dx[3], ds[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    dx[k] = __fadd_rn(__fmul_rn(u[k], 1e-2f), __fmul_rn(p[k], 1e-2f));
    ds[k] = u[8 + k] + p[8 + k];
    const float gm = load_or_zero(g_means, 3 * r + k);
    d_xyz[3 * r + k] = gm;
    du[k] = gm * 1e-2f;
    dp[k] = gm * 1e-2f;
    const float sg = load_or_zero(g_scales, 3 * r + k) * sigmoid(scaling[3 * r + k] + ds[k]);      // d softplus = sigmoid
    d_scaling[3 * r + k] = sg;
    du[8 + k] = sg;
    dp[8 + k] = sg;
  }
  float q[4], dr[4], gr[4], n2 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    dr[k] = u[3 + k] + p[3 + k];
    q[k] = rotation[4 * r + k] + dr[k];
    n2 += q[k] * q[k];
    gr[k] = load_or_zero(g_rots, 4 * r + k);
  }
  quat_normalize_backward(q, n2, gr, du + 3);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    d_rotation[4 * r + k] = du[3 + k];
    dp[3 + k] = du[3 + k];
  }
  d_opacity[r] = sigmoid_backward(load_or_zero(g_opac, r), opacity[r]);
  if (g_reg) {
    const float go = g_reg[0];
    const float w3 = go * 1e-5f / (3.f * N), w4 = go * 1e-5f / (4.f * N), w1 = go * 1e-5f / (float)N;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      // UMF d_xyz (= the sum of both fields' displacements): |.| passes sgn * 1e-2 to both heads
      const float gx = w3 * sgn(dx[k]) * 1e-2f;
      du[k] += gx;
      dp[k] += gx + w3 * sgn(p[k]) * 1e-2f;
      const float gsc = w3 * sgn(ds[k]);
      du[8 + k] += gsc;
      dp[8 + k] += gsc + w3 * sgn(p[8 + k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float grt = w4 * sgn(dr[k]);
      du[3 + k] += grt;
      dp[3 + k] += grt + w4 * sgn(p[3 + k]);
    }
    du[7] += w1 * sgn(u[7]);
    dp[7] += w1 * sgn(p[7]);
    // contrast: the reference zeroes the entries < 0 in place, so the gradient passes where c_j >= 0
    const float wc = go / (float)N;
    for (int j = 0; j < n_others; ++j) {
      const float* hj = oh.h[j] + (size_t)r * 11;
      if (contrast_dot(hj, p) >= 0.f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dp[k] += wc * (hj[k] * 1e-2f) * 1e-2f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    d_hu[(size_t)r * 11 + k] = du[k];
    d_hp[(size_t)r * 11 + k] = dp[k];
  }
}

// ---- mouth stage --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PB)
pretrain_mouth_deform_forward_kernel(int N, const float* __restrict__ xyz, const float* __restrict__ scaling,
                                     const float* __restrict__ rotation, const float* __restrict__ opacity,
                                     const float* __restrict__ h /*[N,7]*/, const float* __restrict__ hs /*[N,1]*/,
                                     const float* __restrict__ hp /*[N,7]*/, const float* __restrict__ hq /*[N,7] or NULL*/,
                                     float sx, float sy, float sz, float* __restrict__ means3D,
                                     float* __restrict__ scales, float* __restrict__ rots, float* __restrict__ opac,
                                     float* __restrict__ reg_partials) {
  __shared__ float s_red[PB / 64];
  const int r = blockIdx.x * PB + threadIdx.x;
  float reg = 0.f;
  if (r < N) {
    float u[7], p[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { u[k] = h[(size_t)r * 7 + k]; p[k] = hp[(size_t)r * 7 + k]; }
    const float sg = sigmoid(hs[r]);
    const float xs[3] = {sx, sy, sz};
    float dx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dx[k] = ((u[k] * xs[k]) * sg) * 2.0f + p[k] * 1e-2f;          // (no contraction: -ffp-contract=off)
      means3D[3 * r + k] = xyz[3 * r + k] + dx[k];
      scales[3 * r + k] = softplus(scaling[3 * r + k]);
    }
    float q[4], n2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k] = rotation[4 * r + k]; n2 += q[k] * q[k]; }
    quat_normalize(q, n2, rots + 4 * r);
    opac[r] = sigmoid(opacity[r]);
    if (reg_partials) {
      const float w3 = 1e-5f / (3.f * N), w4 = 1e-5f / (4.f * N);
      const float umf = w3 * (fabsf(dx[0]) + fabsf(dx[1]) + fabsf(dx[2]))
          + w4 * (fabsf(u[3]) + fabsf(u[4]) + fabsf(u[5]) + fabsf(u[6]));
      const float pmf = w3 * (fabsf(p[0] * 1e-2f) + fabsf(p[1] * 1e-2f) + fabsf(p[2] * 1e-2f))
          + w4 * (fabsf(p[3]) + fabsf(p[4]) + fabsf(p[5]) + fabsf(p[6]));
      const float con = hq ? fmaxf(contrast_dot(hq + (size_t)r * 7, p), 0.f) : 0.f;
      reg = umf + pmf + con / (float)N;
    }
  }
  if (reg_partials) {
    reg = block_sum_256(reg, s_red);
    if (threadIdx.x == 0) reg_partials[blockIdx.x] = reg;
  }
}

__global__ void __launch_bounds__(PB)
pretrain_mouth_deform_backward_kernel(int N, const float* __restrict__ scaling, const float* __restrict__ rotation,
                                      const float* __restrict__ opacity, const float* __restrict__ h,
                                      const float* __restrict__ hs, const float* __restrict__ hp,
                                      const float* __restrict__ hq, float sx, float sy, float sz,
                                      const float* __restrict__ g_means, const float* __restrict__ g_scales,
                                      const float* __restrict__ g_rots, const float* __restrict__ g_opac,
                                      const float* __restrict__ g_reg, float* __restrict__ d_xyz,
                                      float* __restrict__ d_scaling, float* __restrict__ d_rotation,
                                      float* __restrict__ d_opacity, float* __restrict__ d_h /*[N,7]*/,
                                      float* __restrict__ d_hs /*[N,1]*/, float* __restrict__ d_hp /*[N,7]*/) {
  const int r = blockIdx.x * PB + threadIdx.x;
  if (r >= N) return;
  float u[7], p[7], du[7], dp[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    u[k] = h[(size_t)r * 7 + k]; p[k] = hp[(size_t)r * 7 + k];
    du[k] = 0.f; dp[k] = 0.f;
  }
  const float sg = sigmoid(hs[r]);
  const float xs[3] = {sx, sy, sz};
  const bool with_reg = g_reg != nullptr;
  const float go = with_reg ? g_reg[0] : 0.f;
  const float w3 = go * 1e-5f / (3.f * N), w4 = go * 1e-5f / (4.f * N);
  float dgate = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float gm = load_or_zero(g_means, 3 * r + k);
    d_xyz[3 * r + k] = gm;
    // the gradient of the COMBINED displacement: the render's, and |.| of the first regulariser, into both fields
    float G = gm;
    if (with_reg) {
      const float dxk = ((u[k] * xs[k]) * sg) * 2.0f + p[k] * 1e-2f;
      G += w3 * sgn(dxk);
    }
    du[k] = G * 2.0f * sg * xs[k];
    dgate += G * 2.0f * (u[k] * xs[k]);
    dp[k] = G * 1e-2f;
    if (with_reg) dp[k] += w3 * sgn(p[k] * 1e-2f) * 1e-2f;
    d_scaling[3 * r + k] = load_or_zero(g_scales, 3 * r + k) * sigmoid(scaling[3 * r + k]);   // d softplus = sigmoid
  }
  if (with_reg) {
#pragma unroll
    for (int k = 3; k < 7; ++k) {          // d_rot is regularised but never applied
      du[k] = w4 * sgn(u[k]);
      dp[k] = w4 * sgn(p[k]);
    }
    if (hq) {
      // contrast: the reference zeroes the entries < 0 in place, so the gradient passes where c >= 0
      const float* q7 = hq + (size_t)r * 7;
      if (contrast_dot(q7, p) >= 0.f) {
        const float wc = go / (float)N;
#pragma unroll
        for (int k = 0; k < 3; ++k) dp[k] += wc * (q7[k] * 1e-2f) * 1e-2f;
      }
    }
  }
  float q[4], gr[4], n2 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q[k] = rotation[4 * r + k];
    n2 += q[k] * q[k];
    gr[k] = load_or_zero(g_rots, 4 * r + k);
  }
  quat_normalize_backward(q, n2, gr, d_rotation + 4 * r);
  d_opacity[r] = sigmoid_backward(load_or_zero(g_opac, r), opacity[r]);
  d_hs[r] = dgate * sg * (1.f - sg);
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    d_h[(size_t)r * 7 + k] = du[k];
    d_hp[(size_t)r * 7 + k] = dp[k];
  }
}

// One workgroup: copies the n_prev partial sums in front and appends w * mean of the window as the last entry.
__global__ void __launch_bounds__(PB)
window_mean_forward_kernel(const float* __restrict__ x, int H, int W, int ch, const int32_t* __restrict__ rect,
                           float w, const float* __restrict__ prev, int n_prev, float* __restrict__ out) {
  __shared__ float s[PB];
  for (int i = threadIdx.x; i < n_prev; i += PB) out[i] = prev[i];
  const int r0 = min(max(rect[0], 0), H), r1 = min(max(rect[1], r0), H);
  const int c0 = min(max(rect[2], 0), W), c1 = min(max(rect[3], c0), W);
  const int wc = c1 - c0, cnt = (r1 - r0) * wc;
  float acc = 0.f;
  for (int i = threadIdx.x; i < cnt; i += PB) acc += x[((size_t)ch * H + r0 + i / wc) * W + c0 + i % wc];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int o = PB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[n_prev] = w * (s[0] / (float)cnt);
}

__global__ void __launch_bounds__(PB)
window_mean_backward_kernel(int C, int H, int W, int ch, const int32_t* __restrict__ rect, float w,
                            const float* __restrict__ g, float* __restrict__ dx) {
  const int i = blockIdx.x * PB + threadIdx.x;
  if (i >= C * H * W) return;
  const int c = i / (H * W), rr = (i / W) % H, cc = i % W;
  const int r0 = min(max(rect[0], 0), H), r1 = min(max(rect[1], r0), H);
  const int c0 = min(max(rect[2], 0), W), c1 = min(max(rect[3], c0), W);
  const int cnt = (r1 - r0) * (c1 - c0);
  const bool in = c == ch && rr >= r0 && rr < r1 && cc >= c0 && cc < c1;
  dx[i] = in ? (g[0] * w) / (float)cnt : 0.f;
}

int copy_heads(OtherHeads& oh, const void* host_heads, int n_others) {
  memset(&oh, 0, sizeof(oh));
  if (n_others > 0) memcpy(oh.h, host_heads, (size_t)n_others * sizeof(const float*));
  for (int j = 0; j < n_others; ++j)
    if (!oh.h[j]) return INSTAG_E_ARG;
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

int instag_pretrain_deform_max_others(void) { return PRETRAIN_MAX_OTHERS; }

int instag_pretrain_deform_num_partials(int32_t N) { return (N + PB - 1) / PB; }

int instag_pretrain_deform_forward(const float* xyz, const float* scaling, const float* rotation, const float* opacity,
                                   const float* h_u, const float* h_p, const void* host_heads, int32_t n_others,
                                   float* means3D, float* scales, float* rotations, float* opac, float* reg_partials,
                                   int32_t N, instag_stream_t stream) {
  INSTAG_REQUIRE(xyz && scaling && rotation && opacity && h_u && h_p && means3D && scales && rotations && opac,
                 "pretrain_deform_forward: NULL tensor");
  INSTAG_REQUIRE(n_others >= 0 && n_others <= PRETRAIN_MAX_OTHERS && (n_others == 0 || host_heads),
                 "pretrain_deform_forward: 0 <= n_others <= instag_pretrain_deform_max_others()");
  OtherHeads oh;
  INSTAG_REQUIRE(copy_heads(oh, host_heads, n_others) == INSTAG_OK, "pretrain_deform_forward: NULL head");
  if (N <= 0) return INSTAG_OK;
  pretrain_deform_forward_kernel<<<(N + PB - 1) / PB, PB, 0, (hipStream_t)stream>>>(
      N, xyz, scaling, rotation, opacity, h_u, h_p, oh, n_others, means3D, scales, rotations, opac, reg_partials);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_pretrain_deform_backward(const float* scaling, const float* rotation, const float* opacity,
                                    const float* h_u, const float* h_p, const void* host_heads, int32_t n_others,
                                    const float* g_means, const float* g_scales, const float* g_rots,
                                    const float* g_opac, const float* g_reg, float* d_xyz, float* d_scaling,
                                    float* d_rotation, float* d_opacity, float* d_hu, float* d_hp, int32_t N,
                                    instag_stream_t stream) {
  INSTAG_REQUIRE(scaling && rotation && opacity && h_u && h_p && d_xyz && d_scaling && d_rotation && d_opacity &&
                 d_hu && d_hp, "pretrain_deform_backward: NULL tensor");
  INSTAG_REQUIRE(n_others >= 0 && n_others <= PRETRAIN_MAX_OTHERS && (n_others == 0 || host_heads),
                 "pretrain_deform_backward: 0 <= n_others <= instag_pretrain_deform_max_others()");
  OtherHeads oh;
  INSTAG_REQUIRE(copy_heads(oh, host_heads, n_others) == INSTAG_OK, "pretrain_deform_backward: NULL head");
  if (N <= 0) return INSTAG_OK;
  pretrain_deform_backward_kernel<<<(N + PB - 1) / PB, PB, 0, (hipStream_t)stream>>>(
      N, scaling, rotation, opacity, h_u, h_p, oh, n_others, g_means, g_scales, g_rots, g_opac, g_reg, d_xyz,
      d_scaling, d_rotation, d_opacity, d_hu, d_hp);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_pretrain_mouth_deform_num_partials(int32_t N) { return N > 0 ? (N + PB - 1) / PB : 0; }

int instag_pretrain_mouth_deform_forward(const float* xyz, const float* scaling, const float* rotation,
                                         const float* opacity, const float* h, const float* hs, const float* h_p,
                                         const float* h_q, float sx, float sy, float sz, float* means3D, float* scales,
                                         float* rotations, float* opac, float* reg_partials, int32_t N,
                                         instag_stream_t stream) {
  INSTAG_REQUIRE(xyz && scaling && rotation && opacity && h && hs && h_p && means3D && scales && rotations && opac,
                 "pretrain_mouth_deform_forward: NULL tensor");
  INSTAG_REQUIRE(N >= 0, "pretrain_mouth_deform_forward: N >= 0");
  if (N == 0) return INSTAG_OK;
  pretrain_mouth_deform_forward_kernel<<<(N + PB - 1) / PB, PB, 0, (hipStream_t)stream>>>(
      N, xyz, scaling, rotation, opacity, h, hs, h_p, h_q, sx, sy, sz, means3D, scales, rotations, opac, reg_partials);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_pretrain_mouth_deform_backward(const float* scaling, const float* rotation, const float* opacity,
                                          const float* h, const float* hs, const float* h_p, const float* h_q, float sx,
                                          float sy, float sz, const float* g_means, const float* g_scales,
                                          const float* g_rots, const float* g_opac, const float* g_reg, float* d_xyz,
                                          float* d_scaling, float* d_rotation, float* d_opacity, float* d_h, float* d_hs,
                                          float* d_hp, int32_t N, instag_stream_t stream) {
  INSTAG_REQUIRE(scaling && rotation && opacity && h && hs && h_p && d_xyz && d_scaling && d_rotation && d_opacity &&
                 d_h && d_hs && d_hp, "pretrain_mouth_deform_backward: NULL tensor");
  INSTAG_REQUIRE(N >= 0, "pretrain_mouth_deform_backward: N >= 0");
  if (N == 0) return INSTAG_OK;
  pretrain_mouth_deform_backward_kernel<<<(N + PB - 1) / PB, PB, 0, (hipStream_t)stream>>>(
      N, scaling, rotation, opacity, h, hs, h_p, h_q, sx, sy, sz, g_means, g_scales, g_rots, g_opac, g_reg, d_xyz,
      d_scaling, d_rotation, d_opacity, d_h, d_hs, d_hp);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_window_mean_forward(const float* x, int32_t C, int32_t H, int32_t W, int32_t ch, const int32_t* rect,
                               float w, const float* prev, int32_t n_prev, float* out, instag_stream_t stream) {
  INSTAG_REQUIRE(x && rect && out && (n_prev == 0 || prev), "window_mean_forward: NULL tensor");
  INSTAG_REQUIRE(C >= 1 && H >= 1 && W >= 1 && ch >= 0 && ch < C && n_prev >= 0, "window_mean: bad shape");
  window_mean_forward_kernel<<<1, PB, 0, (hipStream_t)stream>>>(x, H, W, ch, rect, w, prev, n_prev, out);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_window_mean_backward(int32_t C, int32_t H, int32_t W, int32_t ch, const int32_t* rect, float w,
                                const float* g, float* dx, instag_stream_t stream) {
  INSTAG_REQUIRE(rect && g && dx, "window_mean_backward: NULL tensor");
  INSTAG_REQUIRE(C >= 1 && H >= 1 && W >= 1 && ch >= 0 && ch < C, "window_mean: bad shape");
  INSTAG_REQUIRE((long long)C * H * W <= 0x7fffffffll, "window_mean: tensor too large");
  const int n = C * H * W;
  window_mean_backward_kernel<<<(n + PB - 1) / PB, PB, 0, (hipStream_t)stream>>>(C, H, W, ch, rect, w, g, dx);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
