// Per-frame conditioning codes of a motion network as ONE workgroup per pass:
//   enc_a = AudioAttNet(AudioNet(a))            scene/motion_net.py:29-64, :67-99 (used at :283-289 / :672-677)
//   enc_e = cat(exp_encode_net(e[:-1]), e[-1:]) scene/motion_net.py:152-173, :297-299 / :684-686
// The reference runs this as ~11 cuDNN conv1d / GEMM launches plus their activations (and three times that in
// backward) on an 8-window batch: launch-latency bound.  Here every activation lives in LDS, weights are staged
// through LDS per layer group, and the backward pass produces every parameter gradient without atomics (deterministic).
//
// Layer stack (B = 8 windows, W = 16 samples, D = dim_in, M = mid, A = dim_aud, LeakyReLU slope 0.02):
//   conv k3 s2 p1: D->M (16->8), M->M (8->4), M->64 (4->2), 64->64 (2->1); fc 64->64 (leaky), fc 64->A
//   attention (B=1, channels = A features, length = 8 windows): conv k3 s1 p1 A->16->8->4->2->1 (leaky each),
//   linear 8->8, softmax, enc_a = sum_t y[t] * feat[t]
//   expression: relu(W1[16x5] e[:5]), W2[5x16], enc_e = (.., e[5])
//
// Three kernel families share that tail: the stock AudioNet on windows of 16 samples (frame_code_*), AudioNet_ave
// (frame_code_ave_*, below) and the wide AudioNet of a 'hubert' head on windows of two samples (frame_code_wide_*, last).
// Their front parts are different algorithms and stay apart; everything behind the feature block [8][A] exists once:
//   att_layer / att_layout / stage_attention  the attention layer table, its LDS segments and their staging
//   attention_forward<T, SPLIT_CONV>          AudioAttNet + expression MLP forward (all three forward kernels)
//   attention_backward                        their backward (both backward kernels)
//   last_to_arrive                            the hand-off of a split forward to its last workgroup
#include "common.hpp"
#include "instag_frame_code_wide.h"

namespace instag {
namespace {

constexpr int FT = 1024;         // threads of the single workgroup
constexpr int NB = 8;             // audio windows per frame (= attention sequence length)
constexpr int WIN = 16;
constexpr float SLOPE = 0.02f;
constexpr int NPARAM = 26;

struct FrameDims { int D, M, A, has_exp; };

// float offsets of every activation inside one LDS / saved block
struct FrameLayout {
  int x0, a1, a2, a3, a4, f1, f2, xt, c1, c2, c3, c4, c5, z, y, eh, end;
};

__host__ __device__ inline FrameLayout frame_layout(int D, int M, int A) {
  FrameLayout L;
  int o = 0;
  L.x0 = o; o += NB * D * WIN;
  L.a1 = o; o += NB * M * 8;
  L.a2 = o; o += NB * M * 4;
  L.a3 = o; o += NB * 64 * 2;
  L.a4 = o; o += NB * 64;
  L.f1 = o; o += NB * 64;
  L.f2 = o; o += NB * A;
  L.xt = o; o += A * NB;
  L.c1 = o; o += 16 * NB;
  L.c2 = o; o += 8 * NB;
  L.c3 = o; o += 4 * NB;
  L.c4 = o; o += 2 * NB;
  L.c5 = o; o += NB;
  L.z = o; o += NB;
  L.y = o; o += NB;
  L.eh = o; o += 16;
  L.end = o;
  return L;
}

struct ParamPtrs { const float* p[NPARAM]; };
struct GradPtrs { float* p[NPARAM]; };

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : SLOPE * v; }
__device__ __forceinline__ float dleaky(float post) { return post > 0.f ? 1.f : SLOPE; }

// Weights are staged into LDS one layer group at a time (coalesced 16-byte loads, all issued before the first
// wait): a MAC loop that reads its weight from global memory pays one L2 round trip per iteration.
// Groups: 0 conv1, 1 conv2, 2 conv3, 3 conv4, 4 fc1+fc2, 5 attention convs + linear + expression MLP.
// The attention stage's layers: five k3 s1 p1 convolutions A -> 16 -> 8 -> 4 -> 2 -> 1 over the eight windows and the
// 8 x 8 linear layer (K = 1).  The only copy of this table: the segment offsets, the staging and both passes read it.
constexpr int NATT = 6;
struct AttLayer { int cin, cout, K; };
__host__ __device__ inline AttLayer att_layer(int i, int A) {
  const AttLayer t[NATT] = {{A, 16, 3}, {16, 8, 3}, {8, 4, 3}, {4, 2, 3}, {2, 1, 3}, {NB, NB, 1}};
  return t[i];
}

// offsets of the group-5 segments inside the staging buffer (segments padded to 4 floats)
struct AttW { int w[NATT], b[NATT], e1, e2, end; };
__host__ __device__ inline AttW att_layout(int A) {
  AttW o;
  int p = 0;
  for (int i = 0; i < NATT; ++i) {
    const AttLayer l = att_layer(i, A);
    o.w[i] = p; p += (l.cout * l.cin * l.K + 3) & ~3;
    o.b[i] = p; p += (l.cout + 3) & ~3;
  }
  o.e1 = p; p += 80;
  o.e2 = p; p += 80;
  o.end = p;
  return o;
}
__host__ __device__ inline int att_floats(int A) { return att_layout(A).end + 4; }   // 48 A + 784: four spare floats
__host__ __device__ inline int weight_stage_floats(int D, int M, int A) {
  int m = M * D * 3 + M;
  m = max(m, M * M * 3 + M);
  m = max(m, 64 * M * 3 + 64);
  m = max(m, 64 * 64 * 3 + 64);
  m = max(m, 64 * 64 + 64 + A * 64 + A);
  m = max(m, att_floats(A));
  return (m + 3) & ~3;
}

// T = threads of the workgroup
template <int T>
__device__ __forceinline__ void stage(float* dst, const float* __restrict__ src, int n) {
  if (src == nullptr) return;
  if ((n & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll 4
    for (int i = threadIdx.x; i < n / 4; i += T) d4[i] = s4[i];
  } else {
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += T) dst[i] = src[i];
  }
}

// Group 5 into dst: p = the stage's 14 parameters (six weight, bias pairs, then the two expression weights).
// weights_only: the backward kernels need the six weights and e2 and load nothing else.
template <int T>
__device__ __forceinline__ void stage_attention(float* dst, const AttW& aw, const float* const* p, int A, bool has_exp,
                                                bool weights_only) {
#pragma unroll
  for (int i = 0; i < NATT; ++i) {
    const AttLayer l = att_layer(i, A);
    stage<T>(dst + aw.w[i], p[2 * i], l.cout * l.cin * l.K);
    if (!weights_only) stage<T>(dst + aw.b[i], p[2 * i + 1], l.cout);
  }
  if (has_exp) {
    if (!weights_only) stage<T>(dst + aw.e1, p[12], 80);
    stage<T>(dst + aw.e2, p[13], 80);
  }
}

// y[b][co][l] = act(bias[co] + sum_{ci,k} w[co][ci][k] * x[b][ci][STRIDE*l + k - pad]); K = 1 is a linear layer.
// x, w, bias live in LDS; the ci loop is unrolled so that several LDS reads are in flight per thread (one
// workgroup on one CU: the passes are latency-, not throughput-bound).
template <int K, int STRIDE>
__device__ __forceinline__ void conv_forward(const float* x, const float* w, const float* bias, float* y, int B, int cin,
                                             int cout, int lin, int lout, bool act) {
  constexpr int PAD = K == 3 ? 1 : 0;
  const int total = B * cout * lout;
  for (int o = threadIdx.x; o < total; o += FT) {
    const int l = o % lout, co = (o / lout) % cout, b = o / (lout * cout);
    const float* wr = w + co * cin * K;
    const float* xb = x + b * cin * lin;
    const int p0 = STRIDE * l - PAD;
    bool ok[K];
#pragma unroll
    for (int k = 0; k < K; ++k) ok[k] = p0 + k >= 0 && p0 + k < lin;
    float acc0 = bias ? bias[co] : 0.f, acc1 = 0.f;
#pragma unroll 4
    for (int ci = 0; ci < cin; ++ci) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float xv = ok[k] ? xb[ci * lin + p0 + k] : 0.f;
        if (ci & 1) acc1 += wr[ci * K + k] * xv; else acc0 += wr[ci * K + k] * xv;
      }
    }
    const float acc = acc0 + acc1;
    y[o] = act ? leaky(acc) : acc;
  }
}

// g_out holds d(pre-activation) of the layer's output.  Writes dW, dbias to global (each unless nullptr) and, when g_in != nullptr,
// d(pre-activation) of the layer's input (x is a leaky output when in_act) or the plain input gradient.
template <int K, int STRIDE>
__device__ __forceinline__ void conv_backward(const float* x, const float* g_out, const float* w, float* __restrict__ dW,
                                              float* __restrict__ dbias, float* g_in, int B, int cin, int cout, int lin,
                                              int lout, bool in_act) {
  constexpr int PAD = K == 3 ? 1 : 0;
  const int nW = dW ? cout * cin * K : 0;
  const int nB = dbias ? cout : 0;
  const int nI = g_in ? B * cin * lin : 0;
  for (int idx = threadIdx.x; idx < nW + nB + nI; idx += FT) {
    if (idx < nW) {
      const int k = idx % K, ci = (idx / K) % cin, co = idx / (K * cin);
      float acc = 0.f;
      for (int b = 0; b < B; ++b) {
        const float* gb = g_out + (b * cout + co) * lout;
        const float* xb = x + (b * cin + ci) * lin;
#pragma unroll 4
        for (int l = 0; l < lout; ++l) {
          const int p = STRIDE * l + k - PAD;
          const float xv = (p >= 0 && p < lin) ? xb[p] : 0.f;
          acc += gb[l] * xv;
        }
      }
      dW[idx] = acc;
    } else if (idx < nW + nB) {
      const int co = idx - nW;
      float acc = 0.f;
      for (int b = 0; b < B; ++b)
#pragma unroll 4
        for (int l = 0; l < lout; ++l) acc += g_out[(b * cout + co) * lout + l];
      dbias[co] = acc;
    } else {
      const int i = idx - nW - nB;
      const int p = i % lin, ci = (i / lin) % cin, b = i / (lin * cin);
      float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int q = p + PAD - k;               // = STRIDE * l
        const int l = q / STRIDE;
        const bool ok = q >= 0 && (q % STRIDE) == 0 && l < lout;
        if (ok) {
          const float* gb = g_out + b * cout * lout + l;
          const float* wk = w + ci * K + k;
#pragma unroll 4
          for (int co = 0; co < cout; ++co) {
            const float t = wk[co * cin * K] * gb[co * lout];
            if (co & 1) acc1 += t; else acc0 += t;
          }
        }
      }
      float acc = acc0 + acc1;
      if (in_act) acc *= dleaky(x[i]);
      g_in[i] = acc;
    }
  }
}

constexpr int FW = 256;           // threads per workgroup of the split forward pass
__device__ __forceinline__ int co_of(int o, int lout) { return o / lout; }

// conv_forward for ONE window and FW threads: one output per group of `tpo` lanes (a power of two <= 64), each lane sums a slice of the input channels
template <int K, int STRIDE>
__device__ __forceinline__ void conv_forward_split(const float* x, const float* w, const float* bias, float* y, int cin,
                                                   int cout, int lin, int lout, bool act) {
  constexpr int PAD = K == 3 ? 1 : 0;
  const int total = cout * lout;
  int tpo = 1;
  while (tpo * 2 * total <= FW && tpo * 2 <= cin && tpo < 64) tpo *= 2;
  for (int base = 0; base < total; base += FW / tpo) {
    const int o = base + (int)threadIdx.x / tpo, part = (int)threadIdx.x % tpo;
    float acc = 0.f;
    if (o < total) {
      const int l = o % lout, co = o / lout;
      const float* wr = w + co * cin * K;
      const int p0 = STRIDE * l - PAD;
#pragma unroll 4
      for (int ci = part; ci < cin; ci += tpo) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int p = p0 + k;
          const float xv = (p >= 0 && p < lin) ? x[ci * lin + p] : 0.f;
          acc += wr[ci * K + k] * xv;
        }
      }
    }
    for (int m = tpo >> 1; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
    if (o < total && part == 0) {
      acc += bias ? bias[co_of(o, lout)] : 0.f;
      y[o] = act ? leaky(acc) : acc;
    }
  }
}

// ---- the stages that every kernel family shares ------------------------------------------------------------------
// Hand-off of a forward pass that is split over n workgroups: stores drained by every wave, workgroup barrier,
// agent-scope release, then the arrival counter.  True in the workgroup that draws the last ticket: it has acquired,
// may read what the others stored, and has zeroed the word for the next launch (stream-ordered behind this one).
__device__ __forceinline__ bool last_to_arrive(uint32_t* arrivals, volatile uint32_t* s_ticket, uint32_t n) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *s_ticket = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (*s_ticket != n - 1u) return false;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *arrivals = 0u;
  }
  __syncthreads();
  return true;
}

// one attention layer forward with the caller's convolution routine: the two sum in different orders
template <bool SPLIT_CONV, int K>
__device__ __forceinline__ void att_conv(const float* x, const float* w, const float* bias, float* y, int cin, int cout,
                                         int len, bool act) {
  if constexpr (SPLIT_CONV) conv_forward_split<K, 1>(x, w, bias, y, cin, cout, len, len, act);
  else conv_forward<K, 1>(x, w, bias, y, 1, cin, cout, len, len, act);
}

// AudioAttNet over the eight windows + the expression MLP, forward.  F2 = the feature block [8][A]; aa[L.<act>] = the
// activations xt .. eh (FrameLayout order); wa = group 5 in LDS, laid out by aw: staged before the call, or its loads
// issued and left to the first barrier here.  T = threads of the workgroup: FW with conv_forward_split, FT without.
template <int T, bool SPLIT_CONV>
__device__ __forceinline__ void attention_forward(const float* F2, float* aa, const FrameLayout& L, const float* wa,
                                                  const AttW& aw, int A, const float* __restrict__ e,
                                                  float* __restrict__ enc_a, float* __restrict__ enc_e, bool has_exp) {
  static_assert(T == (SPLIT_CONV ? FW : FT), "the convolution routines are written for these workgroup sizes");
  const int tid = threadIdx.x;
  for (int i = tid; i < A * NB; i += T) {              // xt[j][t] = feat[t][j]
    const int t = i % NB, j = i / NB;
    aa[L.xt + i] = F2[t * A + j];
  }
  __syncthreads();
  if (has_exp && tid >= T - 16) {                      // expression hidden layer on an idle part of the block
    const int h = tid - (T - 16);
    float acc = 0.f;
    for (int i = 0; i < 5; ++i) acc += wa[aw.e1 + h * 5 + i] * e[i];
    aa[L.eh + h] = fmaxf(acc, 0.f);
  }
  const int act[NATT + 1] = {L.xt, L.c1, L.c2, L.c3, L.c4, L.c5, L.z};    // layer i reads act[i], writes act[i + 1]
#pragma unroll
  for (int i = 0; i < NATT - 1; ++i) {
    const AttLayer l = att_layer(i, A);
    att_conv<SPLIT_CONV, 3>(aa + act[i], wa + aw.w[i], wa + aw.b[i], aa + act[i + 1], l.cin, l.cout, NB, true);
    __syncthreads();
  }
  att_conv<SPLIT_CONV, 1>(aa + L.c5, wa + aw.w[5], wa + aw.b[5], aa + L.z, NB, NB, 1, false);   // the linear layer
  __syncthreads();
  if (tid < NB) {
    float m = aa[L.z];
    for (int t = 1; t < NB; ++t) m = fmaxf(m, aa[L.z + t]);
    float sum = 0.f;
    for (int t = 0; t < NB; ++t) sum += expf(aa[L.z + t] - m);
    aa[L.y + tid] = expf(aa[L.z + tid] - m) / sum;
  }
  __syncthreads();
  for (int j = tid; j < A; j += T) {
    float acc = 0.f;
    for (int t = 0; t < NB; ++t) acc += aa[L.y + t] * F2[t * A + j];
    enc_a[j] = acc;
  }
  if (has_exp && tid >= T - 6) {
    const int q = tid - (T - 6);
    float acc;
    if (q < 5) {
      acc = 0.f;
      for (int h = 0; h < 16; ++h) acc += wa[aw.e2 + q * 16 + h] * aa[L.eh + h];
    } else {
      acc = e[5];
    }
    enc_e[q] = acc;
  }
}

// ... and backward (FT threads).  F2, sa as in attention_forward; gF2 / ga[L.<act>] = the gradients at the same offsets;
// sw = group 5 staged weights-only; G = the stage's 14 gradient slots in parameter order.  `write`: this workgroup
// stores them (every workgroup computes d feat; where several repeat the stage, one writes).  On return gF2 holds
// d feat; no barrier behind the last loop.
__device__ __forceinline__ void attention_backward(const float* F2, float* gF2, const float* sa, float* ga,
                                                   const FrameLayout& L, const float* sw, const AttW& aw, int A,
                                                   const float* __restrict__ e, const float* __restrict__ d_enc_a,
                                                   const float* __restrict__ d_enc_e, float* const* G, bool write,
                                                   bool has_exp) {
  const int tid = threadIdx.x;
  auto G0 = [&](int i) -> float* { return write ? G[i] : nullptr; };
  // enc_a = sum_t y[t] feat[t]: d_y, d_feat; then softmax
  if (tid < NB) {
    float acc = 0.f;
    for (int j = 0; j < A; ++j) acc += d_enc_a[j] * F2[tid * A + j];
    ga[L.y + tid] = acc;
  }
  for (int i = tid; i < NB * A; i += FT) gF2[i] = sa[L.y + i / A] * d_enc_a[i % A];
  if (has_exp && write) {
    // enc_e[q<5] = sum_h W2[q][h] eh[h], eh = relu(W1 e[:5]); 80 + 80 threads own one weight each
    // (two ifs, not if / else: merged into one store, the two arms would index G by a variable)
    const int t = tid - 64;
    if (t >= 0 && t < 80) {
      const int q = t / 16, h = t % 16;
      G[13][t] = (d_enc_e ? d_enc_e[q] : 0.f) * sa[L.eh + h];
    }
    if (t >= 80 && t < 160) {
      const int i = (t - 80) % 5, h = (t - 80) / 5;
      float dh = 0.f;
      if (d_enc_e && sa[L.eh + h] > 0.f)
        for (int q = 0; q < 5; ++q) dh += sw[aw.e2 + q * 16 + h] * d_enc_e[q];
      G[12][h * 5 + i] = dh * e[i];
    }
  }
  __syncthreads();
  if (tid < NB) {
    float dot = 0.f;
    for (int t = 0; t < NB; ++t) dot += sa[L.y + t] * ga[L.y + t];
    ga[L.z + tid] = sa[L.y + tid] * (ga[L.y + tid] - dot);
  }
  __syncthreads();
  conv_backward<1, 1>(sa + L.c5, ga + L.z, sw + aw.w[5], G0(10), G0(11), ga + L.c5, 1, NB, NB, 1, 1, true);
  __syncthreads();
  const int act[NATT + 1] = {L.xt, L.c1, L.c2, L.c3, L.c4, L.c5, L.z};
#pragma unroll
  for (int i = NATT - 2; i >= 0; --i) {
    const AttLayer l = att_layer(i, A);
    conv_backward<3, 1>(sa + act[i], ga + act[i + 1], sw + aw.w[i], G0(2 * i), G0(2 * i + 1), ga + act[i], 1, l.cin,
                        l.cout, NB, NB, i > 0);         // xt is no LeakyReLU output
    __syncthreads();
  }
  for (int i = tid; i < NB * A; i += FT) {              // feat[t][j] also feeds xt[j][t]
    const int j = i % A, t = i / A;
    gF2[i] += ga[L.xt + j * NB + t];
  }
}

__global__ void __launch_bounds__(FT)
frame_code_forward_kernel(FrameDims d, ParamPtrs P, const float* __restrict__ a, const float* __restrict__ e,
                          float* __restrict__ enc_a, float* __restrict__ enc_e, float* __restrict__ saved) {
  extern __shared__ __align__(16) float s[];
  const FrameLayout L = frame_layout(d.D, d.M, d.A);
  float* sw = s + ((L.end + 3) & ~3);            // weight staging buffer
  const int D = d.D, M = d.M, A = d.A;
  for (int i = threadIdx.x; i < NB * D * WIN; i += FT) s[L.x0 + i] = a[i];
  stage<FT>(sw, P.p[0], M * D * 3); stage<FT>(sw + M * D * 3, P.p[1], M);
  __syncthreads();
  conv_forward<3, 2>(s + L.x0, sw, sw + M * D * 3, s + L.a1, NB, D, M, 16, 8, true);
  __syncthreads();
  stage<FT>(sw, P.p[2], M * M * 3); stage<FT>(sw + M * M * 3, P.p[3], M);
  __syncthreads();
  conv_forward<3, 2>(s + L.a1, sw, sw + M * M * 3, s + L.a2, NB, M, M, 8, 4, true);
  __syncthreads();
  stage<FT>(sw, P.p[4], 64 * M * 3); stage<FT>(sw + 64 * M * 3, P.p[5], 64);
  __syncthreads();
  conv_forward<3, 2>(s + L.a2, sw, sw + 64 * M * 3, s + L.a3, NB, M, 64, 4, 2, true);
  __syncthreads();
  stage<FT>(sw, P.p[6], 64 * 64 * 3); stage<FT>(sw + 64 * 64 * 3, P.p[7], 64);
  __syncthreads();
  conv_forward<3, 2>(s + L.a3, sw, sw + 64 * 64 * 3, s + L.a4, NB, 64, 64, 2, 1, true);
  __syncthreads();
  stage<FT>(sw, P.p[8], 4096); stage<FT>(sw + 4096, P.p[9], 64); stage<FT>(sw + 4160, P.p[10], A * 64);
  stage<FT>(sw + 4160 + A * 64, P.p[11], A);
  __syncthreads();
  conv_forward<1, 1>(s + L.a4, sw, sw + 4096, s + L.f1, NB, 64, 64, 1, 1, true);
  __syncthreads();
  conv_forward<1, 1>(s + L.f1, sw + 4160, sw + 4160 + A * 64, s + L.f2, NB, 64, A, 1, 1, false);
  __syncthreads();
  const AttW aw = att_layout(A);
  stage_attention<FT>(sw, aw, P.p + 12, A, d.has_exp, false);         // complete at the stage's first barrier
  attention_forward<FT, false>(s + L.f2, s, L, sw, aw, A, e, enc_a, enc_e, d.has_exp);
  for (int i = threadIdx.x; i < L.end - L.a1; i += FT) saved[i] = s[L.a1 + i];
}

// ---- forward over NB workgroups --------------------------------------------------------------------------------
// AudioNet's eight windows are independent (scene/motion_net.py:67-99): workgroup b runs window b through the four
// convolutions and two linear layers with EVERY weight already in LDS (all staging loads are issued at kernel start:
// one memory round trip instead of one per layer), the last workgroup to finish runs AudioAttNet over the eight feature
// vectors (+ the expression MLP).  The single-workgroup form took 97 us, ~5 us per layer, almost all of it waiting
// for the layer's weights and for barriers.
__global__ void __launch_bounds__(FW)
frame_code_forward_split_kernel(FrameDims d, ParamPtrs P, const float* __restrict__ a, const float* __restrict__ e,
                                float* __restrict__ enc_a, float* __restrict__ enc_e, float* __restrict__ saved,
                                uint32_t* __restrict__ arrivals) {
  extern __shared__ __align__(16) float s[];      // (no static LDS: the dynamic block may be the whole 160 KB)
  const int D = d.D, M = d.M, A = d.A, b = blockIdx.x, tid = threadIdx.x;
  const FrameLayout L = frame_layout(D, M, A);
  // LDS: [weights of the six AudioNet layers][attention + expression weights][this window's activations][attention acts]
  const int w1 = 0, b1 = w1 + M * D * 3, w2 = b1 + ((M + 3) & ~3), b2 = w2 + M * M * 3, w3 = b2 + ((M + 3) & ~3),
            b3 = w3 + 64 * M * 3, w4 = b3 + 64, b4 = w4 + 64 * 64 * 3, w5 = b4 + 64, b5 = w5 + 4096, w6 = b5 + 64,
            b6 = w6 + A * 64, watt = b6 + ((A + 3) & ~3), acts = watt + att_floats(A);
  float* x0 = s + acts;                     // [D][16]
  float* a1 = x0 + D * WIN;                 // [M][8]
  float* a2 = a1 + M * 8;                   // [M][4]
  float* a3 = a2 + M * 4;                   // [64][2]
  float* a4 = a3 + 128;                     // [64]
  float* f1 = a4 + 64;                      // [64]
  float* f2 = f1 + 64;                      // [A]
  float* att = f2 + ((A + 3) & ~3);         // last workgroup: f2 of all windows [8][A], then xt .. eh in FrameLayout order
  volatile uint32_t* s_ticket = reinterpret_cast<volatile uint32_t*>(att + NB * A + (L.end - L.xt));
  // every load of the kernel's weights is issued here
  for (int i = tid; i < D * WIN; i += FW) x0[i] = a[b * D * WIN + i];
  stage<FW>(s + w1, P.p[0], M * D * 3); stage<FW>(s + b1, P.p[1], M);
  stage<FW>(s + w2, P.p[2], M * M * 3); stage<FW>(s + b2, P.p[3], M);
  stage<FW>(s + w3, P.p[4], 64 * M * 3); stage<FW>(s + b3, P.p[5], 64);
  stage<FW>(s + w4, P.p[6], 64 * 64 * 3); stage<FW>(s + b4, P.p[7], 64);
  stage<FW>(s + w5, P.p[8], 4096); stage<FW>(s + b5, P.p[9], 64);
  stage<FW>(s + w6, P.p[10], A * 64); stage<FW>(s + b6, P.p[11], A);
  const AttW aw = att_layout(A);
  stage_attention<FW>(s + watt, aw, P.p + 12, A, d.has_exp, false);
  __syncthreads();
  conv_forward_split<3, 2>(x0, s + w1, s + b1, a1, D, M, 16, 8, true);    __syncthreads();
  conv_forward_split<3, 2>(a1, s + w2, s + b2, a2, M, M, 8, 4, true);     __syncthreads();
  conv_forward_split<3, 2>(a2, s + w3, s + b3, a3, M, 64, 4, 2, true);    __syncthreads();
  conv_forward_split<3, 2>(a3, s + w4, s + b4, a4, 64, 64, 2, 1, true);   __syncthreads();
  conv_forward_split<1, 1>(a4, s + w5, s + b5, f1, 64, 64, 1, 1, true);   __syncthreads();
  conv_forward_split<1, 1>(f1, s + w6, s + b6, f2, 64, A, 1, 1, false);   __syncthreads();
  // this window's slices of the saved activations (batch-major arrays of FrameLayout, offsets relative to a1)
  {
    float* sv = saved - L.a1;
    for (int i = tid; i < M * 8; i += FW) sv[L.a1 + b * M * 8 + i] = a1[i];
    for (int i = tid; i < M * 4; i += FW) sv[L.a2 + b * M * 4 + i] = a2[i];
    for (int i = tid; i < 128; i += FW) sv[L.a3 + b * 128 + i] = a3[i];
    for (int i = tid; i < 64; i += FW) { sv[L.a4 + b * 64 + i] = a4[i]; sv[L.f1 + b * 64 + i] = f1[i]; }
    for (int i = tid; i < A; i += FW) sv[L.f2 + b * A + i] = f2[i];
  }
  if (!last_to_arrive(arrivals, s_ticket, NB)) return;
  // the last workgroup reads all eight feature vectors; activations in FrameLayout order from xt on
  float* F2 = att;                           // [8][A]
  float* aa = F2 + NB * A - L.xt;            // aa[L.<act>] for act in xt .. eh
  const float* svr = saved - L.a1;
  for (int i = tid; i < NB * A; i += FW) F2[i] = svr[L.f2 + i];
  __syncthreads();
  attention_forward<FW, true>(F2, aa, L, s + watt, aw, A, e, enc_a, enc_e, d.has_exp);
  {
    float* sv = saved - L.a1;
    for (int i = tid; i < L.end - L.xt; i += FW) sv[L.xt + i] = aa[L.xt + i];
  }
}

// floats of parameter i (C ABI order: 4 conv + 2 fc layers of AudioNet, 5 conv + 1 linear of AudioAttNet, the two
// expression layers; weight, bias each)
__host__ __device__ inline int param_floats(int i, int D, int M, int A) {
  const int n[NPARAM] = {M * D * 3, M, M * M * 3, M, 64 * M * 3, 64, 64 * 64 * 3, 64, 4096, 64, A * 64, A,
                         16 * A * 3, 16, 8 * 16 * 3, 8, 4 * 8 * 3, 4, 2 * 4 * 3, 2, 1 * 2 * 3, 1, NB * NB, NB, 80, 80};
  return n[i];
}
__host__ __device__ inline int param_total(int D, int M, int A) {
  int t = 0;
  for (int i = 0; i < NPARAM; ++i) t += param_floats(i, D, M, A);
  return t;
}

// SPLIT: one workgroup per audio window.  Every workgroup repeats the small attention / expression
// stage (it needs all eight windows' features) and then runs AudioNet's backward for ITS window only; the parameter
// gradients go to the workgroup's own row of `partial` [NB][param_total] and frame_code_grad_reduce_kernel adds the rows up
// in order (AudioNet's parameters) or takes row 0 (the attention stage's, identical in every row).
template <bool SPLIT>
__global__ void __launch_bounds__(FT)
frame_code_backward_kernel(FrameDims d, ParamPtrs P, GradPtrs G, const float* __restrict__ a,
                           const float* __restrict__ e, const float* __restrict__ saved,
                           const float* __restrict__ d_enc_a, const float* __restrict__ d_enc_e,
                           float* __restrict__ partial) {
  extern __shared__ __align__(16) float s[];
  const FrameLayout L = frame_layout(d.D, d.M, d.A);
  const int D = d.D, M = d.M, A = d.A;
  const int wb = SPLIT ? (int)blockIdx.x : 0;       // first window and number of windows of this workgroup
  const int WB = SPLIT ? 1 : NB;
  if (SPLIT) {
    float* row = partial + (size_t)blockIdx.x * param_total(D, M, A);
    int off = 0;
    for (int i = 0; i < NPARAM; ++i) { G.p[i] = row + off; off += param_floats(i, D, M, A); }
  }
  float* g = s + L.end - L.a1;                  // g[L.<act>] = gradient buffer of activation <act> (offsets >= a1)
  float* sw = s + ((2 * L.end - L.a1 + 3) & ~3);
  const AttW aw = att_layout(A);
  for (int i = threadIdx.x; i < NB * D * WIN; i += FT) s[L.x0 + i] = a[i];
  for (int i = threadIdx.x; i < L.end - L.a1; i += FT) s[L.a1 + i] = saved[i];
  stage_attention<FT>(sw, aw, P.p + 12, A, d.has_exp, true);
  __syncthreads();
  // every workgroup writes the stage's gradients: into G, or (SPLIT) into its row of `partial`
  attention_backward(s + L.f2, g + L.f2, s, g, L, sw, aw, A, e, d_enc_a, d_enc_e, G.p + 12, true, d.has_exp);
  stage<FT>(sw, P.p[8], 4096); stage<FT>(sw + 4096, P.p[10], A * 64);
  __syncthreads();
  // AudioNet, windows wb .. wb + WB - 1 (activations are [window][channel][position])
#define WIN_AT(base, c, l) ((base) + wb * (c) * (l))
  conv_backward<1, 1>(WIN_AT(s + L.f1, 64, 1), WIN_AT(g + L.f2, A, 1), sw + 4096, G.p[10], G.p[11], WIN_AT(g + L.f1, 64, 1), WB, 64, A, 1, 1, true); __syncthreads();
  conv_backward<1, 1>(WIN_AT(s + L.a4, 64, 1), WIN_AT(g + L.f1, 64, 1), sw, G.p[8], G.p[9], WIN_AT(g + L.a4, 64, 1), WB, 64, 64, 1, 1, true);         __syncthreads();
  stage<FT>(sw, P.p[6], 64 * 64 * 3);
  __syncthreads();
  conv_backward<3, 2>(WIN_AT(s + L.a3, 64, 2), WIN_AT(g + L.a4, 64, 1), sw, G.p[6], G.p[7], WIN_AT(g + L.a3, 64, 2), WB, 64, 64, 2, 1, true);         __syncthreads();
  stage<FT>(sw, P.p[4], 64 * M * 3);
  __syncthreads();
  conv_backward<3, 2>(WIN_AT(s + L.a2, M, 4), WIN_AT(g + L.a3, 64, 2), sw, G.p[4], G.p[5], WIN_AT(g + L.a2, M, 4), WB, M, 64, 4, 2, true);          __syncthreads();
  stage<FT>(sw, P.p[2], M * M * 3);
  __syncthreads();
  conv_backward<3, 2>(WIN_AT(s + L.a1, M, 8), WIN_AT(g + L.a2, M, 4), sw, G.p[2], G.p[3], WIN_AT(g + L.a1, M, 8), WB, M, M, 8, 4, true);           __syncthreads();
  conv_backward<3, 2>(WIN_AT(s + L.x0, D, 16), WIN_AT(g + L.a1, M, 8), nullptr, G.p[0], G.p[1], nullptr, WB, D, M, 16, 8, false);
#undef WIN_AT
}

__global__ void __launch_bounds__(256)
frame_code_grad_reduce_kernel(FrameDims d, GradPtrs G, const float* __restrict__ partial) {
  const int PT = param_total(d.D, d.M, d.A);
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= PT) return;
  int i = 0, off = 0;
  for (; i < NPARAM; ++i) {
    const int n = param_floats(i, d.D, d.M, d.A);
    if (t < off + n) break;
    off += n;
  }
  if (G.p[i] == nullptr) return;
  float v = partial[t];
  if (i < 12) {                         // AudioNet: one contribution per window, fixed order
    for (int b = 1; b < NB; ++b) v += partial[(size_t)b * PT + t];
  }
  G.p[i][t - off] = v;
}

inline int set_lds_limit() {
  if (int rc = set_max_dynamic_lds(reinterpret_cast<const void*>(frame_code_forward_kernel), 160 * 1024)) return rc;
  if (int rc = set_max_dynamic_lds(reinterpret_cast<const void*>(frame_code_backward_kernel<false>), 160 * 1024)) return rc;
  if (int rc = set_max_dynamic_lds(reinterpret_cast<const void*>(frame_code_backward_kernel<true>), 160 * 1024)) return rc;
  return set_max_dynamic_lds(reinterpret_cast<const void*>(frame_code_forward_split_kernel), 160 * 1024);
}

// LDS floats of the split forward kernel: all weights + one window's activations + the attention stage
inline size_t split_forward_floats(int D, int M, int A) {
  const FrameLayout L = frame_layout(D, M, A);
  size_t w = (size_t)M * D * 3 + ((M + 3) & ~3) + (size_t)M * M * 3 + ((M + 3) & ~3) + (size_t)64 * M * 3 + 64 +
             64 * 64 * 3 + 64 + 4096 + 64 + (size_t)A * 64 + ((A + 3) & ~3) + att_floats(A);
  size_t acts = (size_t)D * WIN + M * 8 + M * 4 + 128 + 64 + 64 + ((A + 3) & ~3) + NB * A + (L.end - L.xt);
  return w + acts + 8;
}

inline bool dims_ok(int D, int M, int A) {
  if (D < 1 || M < 1 || A < 1) return false;
  const FrameLayout L = frame_layout(D, M, A);
  return (size_t)(2 * L.end - L.a1 + 4 + weight_stage_floats(D, M, A)) * sizeof(float) <= 160u * 1024u;
}

// ---- the 'ave' extractor ---------------------------------------------------------------------------------------
// AudioNet_ave (scene/motion_net.py:132-149) is three linear layers 512 -> 256 -> 128 -> A (LeakyReLU after the first
// two) on the eight windows a [8][512]; AudioAttNet and the expression MLP follow unchanged.  The first weight alone is
// 512 KB: nothing is staged through LDS here.  A WAVE owns an output neuron: its 64 lanes load the neuron's row
// straight into registers (16 bytes per lane and load), use every weight for all eight windows (the windows sit in LDS)
// and add the 64 partial sums of each window up in a fixed butterfly, so each weight is read once per launch.
//   forward : fc1's 256 neurons are split over the workgroups of the launch; the last one to arrive (the arrival
//             protocol of frame_code_forward_split_kernel) runs fc2, fc3, the attention stage and the expression MLP.
//             A launch of ONE workgroup does everything and needs no arrival word.
//   backward: every workgroup repeats the small tail (attention, fc3, down to d z2), then takes ITS 16 fc1 neurons back
//             through fc2 and writes its rows of dW1 = dZ1^T a, db1 and its rows of dW2, db2: disjoint slices, eight-term
//             sums in window order, no workspace, no reduce launch.  Workgroup 0 writes the other gradients.
constexpr int AVE_IN = 512, AVE_H1 = 256, AVE_H2 = 128;
constexpr int AVE_WG = 16;        // workgroups of the split passes
constexpr int AVE_NPARAM = 20;
constexpr int AVE_WAVES = FT / 64;

struct AveDims { int A, has_exp; };
struct AveParamPtrs { const float* p[AVE_NPARAM]; };
struct AveGradPtrs { float* p[AVE_NPARAM]; };

// float offsets inside the saved block (and its LDS copy): z1 [8][256], z2 [8][128] (both after their LeakyReLU),
// f2 [8][A], then FrameLayout's xt .. eh
struct AveLayout { int z1, z2, f2, att, end; };
__host__ __device__ inline AveLayout ave_layout(int A) {
  const FrameLayout L = frame_layout(1, 1, A);
  AveLayout Y;
  Y.z1 = 0;
  Y.z2 = Y.z1 + NB * AVE_H1;
  Y.f2 = Y.z2 + NB * AVE_H2;
  Y.att = Y.f2 + NB * A;
  Y.end = Y.att + (L.end - L.xt);
  return Y;
}

inline size_t ave_forward_floats(int A) { return (size_t)NB * AVE_IN + ave_layout(A).end + att_floats(A) + 4; }
inline size_t ave_backward_floats(int A) {
  return (size_t)NB * AVE_IN + 2 * (size_t)ave_layout(A).end + (size_t)A * AVE_H2 + att_floats(A) + 2 * NB * 16;
}
inline bool ave_dims_ok(int A) {
  return A >= 1 && ave_backward_floats(A) * sizeof(float) <= 160u * 1024u &&
         ave_forward_floats(A) * sizeof(float) <= 160u * 1024u;
}

// The eight partial sums a lane holds, one per window, added up over the wave: the sum of window w = lane >> 3 in every
// lane.  Three exchange steps that halve the windows a lane holds, three plain steps; the order is fixed.
__device__ __forceinline__ float wave_fold8(const float (&acc)[NB], int lane) {
  const bool h5 = (lane & 32) != 0, h4 = (lane & 16) != 0, h3 = (lane & 8) != 0;
  float u[4], t2[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = (h5 ? acc[4 + i] : acc[i]) + __shfl_xor(h5 ? acc[i] : acc[4 + i], 32);
#pragma unroll
  for (int i = 0; i < 2; ++i) t2[i] = (h4 ? u[2 + i] : u[i]) + __shfl_xor(h4 ? u[i] : u[2 + i], 16);
  float r = (h3 ? t2[1] : t2[0]) + __shfl_xor(h3 ? t2[0] : t2[1], 8);
  r += __shfl_xor(r, 4);
  r += __shfl_xor(r, 2);
  r += __shfl_xor(r, 1);
  return r;
}

// sum_k w[k] * x[w][k] (k < K) for the window w = lane >> 3, in every lane.  x [8][K] lives in LDS (16-byte aligned).
// STRIDE == 1: w = row, a dense row (`vec`: it is 16-byte aligned).  STRIDE == 3: w[k] = row[3 k + 1], the centre taps
// of a k3 convolution row [K][3] whose outer taps only meet padding: they are not loaded.  A lane multiplies its K / 64
// weights with all eight windows, then wave_fold8.
template <int K, int STRIDE = 1>
__device__ __forceinline__ float wave_dot8(const float* __restrict__ row, bool vec, const float* x, int lane) {
  constexpr int V = K >= 256 ? 4 : K >= 128 ? 2 : 1;         // consecutive weights per lane and chunk
  constexpr int NC = K / (64 * V);
  float w[NC][V];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float* src = row + (c * 64 * V + lane * V) * STRIDE + STRIDE / 2;
    if (STRIDE == 1 && V > 1 && vec) {
      if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(src);
        w[c][0] = t.x; w[c][1] = t.y; w[c][2] = t.z; w[c][3] = t.w;
      } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2*>(src);
        w[c][0] = t.x; w[c][1] = t.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) w[c][j] = src[j * STRIDE];
    }
  }
  float acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float s0 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float* xs = x + b * K + c * 64 * V + lane * V;
      if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(xs);
        s0 += w[c][0] * t.x; s0 += w[c][1] * t.y; s0 += w[c][2] * t.z; s0 += w[c][3] * t.w;
      } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2*>(xs);
        s0 += w[c][0] * t.x; s0 += w[c][1] * t.y;
      } else {
        s0 += w[c][0] * xs[0];
      }
    }
    acc[b] = s0;
  }
  return wave_fold8(acc, lane);
}

// vec: bit 0 / 1 / 2 = the weight of fc1 / fc2 / fc3 is 16-byte aligned
__global__ void __launch_bounds__(FT)
frame_code_ave_forward_kernel(AveDims d, AveParamPtrs P, const float* __restrict__ a, const float* __restrict__ e,
                              float* __restrict__ enc_a, float* __restrict__ enc_e, float* saved, uint32_t* arrivals,
                              int vec) {
  extern __shared__ __align__(16) float s[];
  const int A = d.A, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwg = gridDim.x;
  const FrameLayout L = frame_layout(1, 1, A);
  const AveLayout Y = ave_layout(A);
  float* xa = s;                                // a [8][512]
  float* act = xa + NB * AVE_IN;                // the saved block
  float* sw = act + Y.end;                      // attention + expression weights
  volatile uint32_t* s_ticket = reinterpret_cast<volatile uint32_t*>(sw + att_floats(A));
  for (int i = tid; i < NB * AVE_IN; i += FT) xa[i] = a[i];
  const AttW aw = att_layout(A);
  stage_attention<FT>(sw, aw, P.p + 6, A, d.has_exp, false);
  __syncthreads();
  // fc1: this workgroup's neurons, all eight windows
  const int per = AVE_H1 / nwg, n0 = (int)blockIdx.x * per;
  for (int j = wave; j < per; j += AVE_WAVES) {
    const int n = n0 + j;
    const float v = wave_dot8<AVE_IN>(P.p[0] + (size_t)n * AVE_IN, (vec & 1) != 0, xa, lane);
    if ((lane & 7) == 0) {
      const int w = lane >> 3;
      const float z = leaky(v + P.p[1][n]);
      saved[Y.z1 + w * AVE_H1 + n] = z;
      if (nwg == 1) act[Y.z1 + w * AVE_H1 + n] = z;
    }
  }
  if (nwg > 1) {
    if (!last_to_arrive(arrivals, s_ticket, nwg)) return;
    // the last workgroup reads all of z1
    for (int i = tid; i < NB * AVE_H1; i += FT) act[Y.z1 + i] = saved[Y.z1 + i];
  }
  __syncthreads();
  for (int j = wave; j < AVE_H2; j += AVE_WAVES) {
    const float v = wave_dot8<AVE_H1>(P.p[2] + (size_t)j * AVE_H1, (vec & 2) != 0, act + Y.z1, lane);
    if ((lane & 7) == 0) act[Y.z2 + (lane >> 3) * AVE_H2 + j] = leaky(v + P.p[3][j]);
  }
  __syncthreads();
  for (int j = wave; j < A; j += AVE_WAVES) {
    const float v = wave_dot8<AVE_H2>(P.p[4] + (size_t)j * AVE_H2, (vec & 4) != 0, act + Y.z2, lane);
    if ((lane & 7) == 0) act[Y.f2 + (lane >> 3) * A + j] = v + P.p[5][j];
  }
  __syncthreads();
  // activations in FrameLayout order from xt on: aa[L.<act>] for act in xt .. eh
  attention_forward<FT, false>(act + Y.f2, act + Y.att - L.xt, L, sw, aw, A, e, enc_a, enc_e, d.has_exp);
  for (int i = tid; i < Y.end - Y.z2; i += FT) saved[Y.z2 + i] = act[Y.z2 + i];
}

// vec: bit 0 = the gradient of fc1's weight is 16-byte aligned
__global__ void __launch_bounds__(FT)
frame_code_ave_backward_kernel(AveDims d, AveParamPtrs P, AveGradPtrs G, const float* __restrict__ a,
                               const float* __restrict__ e, const float* __restrict__ saved,
                               const float* __restrict__ d_enc_a, const float* __restrict__ d_enc_e, int vec) {
  static_assert(FT == 1024 && AVE_H1 / AVE_WG == 16 && AVE_H2 % AVE_WG == 0, "the thread maps below assume these");
  extern __shared__ __align__(16) float s[];
  const int A = d.A, tid = threadIdx.x;
  const bool first = blockIdx.x == 0;           // writes the gradients that are the same in every workgroup
  const FrameLayout L = frame_layout(1, 1, A);
  const AveLayout Y = ave_layout(A);
  float* xa = s;                                // a [8][512]
  float* act = xa + NB * AVE_IN;                // saved activations
  float* g = act + Y.end;                       // their gradients, same offsets
  float* w3 = g + Y.end;                        // fc3 weight [A][128]
  float* sw = w3 + A * AVE_H2;                  // attention + expression weights
  float* part = sw + att_floats(A);             // [8][2][16] partial sums of d z1
  const AttW aw = att_layout(A);
  for (int i = tid; i < NB * AVE_IN; i += FT) xa[i] = a[i];
  for (int i = tid; i < Y.end; i += FT) act[i] = saved[i];
  stage_attention<FT>(sw, aw, P.p + 6, A, d.has_exp, true);
  stage<FT>(w3, P.p[4], A * AVE_H2);
  __syncthreads();
  float* gF2 = g + Y.f2;
  auto G0 = [&](int i) -> float* { return first ? G.p[i] : nullptr; };
  // sa[L.<act>], ga[L.<act>] for act in xt .. eh
  attention_backward(act + Y.f2, gF2, act + Y.att - L.xt, g + Y.att - L.xt, L, sw, aw, A, e, d_enc_a, d_enc_e, G.p + 6,
                     first, d.has_exp);
  __syncthreads();
  // fc3 (no activation behind it): dW3, db3 once, d z2 (before its LeakyReLU) in every workgroup
  conv_backward<1, 1>(act + Y.z2, gF2, w3, G0(4), G0(5), g + Y.z2, NB, AVE_H2, A, 1, 1, true);
  __syncthreads();
  const float* z1 = act + Y.z1;
  const float* gz2 = g + Y.z2;
  // fc2: this workgroup's rows of dW2 [128][256] and db2
  {
    constexpr int ROWS = AVE_H2 / AVE_WG;
    const int r0 = (int)blockIdx.x * ROWS;
    for (int idx = tid; idx < ROWS * AVE_H1 + ROWS; idx += FT) {
      float acc = 0.f;
      if (idx < ROWS * AVE_H1) {
        const int j = r0 + idx / AVE_H1, k = idx % AVE_H1;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc += gz2[b * AVE_H2 + j] * z1[b * AVE_H1 + k];
        G.p[2][j * AVE_H1 + k] = acc;
      } else {
        const int j = r0 + idx - ROWS * AVE_H1;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc += gz2[b * AVE_H2 + j];
        G.p[3][j] = acc;
      }
    }
  }
  // d z1 of this workgroup's 16 neurons: wave = (window, half of the 128 fc2 rows), lane = (quarter of the half, neuron)
  const int n0 = (int)blockIdx.x * 16;
  {
    const int wave = tid >> 6, lane = tid & 63, b = wave >> 1, half = wave & 1, jq = lane >> 4, kk = lane & 15;
    const float* w2 = P.p[2] + n0 + kk;
    float acc = 0.f;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = half * 64 + jq * 16 + jj;
      acc += w2[(size_t)j * AVE_H1] * gz2[b * AVE_H2 + j];
    }
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    if (jq == 0) part[(b * 2 + half) * 16 + kk] = acc;
  }
  __syncthreads();
  float* gz1 = g + Y.z1;                        // [8][16]: only this workgroup's neurons
  if (tid < NB * 16) {
    const int b = tid >> 4, kk = tid & 15;
    gz1[tid] = (part[(b * 2) * 16 + kk] + part[(b * 2 + 1) * 16 + kk]) * dleaky(z1[b * AVE_H1 + n0 + kk]);
  }
  __syncthreads();
  // dW1 rows n0 .. n0 + 15 (512 contiguous floats each) and db1
  {
    const int c = tid & 127, r = tid >> 7;
    float4 x4[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) x4[b] = *reinterpret_cast<const float4*>(xa + b * AVE_IN + 4 * c);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kk = r + 8 * h;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float gv = gz1[b * 16 + kk];
        acc.x += gv * x4[b].x; acc.y += gv * x4[b].y; acc.z += gv * x4[b].z; acc.w += gv * x4[b].w;
      }
      float* dst = G.p[0] + (size_t)(n0 + kk) * AVE_IN + 4 * c;
      if (vec & 1) {
        *reinterpret_cast<float4*>(dst) = acc;
      } else {
        dst[0] = acc.x; dst[1] = acc.y; dst[2] = acc.z; dst[3] = acc.w;
      }
    }
    if (tid < 16) {
      float acc = 0.f;
#pragma unroll
      for (int b = 0; b < NB; ++b) acc += gz1[b * 16 + tid];
      G.p[1][n0 + tid] = acc;
    }
  }
}

inline int set_ave_lds_limit() {
  if (int rc = set_max_dynamic_lds(reinterpret_cast<const void*>(frame_code_ave_forward_kernel), 160 * 1024)) return rc;
  return set_max_dynamic_lds(reinterpret_cast<const void*>(frame_code_ave_backward_kernel), 160 * 1024);
}

// ---- the 'hubert' extractor: the wide AudioNet -----------------------------------------------------------------
// AudioNet(dim_in = D, dim_aud = A) on windows a [8][D][2] (scene/motion_net.py:67-99 with D = 1024): the slice keeps
// both samples, the lengths go 2 -> 1 -> 1 -> 1 -> 1, and the four k3 s2 p1 convolutions D -> 128 -> 128 -> 64 -> 64 are
// linear layers in disguise:
//   conv1   z1[b][co] = bias[co] + sum_ci (w[co][ci][1] a[b][ci][0] + w[co][ci][2] a[b][ci][1])   tap 0 meets padding only
//   conv2-4 only the centre tap w[co][ci][1] is live
// then Linear 64 -> 64 (leaky), Linear 64 -> A, AudioAttNet and the expression MLP as everywhere.  The parameters are
// the 26 of frame_code_*; the design is the 'ave' one: nothing of conv1 (1.5 MB at D = 1024) or conv2 passes
// through LDS in the forward pass, a wave owns an output neuron (wave_dot8 / wave_dot8_taps), dead taps are neither read for a product nor
// multiplied by zero, and their gradients are written as zeros.
//   forward : conv1's 128 neurons are split over the workgroups of the launch; the last one to arrive runs conv2 .. fc2
//             (weights straight from global memory, one neuron per wave), the attention stage and the expression MLP.
//             A launch of ONE workgroup does everything and needs no arrival word.
//   backward: every workgroup stages the small tail's weights (fc2, fc1, the centre taps of conv4 and conv3, the eight
//             columns of conv2's centre taps that belong to ITS conv1 neurons) in one round of loads, repeats the tail
//             down to d z1 of its 8 neurons, then writes its rows of dW1 (3 D contiguous floats each: tap 0 zero, taps 1
//             and 2 eight-term sums in window order) and db1.  Workgroup 0 writes every other gradient.  No workspace,
//             no float atomics, no reduce launch.
constexpr int WIDE_M = 128, WIDE_C = 64;
constexpr int WIDE_WG = 16;       // workgroups of the split passes
constexpr int WIDE_ROWS = WIDE_M / WIDE_WG;
constexpr int WIDE_WAVES = FT / 64;
constexpr int WIDE_MAX_CHUNKS = 4;             // D = 256 chunks of 4 channels x 64 lanes

struct WideDims { int D, A, has_exp; };

// float offsets inside the saved block (and its LDS copy): z1, z2 [8][128], z3, z4, f1 [8][64] (all after their
// LeakyReLU), f2 [8][A], then FrameLayout's xt .. eh
struct WideLayout { int z1, z2, z3, z4, f1, f2, att, end; };
__host__ __device__ inline WideLayout wide_layout(int A) {
  const FrameLayout L = frame_layout(1, 1, A);
  WideLayout Y;
  Y.z1 = 0;
  Y.z2 = Y.z1 + NB * WIDE_M;
  Y.z3 = Y.z2 + NB * WIDE_M;
  Y.z4 = Y.z3 + NB * WIDE_C;
  Y.f1 = Y.z4 + NB * WIDE_C;
  Y.f2 = Y.f1 + NB * WIDE_C;
  Y.att = Y.f2 + NB * A;
  Y.end = Y.att + (L.end - L.xt);
  return Y;
}

// backward: the tail's weights [fc2 A x 64][fc1 64 x 64][conv4 centre 64 x 64][conv3 centre 64 x 128]; the windows
// [8][2 D] take the same floats once the tail is through
__host__ __device__ inline int wide_tail_floats(int A) { return A * WIDE_C + 2 * WIDE_C * WIDE_C + WIDE_C * WIDE_M; }
__host__ __device__ inline int wide_region_floats(int D, int A) { return max(NB * 2 * D, wide_tail_floats(A)); }

inline size_t wide_forward_floats(int D, int A) {
  return (size_t)NB * 2 * D + wide_layout(A).end + att_floats(A) + 4;
}
inline size_t wide_backward_floats(int D, int A) {
  return (size_t)wide_region_floats(D, A) + WIDE_M * WIDE_ROWS + 2 * (size_t)wide_layout(A).end + att_floats(A);
}
inline bool wide_dims_ok(int D, int M, int A) {
  if (M != WIDE_M || D < 256 || D > 256 * WIDE_MAX_CHUNKS || D % 256 != 0 || A < 1 || A > 4096) return false;
  return wide_backward_floats(D, A) * sizeof(float) <= 160u * 1024u &&
         wide_forward_floats(D, A) * sizeof(float) <= 160u * 1024u;
}

// conv1 of the wide AudioNet, one output neuron: sum_ci (row[ci][1] x[w][ci][0] + row[ci][2] x[w][ci][1]) for the window
// w = lane >> 3, in every lane.  row [D][3] in global memory (`vec`: 16-byte aligned), x [8][D][2] in LDS, nc = D / 256.
// A lane takes four channels per chunk: 12 contiguous weights (three 16-byte loads, all chunks' loads issued before
// the first product) against 8 contiguous window floats (two 16-byte LDS reads); tap 0 takes no part.
__device__ __forceinline__ float wave_dot8_taps(const float* __restrict__ row, bool vec, const float* x, int lane,
                                                int nc) {
  float w[WIDE_MAX_CHUNKS][12];
#pragma unroll
  for (int c = 0; c < WIDE_MAX_CHUNKS; ++c) {
    if (c < nc) {
      const float* src = row + (c * 256 + lane * 4) * 3;
      if (vec) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float4 t = reinterpret_cast<const float4*>(src)[q];
          w[c][4 * q] = t.x; w[c][4 * q + 1] = t.y; w[c][4 * q + 2] = t.z; w[c][4 * q + 3] = t.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) w[c][j] = src[j];
      }
    }
  }
  const int D = nc * 256;
  float acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = 0.f;
#pragma unroll
  for (int c = 0; c < WIDE_MAX_CHUNKS; ++c) {
    if (c < nc) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float* xs = x + b * 2 * D + (c * 256 + lane * 4) * 2;
        const float4 t0 = *reinterpret_cast<const float4*>(xs), t1 = *reinterpret_cast<const float4*>(xs + 4);
        float s0 = acc[b];
        s0 += w[c][1] * t0.x; s0 += w[c][2] * t0.y; s0 += w[c][4] * t0.z; s0 += w[c][5] * t0.w;
        s0 += w[c][7] * t1.x; s0 += w[c][8] * t1.y; s0 += w[c][10] * t1.z; s0 += w[c][11] * t1.w;
        acc[b] = s0;
      }
    }
  }
  return wave_fold8(acc, lane);
}

// one layer of the tail, forward: y[w][j] = act(bias[j] + sum_k W[j][k] x[w][k]), a wave per neuron j < n
template <int K, int STRIDE>
__device__ __forceinline__ void wide_tail_layer(const float* __restrict__ W, const float* __restrict__ bias,
                                                const float* x, float* y, int n, bool act) {
  const int lane = threadIdx.x & 63;
  for (int j = threadIdx.x >> 6; j < n; j += WIDE_WAVES) {
    const float v = wave_dot8<K, STRIDE>(W + (size_t)j * K * STRIDE, false, x, lane);
    if ((lane & 7) == 0) y[(lane >> 3) * n + j] = act ? leaky(v + bias[j]) : v + bias[j];
  }
}

// vec: bit 0 = conv1's weight is 16-byte aligned
__global__ void __launch_bounds__(FT)
frame_code_wide_forward_kernel(WideDims d, ParamPtrs P, const float* __restrict__ a, const float* __restrict__ e,
                               float* __restrict__ enc_a, float* __restrict__ enc_e, float* saved, uint32_t* arrivals,
                               int vec) {
  extern __shared__ __align__(16) float s[];
  const int D = d.D, A = d.A, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwg = gridDim.x;
  const FrameLayout L = frame_layout(1, 1, A);
  const WideLayout Y = wide_layout(A);
  float* xa = s;                                // a [8][D][2]
  float* act = xa + NB * 2 * D;                 // the saved block
  float* sw = act + Y.end;                      // attention + expression weights
  volatile uint32_t* s_ticket = reinterpret_cast<volatile uint32_t*>(sw + att_floats(A));
  for (int i = tid; i < NB * 2 * D; i += FT) xa[i] = a[i];
  const AttW aw = att_layout(A);
  stage_attention<FT>(sw, aw, P.p + 12, A, d.has_exp, false);
  __syncthreads();
  // conv1: this workgroup's neurons, all eight windows
  const int per = WIDE_M / nwg, n0 = (int)blockIdx.x * per;
  for (int j = wave; j < per; j += WIDE_WAVES) {
    const int n = n0 + j;
    const float v = wave_dot8_taps(P.p[0] + (size_t)n * D * 3, (vec & 1) != 0, xa, lane, D / 256);
    if ((lane & 7) == 0) {
      const int w = lane >> 3;
      const float z = leaky(v + P.p[1][n]);
      saved[Y.z1 + w * WIDE_M + n] = z;
      if (nwg == 1) act[Y.z1 + w * WIDE_M + n] = z;
    }
  }
  if (nwg > 1) {
    if (!last_to_arrive(arrivals, s_ticket, nwg)) return;
    // the last workgroup reads all of z1
    for (int i = tid; i < NB * WIDE_M; i += FT) act[Y.z1 + i] = saved[Y.z1 + i];
  }
  __syncthreads();
  wide_tail_layer<WIDE_M, 3>(P.p[2], P.p[3], act + Y.z1, act + Y.z2, WIDE_M, true);   __syncthreads();
  wide_tail_layer<WIDE_M, 3>(P.p[4], P.p[5], act + Y.z2, act + Y.z3, WIDE_C, true);   __syncthreads();
  wide_tail_layer<WIDE_C, 3>(P.p[6], P.p[7], act + Y.z3, act + Y.z4, WIDE_C, true);   __syncthreads();
  wide_tail_layer<WIDE_C, 1>(P.p[8], P.p[9], act + Y.z4, act + Y.f1, WIDE_C, true);   __syncthreads();
  wide_tail_layer<WIDE_C, 1>(P.p[10], P.p[11], act + Y.f1, act + Y.f2, A, false);     __syncthreads();
  // activations in FrameLayout order from xt on: aa[L.<act>] for act in xt .. eh
  attention_forward<FT, false>(act + Y.f2, act + Y.att - L.xt, L, sw, aw, A, e, enc_a, enc_e, d.has_exp);
  for (int i = tid; i < Y.end - Y.z2; i += FT) saved[Y.z2 + i] = act[Y.z2 + i];
}

// Gradients of a k3 convolution [cout][cin][3] whose outer taps only met padding: the centre tap's eight-term sum in
// window order, the outer taps 0.0 (torch's value) without a product; and the bias gradient.  x [8][cin], g_out [8][cout].
__device__ __forceinline__ void centre_tap_grads(const float* x, const float* g_out, float* __restrict__ dW,
                                                 float* __restrict__ dbias, int cin, int cout) {
  const int nW = cout * cin * 3;
  for (int idx = threadIdx.x; idx < nW + cout; idx += FT) {
    float acc = 0.f;
    if (idx < nW) {
      if (idx % 3 == 1) {
        const int ci = (idx / 3) % cin, co = idx / (3 * cin);
#pragma unroll
        for (int b = 0; b < NB; ++b) acc += g_out[b * cout + co] * x[b * cin + ci];
      }
      dW[idx] = acc;
    } else {
      const int co = idx - nW;
#pragma unroll
      for (int b = 0; b < NB; ++b) acc += g_out[b * cout + co];
      dbias[co] = acc;
    }
  }
}

// dst[i] = the centre tap of src [n][3]
__device__ __forceinline__ void stage_centre_taps(float* dst, const float* __restrict__ src, int n) {
#pragma unroll 4
  for (int i = threadIdx.x; i < n; i += FT) dst[i] = src[3 * i + 1];
}

// vec: bit 0 = the gradient of conv1's weight is 16-byte aligned
__global__ void __launch_bounds__(FT)
frame_code_wide_backward_kernel(WideDims d, ParamPtrs P, GradPtrs G, const float* __restrict__ a,
                                const float* __restrict__ e, const float* __restrict__ saved,
                                const float* __restrict__ d_enc_a, const float* __restrict__ d_enc_e, int vec) {
  static_assert(FT == 1024 && WIDE_ROWS == 8 && NB == 8, "the thread maps below assume these");
  extern __shared__ __align__(16) float s[];
  const int D = d.D, A = d.A, tid = threadIdx.x;
  const bool first = blockIdx.x == 0;           // writes the gradients that are the same in every workgroup
  const int n0 = (int)blockIdx.x * WIDE_ROWS;   // this workgroup's conv1 neurons
  const FrameLayout L = frame_layout(1, 1, A);
  const WideLayout Y = wide_layout(A);
  float* wfc2 = s;                              // [A][64]; the region holds a [8][D][2] later
  float* wfc1 = wfc2 + A * WIDE_C;              // [64][64]
  float* w4c = wfc1 + WIDE_C * WIDE_C;          // conv4 centre taps [64][64]
  float* w3c = w4c + WIDE_C * WIDE_C;           // conv3 centre taps [64][128]
  float* xa = s;
  float* w2col = s + wide_region_floats(D, A);  // conv2 centre taps [128][8]: the columns of this workgroup's neurons
  float* act = w2col + WIDE_M * WIDE_ROWS;      // saved activations
  float* g = act + Y.end;                       // their gradients, same offsets
  float* sw = g + Y.end;                        // attention + expression weights
  const AttW aw = att_layout(A);
  // every load of the tail is issued here
  for (int i = tid; i < Y.end; i += FT) act[i] = saved[i];
  stage_attention<FT>(sw, aw, P.p + 12, A, d.has_exp, true);
  stage<FT>(wfc2, P.p[10], A * WIDE_C);
  stage<FT>(wfc1, P.p[8], WIDE_C * WIDE_C);
  stage_centre_taps(w4c, P.p[6], WIDE_C * WIDE_C);
  stage_centre_taps(w3c, P.p[4], WIDE_C * WIDE_M);
  w2col[tid] = P.p[2][((tid >> 3) * WIDE_M + n0 + (tid & 7)) * 3 + 1];
  __syncthreads();
  float* gF2 = g + Y.f2;
  auto G0 = [&](int i) -> float* { return first ? G.p[i] : nullptr; };
  // sa[L.<act>], ga[L.<act>] for act in xt .. eh
  attention_backward(act + Y.f2, gF2, act + Y.att - L.xt, g + Y.att - L.xt, L, sw, aw, A, e, d_enc_a, d_enc_e, G.p + 12,
                     first, d.has_exp);
  __syncthreads();
  // fc2 (no activation behind it), fc1: their gradients once, d(pre-activation) of the layer below in every workgroup
  conv_backward<1, 1>(act + Y.f1, gF2, wfc2, G0(10), G0(11), g + Y.f1, NB, WIDE_C, A, 1, 1, true);
  __syncthreads();
  conv_backward<1, 1>(act + Y.z4, g + Y.f1, wfc1, G0(8), G0(9), g + Y.z4, NB, WIDE_C, WIDE_C, 1, 1, true);
  __syncthreads();
  // conv4, conv3: linear layers on their centre taps
  conv_backward<1, 1>(act + Y.z3, g + Y.z4, w4c, nullptr, nullptr, g + Y.z3, NB, WIDE_C, WIDE_C, 1, 1, true);
  if (first) centre_tap_grads(act + Y.z3, g + Y.z4, G.p[6], G.p[7], WIDE_C, WIDE_C);
  __syncthreads();
  conv_backward<1, 1>(act + Y.z2, g + Y.z3, w3c, nullptr, nullptr, g + Y.z2, NB, WIDE_M, WIDE_C, 1, 1, true);
  if (first) centre_tap_grads(act + Y.z2, g + Y.z3, G.p[4], G.p[5], WIDE_M, WIDE_C);
  __syncthreads();
  // the tail's weights are through: the windows take their floats (complete at the barrier behind d z1)
  for (int i = tid; i < NB * 2 * D; i += FT) xa[i] = a[i];
  const float* z1 = act + Y.z1;
  const float* gz2 = g + Y.z2;
  if (first) centre_tap_grads(z1, gz2, G.p[2], G.p[3], WIDE_M, WIDE_M);
  // d z1 of this workgroup's 8 neurons: 16 lanes per (window, neuron), each sums 8 of the 128 conv2 rows
  float* gz1 = g + Y.z1;                        // [8][8]: only this workgroup's neurons
  {
    const int out = tid >> 4, part = tid & 15, b = out >> 3, kk = out & 7;
    float acc = 0.f;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int j = part * 8 + jj;
      acc += w2col[j * WIDE_ROWS + kk] * gz2[b * WIDE_M + j];
    }
    acc += __shfl_xor(acc, 8);
    acc += __shfl_xor(acc, 4);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 1);
    if (part == 0) gz1[b * WIDE_ROWS + kk] = acc * dleaky(z1[b * WIDE_M + n0 + kk]);
  }
  __syncthreads();
  // dW1 rows n0 .. n0 + 7 (3 D contiguous floats each) and db1: a thread owns four channels of a row, 12 floats
  const int nq = D / 4;
  for (int idx = tid; idx < WIDE_ROWS * nq; idx += FT) {
    const int c = idx % nq, kk = idx / nq;
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float gv = gz1[b * WIDE_ROWS + kk];
      const float4 x0 = *reinterpret_cast<const float4*>(xa + b * 2 * D + 8 * c);
      const float4 x1 = *reinterpret_cast<const float4*>(xa + b * 2 * D + 8 * c + 4);
      t[0] += gv * x0.x; t[1] += gv * x0.y; t[2] += gv * x0.z; t[3] += gv * x0.w;
      t[4] += gv * x1.x; t[5] += gv * x1.y; t[6] += gv * x1.z; t[7] += gv * x1.w;
    }
    float* dst = G.p[0] + (size_t)(n0 + kk) * D * 3 + 12 * c;
    if (vec & 1) {
      reinterpret_cast<float4*>(dst)[0] = make_float4(0.f, t[0], t[1], 0.f);
      reinterpret_cast<float4*>(dst)[1] = make_float4(t[2], t[3], 0.f, t[4]);
      reinterpret_cast<float4*>(dst)[2] = make_float4(t[5], 0.f, t[6], t[7]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) { dst[3 * i] = 0.f; dst[3 * i + 1] = t[2 * i]; dst[3 * i + 2] = t[2 * i + 1]; }
    }
  }
  if (tid < WIDE_ROWS) {
    float acc = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b) acc += gz1[b * WIDE_ROWS + tid];
    G.p[1][n0 + tid] = acc;
  }
}

inline int set_wide_lds_limit() {
  if (int rc = set_max_dynamic_lds(reinterpret_cast<const void*>(frame_code_wide_forward_kernel), 160 * 1024)) return rc;
  return set_max_dynamic_lds(reinterpret_cast<const void*>(frame_code_wide_backward_kernel), 160 * 1024);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The n parameter pointers of an entry point into P and, for a backward pass, the gradient pointers into G (else
// G == grads == nullptr).  Only the last two, the expression weights, may be NULL, and only without the branch.
inline int gather_params(const float** P, float** G, const float* const* params, float* const* grads, int n,
                         bool has_exp, const char* error) {
  for (int i = 0; i < n; ++i) {
    P[i] = params[i];
    if (G) G[i] = grads[i];
    INSTAG_REQUIRE((P[i] && (!G || G[i])) || (i >= n - 2 && !has_exp), error);
  }
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

int64_t instag_frame_code_saved_floats(int32_t dim_in, int32_t mid, int32_t dim_aud) {
  if (!dims_ok(dim_in, mid, dim_aud)) return -1;
  const FrameLayout L = frame_layout(dim_in, mid, dim_aud);
  return L.end - L.a1;
}

int instag_frame_code_forward(const float* a, const float* e, const float* const* params, float* enc_a,
                              float* enc_e, float* saved, int32_t dim_in, int32_t mid, int32_t dim_aud,
                              uint32_t* arrivals, instag_stream_t stream) {
  INSTAG_REQUIRE(a && params && enc_a && saved, "frame_code_forward: NULL tensor");
  INSTAG_REQUIRE(dims_ok(dim_in, mid, dim_aud), "frame_code: activations do not fit the 160 KB LDS");
  INSTAG_REQUIRE((e == nullptr) == (enc_e == nullptr), "frame_code_forward: e and enc_e go together");
  const int has_exp = e != nullptr;
  ParamPtrs P;
  if (int rc = gather_params(P.p, nullptr, params, nullptr, NPARAM, has_exp, "frame_code_forward: NULL parameter"))
    return rc;
  if (int rc = set_lds_limit()) return rc;
  const FrameLayout L = frame_layout(dim_in, mid, dim_aud);
  const FrameDims d{dim_in, mid, dim_aud, has_exp};
  const size_t split_bytes = split_forward_floats(dim_in, mid, dim_aud) * sizeof(float);
  if (arrivals != nullptr && split_bytes <= 160u * 1024u) {
    // one workgroup per audio window, the last one to arrive runs the attention stage (see the kernel)
    frame_code_forward_split_kernel<<<NB, FW, split_bytes, (hipStream_t)stream>>>(d, P, a, e, enc_a, enc_e, saved,
                                                                                   arrivals);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  }
  frame_code_forward_kernel<<<1, FT, (size_t)(L.end + 4 + weight_stage_floats(dim_in, mid, dim_aud)) * sizeof(float),
                              (hipStream_t)stream>>>(d, P, a, e, enc_a, enc_e,
                                                                                        saved);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

size_t instag_frame_code_backward_workspace_bytes(int32_t dim_in, int32_t mid, int32_t dim_aud) {
  if (!dims_ok(dim_in, mid, dim_aud)) return 0;
  return (size_t)NB * param_total(dim_in, mid, dim_aud) * sizeof(float);
}

int instag_frame_code_backward(const float* a, const float* e, const float* const* params, const float* saved,
                               const float* d_enc_a, const float* d_enc_e, float* const* grads, int32_t dim_in,
                               int32_t mid, int32_t dim_aud, void* workspace, size_t workspace_bytes,
                               instag_stream_t stream) {
  INSTAG_REQUIRE(a && params && saved && d_enc_a && grads, "frame_code_backward: NULL tensor");
  INSTAG_REQUIRE(dims_ok(dim_in, mid, dim_aud), "frame_code: activations do not fit the 160 KB LDS");
  const int has_exp = e != nullptr;
  ParamPtrs P;
  GradPtrs G;
  if (int rc = gather_params(P.p, G.p, params, grads, NPARAM, has_exp,
                             "frame_code_backward: NULL parameter / gradient"))
    return rc;
  if (int rc = set_lds_limit()) return rc;
  const FrameLayout L = frame_layout(dim_in, mid, dim_aud);
  const FrameDims d{dim_in, mid, dim_aud, has_exp};
  const size_t lds = (size_t)(2 * L.end - L.a1 + 4 + weight_stage_floats(dim_in, mid, dim_aud)) * sizeof(float);
  if (workspace != nullptr && workspace_bytes >= instag_frame_code_backward_workspace_bytes(dim_in, mid, dim_aud)) {
    // one workgroup per audio window + a fixed-order sum of the eight rows of parameter gradients
    frame_code_backward_kernel<true><<<NB, FT, lds, (hipStream_t)stream>>>(d, P, G, a, e, saved, d_enc_a, d_enc_e,
                                                                          (float*)workspace);
    INSTAG_CHECK_LAUNCH();
    const int PT = param_total(dim_in, mid, dim_aud);
    frame_code_grad_reduce_kernel<<<(PT + 255) / 256, 256, 0, (hipStream_t)stream>>>(d, G, (const float*)workspace);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  }
  frame_code_backward_kernel<false><<<1, FT, lds, (hipStream_t)stream>>>(d, P, G, a, e, saved, d_enc_a, d_enc_e, nullptr);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int64_t instag_frame_code_ave_saved_floats(int32_t dim_aud) {
  if (!ave_dims_ok(dim_aud)) return -1;
  return ave_layout(dim_aud).end;
}

int instag_frame_code_ave_forward(const float* a, const float* e, const float* const* params, float* enc_a,
                                  float* enc_e, float* saved, int32_t dim_aud, uint32_t* arrivals,
                                  instag_stream_t stream) {
  INSTAG_REQUIRE(a && params && enc_a && saved, "frame_code_ave_forward: NULL tensor");
  INSTAG_REQUIRE(ave_dims_ok(dim_aud), "frame_code_ave: activations do not fit the 160 KB LDS");
  INSTAG_REQUIRE((e == nullptr) == (enc_e == nullptr), "frame_code_ave_forward: e and enc_e go together");
  const int has_exp = e != nullptr;
  AveParamPtrs P;
  if (int rc = gather_params(P.p, nullptr, params, nullptr, AVE_NPARAM, has_exp,
                             "frame_code_ave_forward: NULL parameter"))
    return rc;
  if (int rc = set_ave_lds_limit()) return rc;
  const AveDims d{dim_aud, has_exp};
  const int vec = (aligned16(P.p[0]) ? 1 : 0) | (aligned16(P.p[2]) ? 2 : 0) | (aligned16(P.p[4]) ? 4 : 0);
  // with an arrival word fc1 is split over AVE_WG workgroups and the last one to arrive runs the rest
  frame_code_ave_forward_kernel<<<arrivals ? AVE_WG : 1, FT, ave_forward_floats(dim_aud) * sizeof(float),
                                  (hipStream_t)stream>>>(d, P, a, e, enc_a, enc_e, saved, arrivals, vec);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

size_t instag_frame_code_ave_backward_workspace_bytes(int32_t) { return 0; }

int instag_frame_code_ave_backward(const float* a, const float* e, const float* const* params, const float* saved,
                                   const float* d_enc_a, const float* d_enc_e, float* const* grads, int32_t dim_aud,
                                   void*, size_t, instag_stream_t stream) {
  INSTAG_REQUIRE(a && params && saved && d_enc_a && grads, "frame_code_ave_backward: NULL tensor");
  INSTAG_REQUIRE(ave_dims_ok(dim_aud), "frame_code_ave: activations do not fit the 160 KB LDS");
  const int has_exp = e != nullptr;
  AveParamPtrs P;
  AveGradPtrs G;
  if (int rc = gather_params(P.p, G.p, params, grads, AVE_NPARAM, has_exp,
                             "frame_code_ave_backward: NULL parameter / gradient"))
    return rc;
  if (int rc = set_ave_lds_limit()) return rc;
  const AveDims d{dim_aud, has_exp};
  frame_code_ave_backward_kernel<<<AVE_WG, FT, ave_backward_floats(dim_aud) * sizeof(float), (hipStream_t)stream>>>(
      d, P, G, a, e, saved, d_enc_a, d_enc_e, aligned16(G.p[0]) ? 1 : 0);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int64_t instag_frame_code_wide_saved_floats(int32_t dim_in, int32_t mid, int32_t dim_aud) {
  if (!wide_dims_ok(dim_in, mid, dim_aud)) return -1;
  return wide_layout(dim_aud).end;
}

int instag_frame_code_wide_forward(const float* a, const float* e, const float* const* params, float* enc_a,
                                   float* enc_e, float* saved, int32_t dim_in, int32_t mid, int32_t dim_aud,
                                   uint32_t* arrivals, instag_stream_t stream) {
  INSTAG_REQUIRE(a && params && enc_a && saved, "frame_code_wide_forward: NULL tensor");
  INSTAG_REQUIRE(wide_dims_ok(dim_in, mid, dim_aud),
                 "frame_code_wide: dim_in must be 256, 512, 768 or 1024, mid 128, and dim_aud fit the 160 KB LDS");
  INSTAG_REQUIRE((e == nullptr) == (enc_e == nullptr), "frame_code_wide_forward: e and enc_e go together");
  const int has_exp = e != nullptr;
  ParamPtrs P;
  if (int rc = gather_params(P.p, nullptr, params, nullptr, NPARAM, has_exp, "frame_code_wide_forward: NULL parameter"))
    return rc;
  if (int rc = set_wide_lds_limit()) return rc;
  const WideDims d{dim_in, dim_aud, has_exp};
  // with an arrival word conv1 is split over WIDE_WG workgroups and the last one to arrive runs the rest
  frame_code_wide_forward_kernel<<<arrivals ? WIDE_WG : 1, FT, wide_forward_floats(dim_in, dim_aud) * sizeof(float),
                                   (hipStream_t)stream>>>(d, P, a, e, enc_a, enc_e, saved, arrivals,
                                                          aligned16(P.p[0]) ? 1 : 0);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_frame_code_wide_backward(const float* a, const float* e, const float* const* params, const float* saved,
                                    const float* d_enc_a, const float* d_enc_e, float* const* grads, int32_t dim_in,
                                    int32_t mid, int32_t dim_aud, void*, size_t, instag_stream_t stream) {
  INSTAG_REQUIRE(a && params && saved && d_enc_a && grads, "frame_code_wide_backward: NULL tensor");
  INSTAG_REQUIRE(wide_dims_ok(dim_in, mid, dim_aud),
                 "frame_code_wide: dim_in must be 256, 512, 768 or 1024, mid 128, and dim_aud fit the 160 KB LDS");
  const int has_exp = e != nullptr;
  ParamPtrs P;
  GradPtrs G;
  if (int rc = gather_params(P.p, G.p, params, grads, NPARAM, has_exp,
                             "frame_code_wide_backward: NULL parameter / gradient"))
    return rc;
  if (int rc = set_wide_lds_limit()) return rc;
  const WideDims d{dim_in, dim_aud, has_exp};
  frame_code_wide_backward_kernel<<<WIDE_WG, FT, wide_backward_floats(dim_in, dim_aud) * sizeof(float),
                                    (hipStream_t)stream>>>(d, P, G, a, e, saved, d_enc_a, d_enc_e,
                                                           aligned16(G.p[0]) ? 1 : 0);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
