// The pre-LayerNorm transformer layers every network of this library runs: wav2vec.hip and hubert.hip through
// wav2vec_net.hpp (LayerNorm eps 1e-5) and the Sapiens backbone of sapiens.hip (1e-6).  Token-major activations
// [B, T, hidden]; per layer
//
//   h += out(attention(q | k | v = W_qkv LayerNorm(h)))        h += W2 GELU(W1 LayerNorm(h))
//
// with q|k|v as one product, the erf-GELU and the residuals in the GEMM epilogues of gemm_mfma.hpp.  The attention is
// the caller's and comes as a parameter; heads are 64 wide.  The weights are any struct with the fields hidden,
// intermediate, layers and ln1_g, ln1_b, qkv_w, qkv_b, out_w, out_b, ln2_g, ln2_b, ff1_w, ff1_b, ff2_w, ff2_b per
// layer, every matrix [K][N] (instag_wav2vec_weights, instag_sapiens_weights).
//
// No atomics; every reduction has a fixed order and no kernel's arithmetic depends on the batch size.
#pragma once
#include "gemm_mfma.hpp"
#include "device_math.hpp"

namespace instag {
namespace {

constexpr int HEAD_DIM = 64;
constexpr int MAX_ROW = 1024;                          // a LayerNorm row: 16 values per lane of one wave

// ---- LayerNorm over a row of C <= 1024 (+ GELU), one wave per row; out may be in ----------------------------------------
__global__ void __launch_bounds__(TB) layernorm_kernel(const float* in, float* out, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, int rows, int C, int gelu, float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* src = in + (size_t)r * C;
  float v[MAX_ROW / 64], s = 0.f;
#pragma unroll
  for (int i = 0; i < MAX_ROW / 64; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < C ? src[c] : 0.f;
    s += v[i];
  }
  const float mu = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAX_ROW / 64; ++i)
    if (lane + 64 * i < C) q += (v[i] - mu) * (v[i] - mu);
  const float rs = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
  float* dst = out + (size_t)r * C;
#pragma unroll
  for (int i = 0; i < MAX_ROW / 64; ++i) {
    const int c = lane + 64 * i;
    if (c < C) {
      const float y = (v[i] - mu) * rs * gamma[c] + beta[c];
      dst[c] = gelu ? gelu_erf(y) : y;
    }
  }
}

int layernorm(const float* in, float* out, const float* g, const float* b, size_t rows, int C, int gelu, float eps,
              hipStream_t st) {
  layernorm_kernel<<<(unsigned)div_up(rows, (size_t)(TB / 64)), TB, 0, st>>>(in, out, g, b, (int)rows, C, gelu, eps);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

// D [M, N] = epilogue(A [M, K] W + bias): the ordinary case, one batch of contiguous rows
int linear(const float* a, const float* w, const float* bias, const float* res, float* d, int M, int K, int N, int gelu,
           int tile, hipStream_t st) {
  GemmArgs g{};
  g.a = a; g.w = w; g.bias = bias; g.res = res; g.d = d;
  g.M = M; g.rows = M; g.N = N; g.K = K; g.groups = 1; g.lda = K; g.ldd = N; g.gelu = gelu;
  return launch_gemm(g, st, tile);
}

// the pieces of the workspace the layers work in: h [M, hidden] in and out, x and ctx [M, hidden], qkv [M, 3 hidden],
// ff [M, intermediate]
struct LayerBuffers {
  float *h, *x, *qkv, *ctx, *ff;
};

// All layers of `w` on h [B, T, hidden], in place.  tap(h, count) -> code copies h behind every attention and every
// feed-forward; attention(qkv, ctx, B, T, H, st) -> code runs ctx = softmax(q k^T / 8) v of every (segment, head).
template <typename Weights, typename Tap, typename Attention>
int run_layers(const Weights* w, int B, int T, const LayerBuffers& b, float ln_eps, int tile, Tap&& tap, hipStream_t st,
               Attention&& attention) {
  const int H = w->hidden, I = w->intermediate, M = B * T;
  float *h = b.h, *x = b.x, *qkv = b.qkv, *ctx = b.ctx, *ff = b.ff;
  for (int l = 0; l < w->layers; ++l) {
    INSTAG_TRY(layernorm(h, x, w->ln1_g[l], w->ln1_b[l], M, H, 0, ln_eps, st));
    INSTAG_TRY(linear(x, w->qkv_w[l], w->qkv_b[l], nullptr, qkv, M, H, 3 * H, 0, tile, st));
    INSTAG_TRY(attention(qkv, ctx, B, T, H, st));
    INSTAG_TRY(linear(ctx, w->out_w[l], w->out_b[l], h, h, M, H, H, 0, tile, st));
    INSTAG_TRY(tap(h, (size_t)M * H));
    INSTAG_TRY(layernorm(h, x, w->ln2_g[l], w->ln2_b[l], M, H, 0, ln_eps, st));
    INSTAG_TRY(linear(x, w->ff1_w[l], w->ff1_b[l], nullptr, ff, M, H, I, 1, tile, st));
    INSTAG_TRY(linear(ff, w->ff2_w[l], w->ff2_b[l], h, h, M, I, H, 0, tile, st));
    INSTAG_TRY(tap(h, (size_t)M * H));
  }
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag
