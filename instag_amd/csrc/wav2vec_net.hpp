// What the two entries of the wav2vec 2.0 "stable layer norm" network share: wav2vec.hip (CTC logits, at most 128 rows,
// include/instag_wav2vec.h) and hubert.hip (the encoder's hidden states, at most 1024 rows, include/instag_hubert.h).
//
// Activations are time-major [B, T, C].  Everything heavy is the one GEMM of gemm_mfma.hpp: the convolutions 1..6 over
// overlapping rows (lda = stride C, K = kernel C), the positional convolution over a group-major zero-padded copy of h
// (batch x groups, lda = channels per group, K = kernel x channels per group), q|k|v as one product, the output
// projection and the two feed-forward products with bias, GELU and the residual in their epilogues and the feature
// projection.  Around it: layer 0 (one input channel: VALU) fused with its LayerNorm and GELU, a one-wave-per-row
// LayerNorm (+GELU) and the padded copy.  The attention is the entry's own and comes to run_network as a parameter.
// The LayerNorm, the plain product and the loop over the transformer's layers are transformer.hpp's, which the Sapiens
// backbone (sapiens.hip) shares.
//
// No atomics; every reduction has a fixed order and no kernel's arithmetic depends on the batch size.
#pragma once
#include "transformer.hpp"
#include "instag_wav2vec.h"

namespace instag {
namespace {

constexpr int N_CONV = 7;
constexpr int CONV_K[N_CONV] = {10, 3, 3, 3, 3, 2, 2};
constexpr int CONV_S[N_CONV] = {5, 2, 2, 2, 2, 2, 2};
constexpr int MAX_SAMPLES = 1 << 20;
constexpr float LN_EPS = 1e-5f, NORM_EPS = 1e-7f;

// ---- layer 0: conv1d(1 -> C, kernel 10, stride 5) on the normalised samples, LayerNorm over channels, GELU ---------------
// A workgroup walks ROWS0 output rows of one segment; thread t owns channels t, t + 256, ... (C <= 1024).
// stats: per segment (mean, 1 / sqrt(var + 1e-7)), or NULL for samples that are taken as given.
constexpr int ROWS0 = 16;
__global__ void __launch_bounds__(TB) conv0_kernel(const float* __restrict__ x, int n, const float* __restrict__ stats,
                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   float* __restrict__ out, int T0, int C) {
  __shared__ float s_a[4], s_b[4];
  const int b = blockIdx.y, t0 = blockIdx.x * ROWS0;
  const float mean = stats ? stats[2 * b] : 0.f, rstd = stats ? stats[2 * b + 1] : 1.f;
  const float* seg = x + (size_t)b * n;
  float wr[4][10], bs[4], ga[4], be[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = threadIdx.x + TB * q;
    const bool ok = c < C;
#pragma unroll
    for (int j = 0; j < 10; ++j) wr[q][j] = ok ? w[j * C + c] : 0.f;
    bs[q] = ok ? bias[c] : 0.f;
    ga[q] = ok ? gamma[c] : 0.f;
    be[q] = ok ? beta[c] : 0.f;
  }
  for (int t = t0; t < min(t0 + ROWS0, T0); ++t) {
    float xs[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) xs[j] = (seg[5 * t + j] - mean) * rstd;
    float y[4], s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 10; ++j) v = fmaf(wr[q][j], xs[j], v);
      y[q] = v + bs[q];
      if (threadIdx.x + TB * q < C) s += y[q];
    }
    const float mu = block_sum_256(s, s_a) / (float)C;
    float qq = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (threadIdx.x + TB * q < C) qq += (y[q] - mu) * (y[q] - mu);
    const float rs = 1.f / sqrtf(block_sum_256(qq, s_b) / (float)C + LN_EPS);
    float* row = out + ((size_t)b * T0 + t) * C;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = threadIdx.x + TB * q;
      if (c < C) row[c] = gelu_erf((y[q] - mu) * rs * ga[q] + be[q]);
    }
  }
}

// ---- h [B, T, H] -> pad [B, G, half + T + half - 1, H / G], zero rows in front and behind ---------------------------------
__global__ void __launch_bounds__(TB) pad_groups_kernel(const float* __restrict__ h, float* __restrict__ pad, int B, int T,
                                                        int H, int G, int half) {
  const int Cg = H / G, Tp = 2 * half + T - 1;
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)B * G * Tp * Cg) return;
  const int c = (int)(i % Cg);
  const int p = (int)((i / Cg) % Tp);
  const int g = (int)((i / ((size_t)Cg * Tp)) % G);
  const int b = (int)(i / ((size_t)Cg * Tp * G));
  const int t = p - half;
  pad[i] = (t >= 0 && t < T) ? h[((size_t)b * T + t) * H + g * Cg + c] : 0.f;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// head: the entry ends in the CTC head, so vocab counts
const char* shape_error(const instag_wav2vec_weights* w, bool head = true) {
  if (!w) return "NULL weights";
  if (w->heads < 1 || w->hidden != w->heads * HEAD_DIM) return "hidden / heads must be 64";
  if (w->conv_dim < 32 || w->conv_dim % 32 || w->conv_dim > MAX_ROW) return "conv_dim must be a multiple of 32 in [32, 1024]";
  if (w->hidden % 32 || w->hidden > MAX_ROW) return "hidden must be a multiple of 32, at most 1024";
  if (w->intermediate < 32 || w->intermediate % 32 || w->intermediate > 65536) return "intermediate must be a multiple of 32";
  if (w->layers < 1 || w->layers > INSTAG_WAV2VEC_MAX_LAYERS) return "layers must be in [1, INSTAG_WAV2VEC_MAX_LAYERS]";
  if (w->pos_kernel < 2 || w->pos_kernel % 2 || w->pos_kernel > 1024) return "pos_kernel must be even, in [2, 1024]";
  if (w->pos_groups < 1 || w->hidden % w->pos_groups || (w->hidden / w->pos_groups) % 32)
    return "hidden / pos_groups must be a multiple of 32";
  if (head && (w->vocab < 4 || w->vocab % 4 || w->vocab > 65536)) return "vocab must be a multiple of 4";
  return nullptr;
}

struct Plan {
  int t[N_CONV + 1];       // t[0] = n, t[l + 1] = rows after layer l
  size_t stats, buf_a, buf_b, h, x, qkv, ctx, ff, pad, total;      // offsets in floats
  int Tp;
};

// rows after every convolution, or false when the segment is too short, too long or gives more than max_t frames
bool make_plan(const instag_wav2vec_weights* w, int B, int n, int max_t, Plan* p) {
  if (B < 1 || B > 4096 || n < 400 || n > MAX_SAMPLES) return false;
  p->t[0] = n;
  for (int l = 0; l < N_CONV; ++l) p->t[l + 1] = (p->t[l] - CONV_K[l]) / CONV_S[l] + 1;
  const int T = p->t[N_CONV];
  if (T < 1 || T > max_t) return false;
  const size_t C = w->conv_dim, H = w->hidden, rows = (size_t)B * T;
  p->Tp = w->pos_kernel + T - 1;
  Arena a;
  p->stats = a.take((size_t)2 * B);
  p->buf_a = a.take((size_t)B * p->t[1] * C);
  p->buf_b = a.take((size_t)B * p->t[2] * C);
  p->h = a.take(rows * H);
  p->x = a.take(rows * H);
  p->qkv = a.take(rows * 3 * H);
  p->ctx = a.take(rows * H);
  p->ff = a.take(rows * w->intermediate);
  p->pad = a.take((size_t)B * p->Tp * H);
  p->total = a.off;
  return true;
}

// floats of the taps buffer: the seven convolution blocks [B, T_l, C], then projection, positional and two per layer [B, T, H]
size_t taps_floats(const instag_wav2vec_weights* w, int B, const Plan& p) {
  size_t n = 0;
  for (int l = 0; l < N_CONV; ++l) n += (size_t)B * p.t[l + 1] * w->conv_dim;
  return n + (size_t)(2 + 2 * w->layers) * B * p.t[N_CONV] * w->hidden;
}

// every pointer the network reads, the head's among them where the entry has one; who: the entry's name in the message
int require_weights(const instag_wav2vec_weights* w, const std::string& who, bool head) {
  for (int l = 0; l < N_CONV; ++l)
    INSTAG_REQUIRE(w->conv_w[l] && w->conv_b[l] && w->conv_ln_g[l] && w->conv_ln_b[l],
                   who + ": NULL weight in convolution " + std::to_string(l));
  INSTAG_REQUIRE(w->proj_ln_g && w->proj_ln_b && w->proj_w && w->proj_b && w->pos_w && w->pos_b && w->enc_ln_g &&
                     w->enc_ln_b && (!head || (w->head_w && w->head_b)), who + ": NULL weight outside the layers");
  for (int l = 0; l < w->layers; ++l)
    INSTAG_REQUIRE(w->ln1_g[l] && w->ln1_b[l] && w->qkv_w[l] && w->qkv_b[l] && w->out_w[l] && w->out_b[l] && w->ln2_g[l] &&
                       w->ln2_b[l] && w->ff1_w[l] && w->ff1_b[l] && w->ff2_w[l] && w->ff2_b[l],
                   who + ": NULL weight in layer " + std::to_string(l));
  return INSTAG_OK;
}

// What tells the entries of wav2vec.hip and hubert.hip apart in their checks: the prefix of their names, the text for a
// refused batch or length (it names the file's own frame bound), that bound, and whether the network ends in the CTC head.
struct Net {
  const char* name;
  const char* plan_error;
  int max_t;
  bool head;
};

// The plan of entry instag_<net>_<fn>, or false with the error set.  shape_text: say what is wrong with the dimensions
// (otherwise they are refused with the plan's text, as a batch or a length is).
bool entry_plan(const Net& net, const char* fn, bool shape_text, const instag_wav2vec_weights* w, int batch, int n_samples,
                Plan* p) {
  const std::string who = std::string(net.name) + "_" + fn;
  const char* e = shape_error(w, net.head);
  if (e && shape_text) {
    set_error(who + ": " + e);
    return false;
  }
  if (e || !make_plan(w, batch, n_samples, net.max_t, p)) {
    set_error(who + net.plan_error);
    return false;
  }
  return true;
}

// What a forward entry checks before its first launch, in this order: the dimensions, the tensors, the tile, the plan,
// the weights' pointers and the workspace's size.
int forward_prologue(const Net& net, const instag_wav2vec_weights* w, const void* in, const void* out, int batch,
                     int n_samples, const void* workspace, size_t workspace_bytes, int tile, Plan* p) {
  const std::string who = std::string(net.name) + "_forward";
  if (const char* e = shape_error(w, net.head)) {
    set_error(who + ": " + e);
    return INSTAG_E_ARG;
  }
  INSTAG_REQUIRE(in && out && workspace, who + ": NULL tensor");
  INSTAG_REQUIRE(tile >= 0 && tile <= 3, who + ": tile must be 0..3");
  if (!entry_plan(net, "forward", false, w, batch, n_samples, p)) return INSTAG_E_ARG;
  INSTAG_TRY(require_weights(w, who, net.head));
  if (workspace_bytes < p->total * sizeof(float)) {
    set_error(who + ": workspace smaller than instag_" + net.name + "_workspace_bytes(w, batch, n_samples)");
    return INSTAG_E_SPACE;
  }
  return INSTAG_OK;
}

// The network behind the samples' normalisation: feature extractor, projection, positional convolution, the layers and
// the encoder's last LayerNorm, which writes `out` [B, T, hidden] (a piece of the workspace, or the caller's tensor).
// stats: the per-segment statistics layer 0 applies, or NULL.  attention(qkv, ctx, B, T, H, st) -> code runs
// ctx = softmax(q k^T / 8) v of every (segment, head).
template <typename Attention>
int run_network(const instag_wav2vec_weights* w, const Plan& p, const float* segments, const float* stats, int B,
                float* ws, int tile, float* taps, float* out, hipStream_t st, Attention&& attention) {
  const int n = p.t[0], C = w->conv_dim, H = w->hidden, G = w->pos_groups;
  const int T = p.t[N_CONV], M = B * T, Cg = H / G;
  float* buf[2] = {ws + p.buf_a, ws + p.buf_b};
  float *h = ws + p.h, *x = ws + p.x, *qkv = ws + p.qkv, *ctx = ws + p.ctx, *ff = ws + p.ff, *pad = ws + p.pad;

  // the debug copy of a stage's output, in the order of instag_wav2vec_taps_floats
  size_t tap_off = 0;
  auto tap = [&](const float* src, size_t count) -> int {
    if (taps) {
      INSTAG_CHECK_HIP(hipMemcpyAsync(taps + tap_off, src, count * sizeof(float), hipMemcpyDeviceToDevice, st));
      tap_off += count;
    }
    return INSTAG_OK;
  };

  // feature extractor
  conv0_kernel<<<dim3((unsigned)div_up(p.t[1], ROWS0), (unsigned)B), TB, 0, st>>>(
      segments, n, stats, w->conv_w[0], w->conv_b[0], w->conv_ln_g[0], w->conv_ln_b[0], buf[0], p.t[1], C);
  INSTAG_CHECK_LAUNCH();
  INSTAG_TRY(tap(buf[0], (size_t)B * p.t[1] * C));
  int cur = 0;
  for (int l = 1; l < N_CONV; ++l) {
    GemmArgs g{};
    g.a = buf[cur]; g.w = w->conv_w[l]; g.bias = w->conv_b[l]; g.d = buf[cur ^ 1];
    g.M = B * p.t[l + 1]; g.rows = p.t[l + 1]; g.N = C; g.K = CONV_K[l] * C; g.groups = 1;
    g.a_batch = (int64_t)p.t[l] * C; g.lda = CONV_S[l] * C; g.d_batch = (int64_t)p.t[l + 1] * C; g.ldd = C;
    INSTAG_TRY(launch_gemm(g, st, tile));
    cur ^= 1;
    INSTAG_TRY(layernorm(buf[cur], buf[cur], w->conv_ln_g[l], w->conv_ln_b[l], (size_t)g.M, C, 1, LN_EPS, st));
    INSTAG_TRY(tap(buf[cur], (size_t)g.M * C));
  }
  // feature projection
  INSTAG_TRY(layernorm(buf[cur], buf[cur], w->proj_ln_g, w->proj_ln_b, M, C, 0, LN_EPS, st));
  INSTAG_TRY(linear(buf[cur], w->proj_w, w->proj_b, nullptr, h, M, C, H, 0, tile, st));
  INSTAG_TRY(tap(h, (size_t)M * H));
  // positional convolution: h += GELU(conv(h))
  {
    const size_t n_pad = (size_t)B * p.Tp * H;
    pad_groups_kernel<<<(unsigned)div_up(n_pad, (size_t)TB), TB, 0, st>>>(h, pad, B, T, H, G, w->pos_kernel / 2);
    INSTAG_CHECK_LAUNCH();
    GemmArgs g{};
    g.a = pad; g.w = w->pos_w; g.bias = w->pos_b; g.res = h; g.d = h;
    g.M = M; g.rows = T; g.N = Cg; g.K = w->pos_kernel * Cg; g.groups = G;
    g.a_batch = (int64_t)G * p.Tp * Cg; g.a_group = (int64_t)p.Tp * Cg; g.lda = Cg;
    g.d_batch = (int64_t)T * H; g.ldd = H; g.gelu = 1;
    INSTAG_TRY(launch_gemm(g, st, tile));
    INSTAG_TRY(tap(h, (size_t)M * H));
  }
  // transformer
  INSTAG_TRY(run_layers(w, B, T, LayerBuffers{h, x, qkv, ctx, ff}, LN_EPS, tile, tap, st, attention));
  return layernorm(h, out, w->enc_ln_g, w->enc_ln_b, M, H, 0, LN_EPS, st);
}

}  // namespace
}  // namespace instag
