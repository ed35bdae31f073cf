// wav2vec 2.0 CTC network of the 'esperanto' audio features (include/instag_wav2vec.h), fp32, forward only.
//
// The network up to the encoder's last LayerNorm is wav2vec_net.hpp's, shared with hubert.hip.  This file's own: the
// per-segment statistics, the head (one more GEMM), and the attention of one (segment, head) per workgroup with K, Q,
// V and the T x T scores in LDS, which bounds T by INSTAG_WAV2VEC_MAX_FRAMES.
//
// No atomics; every reduction has a fixed order and no kernel's arithmetic depends on the batch size.
#include "wav2vec_net.hpp"

namespace instag {
namespace {

constexpr int MAX_T = INSTAG_WAV2VEC_MAX_FRAMES;

// ---- per-segment mean and 1 / sqrt(var + 1e-7) ---------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) segment_stats_kernel(const float* __restrict__ x, int n, float* __restrict__ stats) {
  __shared__ float s_a[4], s_b[4];
  const float* seg = x + (size_t)blockIdx.x * n;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += TB) s += seg[i];
  const float mean = block_sum_256(s, s_a) / (float)n;
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += TB) {
    const float d = seg[i] - mean;
    q += d * d;
  }
  const float var = block_sum_256(q, s_b) / (float)n;
  if (threadIdx.x == 0) {
    stats[2 * blockIdx.x] = mean;
    stats[2 * blockIdx.x + 1] = 1.f / sqrtf(var + NORM_EPS);
  }
}

// ---- attention of one (segment, head): softmax(q k^T / 8) v, T <= MAX_T ---------------------------------------------------
// LDS: Q and K [T][65], behind them the scores [T][T + 1]; V [T][64] takes Q's and K's place once the scores stand.
constexpr int LDQ = HEAD_DIM + 1;
inline size_t attention_lds(int T) { return ((size_t)2 * T * LDQ + (size_t)T * (T + 1)) * sizeof(float); }

__global__ void __launch_bounds__(TB) attention_kernel(const float* __restrict__ qkv, float* __restrict__ ctx, int T, int H) {
  extern __shared__ float lds[];
  float* Q = lds;
  float* K = lds + T * LDQ;
  float* V = lds;
  float* S = lds + 2 * T * LDQ;
  const int LDS_S = T + 1;
  const int head = blockIdx.x, b = blockIdx.y;
  const float* base = qkv + (size_t)b * T * 3 * H + head * HEAD_DIM;
  for (int i = threadIdx.x; i < T * HEAD_DIM; i += TB) {
    const int t = i >> 6, d = i & 63;
    Q[t * LDQ + d] = base[(size_t)t * 3 * H + d];
    K[t * LDQ + d] = base[(size_t)t * 3 * H + H + d];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * T; i += TB) {
    const int r = i / T, c = i - r * T;
    float s = 0.f;
#pragma unroll 16
    for (int d = 0; d < HEAD_DIM; ++d) s = fmaf(Q[r * LDQ + d], K[c * LDQ + d], s);
    S[r * LDS_S + c] = s * 0.125f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * HEAD_DIM; i += TB) {
    const int t = i >> 6, d = i & 63;
    V[t * HEAD_DIM + d] = base[(size_t)t * 3 * H + 2 * H + d];
  }
  const int lane = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < T; r += TB / 64) {
    float* row = S + r * LDS_S;
    const float a0 = lane < T ? row[lane] : -INFINITY, a1 = lane + 64 < T ? row[lane + 64] : -INFINITY;
    const float mx = wave_max(fmaxf(a0, a1));
    const float e0 = lane < T ? expf(a0 - mx) : 0.f, e1 = lane + 64 < T ? expf(a1 - mx) : 0.f;
    const float inv = 1.f / wave_sum(e0 + e1);
    if (lane < T) row[lane] = e0 * inv;
    if (lane + 64 < T) row[lane + 64] = e1 * inv;
  }
  __syncthreads();
  float* dst = ctx + (size_t)b * T * H + head * HEAD_DIM;
  for (int i = threadIdx.x; i < T * HEAD_DIM; i += TB) {
    const int r = i >> 6, d = i & 63;
    float o = 0.f;
    for (int c = 0; c < T; ++c) o = fmaf(S[r * LDS_S + c], V[c * HEAD_DIM + d], o);
    dst[(size_t)r * H + d] = o;
  }
}

constexpr Net NET = {"wav2vec", ": batch in [1, 4096], 400 <= n_samples <= 2^20 and at most INSTAG_WAV2VEC_MAX_FRAMES frames",
                     MAX_T, true};

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_wav2vec_workspace_bytes(const instag_wav2vec_weights* w, int32_t batch, int32_t n_samples) {
  Plan p;
  return entry_plan(NET, "workspace_bytes", true, w, batch, n_samples, &p) ? p.total * sizeof(float) : 0;
}

size_t instag_wav2vec_taps_floats(const instag_wav2vec_weights* w, int32_t batch, int32_t n_samples) {
  Plan p;
  return entry_plan(NET, "taps_floats", false, w, batch, n_samples, &p) ? taps_floats(w, batch, p) : 0;
}

int instag_wav2vec_forward(const instag_wav2vec_weights* w, const float* segments, int32_t batch, int32_t n_samples,
                           float* logits, void* workspace, size_t workspace_bytes, int32_t tile, float* taps,
                           instag_stream_t stream) {
  Plan p;
  INSTAG_TRY(forward_prologue(NET, w, segments, logits, batch, n_samples, workspace, workspace_bytes, tile, &p));
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int B = batch, H = w->hidden, T = p.t[N_CONV];
  float *stats = ws + p.stats, *x = ws + p.x;
  segment_stats_kernel<<<B, TB, 0, st>>>(segments, n_samples, stats);
  INSTAG_CHECK_LAUNCH();
  const size_t lds = attention_lds(T);
  if (lds > 48 * 1024) INSTAG_TRY(set_max_dynamic_lds((const void*)attention_kernel, (int)attention_lds(MAX_T)));
  auto attention = [lds](const float* qkv, float* ctx, int B, int T, int H, hipStream_t st) -> int {
    attention_kernel<<<dim3((unsigned)(H / HEAD_DIM), (unsigned)B), TB, lds, st>>>(qkv, ctx, T, H);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  };
  INSTAG_TRY(run_network(w, p, segments, stats, B, ws, tile, taps, x, st, attention));
  return linear(x, w->head_w, w->head_b, nullptr, logits, B * T, H, w->vocab, 0, tile, st);
}

}  // extern "C"
