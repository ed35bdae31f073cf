// DeepSpeech 0.1.0 of the 'deepspeech' audio features (include/instag_deepspeech.h), fp32, forward only, batch 1.
//
// The five dense layers and the input projections of both LSTM directions are the GEMM of gemm_mfma.hpp, the clipped
// ReLU its epilogue option.  This file's own is the recurrence: per time step and direction a matrix-vector product of
// the previous output h [cell] against the recurrent weights [cell, 4 cell], then the gate arithmetic.  The steps are
// strictly in order, so a step is one plain launch that serves both directions (the stream orders the steps; nothing
// waits inside a kernel):
//
//   a wave owns one unit of one direction.  Its four weight rows (gates i, j, f, o) are stored one behind the other,
//   wh[dir][unit][gate][k], 4 cell contiguous floats; lane l takes the 16 bytes at k = 4 (l + 64 n) of each row, n = 0 ..
//   cell / 256 - 1, against the same four floats of h, which the workgroup's four waves (always of one direction)
//   share through LDS.  A lane's partial sums run over n in order, the 64 lanes are folded by the xor butterfly of
//   wave_sum: one fixed order, the same for every unit, direction and sequence length.  Then z = sum + xp[t][dir]
//   (the precomputed input half with the bias), the cell state is updated in place and h_t goes straight into column
//   block dir of row t of the [S, 2 cell] array layer 5 reads; h_{t-1} is that array's neighbouring row.
//
// A step reads all of wh, 2 x 4 cell^2 floats (128 MiB at 2048 cells): every step streams them again, from the
// Infinity Cache where they fit.  No atomics.
//
// Time blocks.  xp is 8 cell floats a step, so the dense layers in front of the recurrence run in blocks of at most
// max_rows steps: steps [s0, s1) need the rows [s0, s1) forward and their mirror image [S - s1, S - s0) backward, which
// go through layers 1..3 as one batch of 2 (s1 - s0) rows (the two halves of a grouped GEMM's A: group = direction) --
// or, when one block holds the whole sequence, as S rows that both groups read.  The cell states and the output array
// live across blocks.  Layers 5 and 6 follow in blocks of their own.  A GEMM's element does not depend on the rows it
// was tiled with, so the result does not depend on max_rows.
#include "gemm_mfma.hpp"
#include "device_math.hpp"
#include "instag_deepspeech.h"

namespace instag {
namespace {

constexpr int MAX_CELL = INSTAG_DEEPSPEECH_MAX_CELL;
constexpr int MAX_STEPS = INSTAG_DEEPSPEECH_MAX_STEPS;

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// One step of both directions.  grid: 2 cell / 4 workgroups of four waves; wave = dir * cell + unit.
// xp0 / xp1: this step's [4 cell] row of the input projections of direction 0 / 1; t0 / t1: the row of hseq the
// direction writes; p0 / p1: the row that holds its previous output, or -1 at the first step (zeros).
__global__ void __launch_bounds__(TB) lstm_step_kernel(const float* __restrict__ wh, const float* __restrict__ xp0,
                                                       const float* __restrict__ xp1, float* hseq, float* __restrict__ c,
                                                       int cell, float forget_bias, int t0, int t1, int p0, int p1) {
  __shared__ __attribute__((aligned(16))) float hs[MAX_CELL];
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  const int dir = wave >= cell, unit = wave - dir * cell;          // (cell is a multiple of 4: a workgroup has one dir)
  const int t = dir ? t1 : t0, p = dir ? p1 : p0;
  const float* xp = dir ? xp1 : xp0;
  const size_t ld = (size_t)2 * cell;

  for (int k = 4 * threadIdx.x; k < cell; k += 4 * TB) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p >= 0) v = *reinterpret_cast<const float4*>(hseq + (size_t)p * ld + (size_t)dir * cell + k);
    *reinterpret_cast<float4*>(&hs[k]) = v;
  }
  __syncthreads();

  // (Asking for the first weights in front of the barrier was tried: 23.5 against 23.7 us a step, not kept.)
  const float* row = wh + ((size_t)dir * cell + unit) * 4 * cell;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (p >= 0) {                                                    // (the first step's product is zero: nothing to read)
#pragma unroll 2
    for (int k = 4 * lane; k < cell; k += 256) {
      float4 w[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) w[g] = *reinterpret_cast<const float4*>(row + (size_t)g * cell + k);
      const float4 h = *reinterpret_cast<const float4*>(&hs[k]);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        acc[g] = fmaf(w[g].x, h.x, acc[g]);
        acc[g] = fmaf(w[g].y, h.y, acc[g]);
        acc[g] = fmaf(w[g].z, h.z, acc[g]);
        acc[g] = fmaf(w[g].w, h.w, acc[g]);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = wave_sum(acc[g]);
  if (lane == 0) {
    const float zi = acc[0] + xp[unit], zj = acc[1] + xp[cell + unit];
    const float zf = acc[2] + xp[2 * cell + unit], zo = acc[3] + xp[3 * cell + unit];
    const float cn = c[dir * cell + unit] * sigmoidf(zf + forget_bias) + sigmoidf(zi) * tanhf(zj);
    c[dir * cell + unit] = cn;
    hseq[(size_t)t * ld + (size_t)dir * cell + unit] = tanhf(cn) * sigmoidf(zo);
  }
}

// dst [rows, dst_cols] = src [rows, src_cols] cut or zero-padded on the right
__global__ void __launch_bounds__(TB) copy_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows,
                                                       int src_cols, int dst_cols) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)rows * dst_cols) return;
  const size_t r = i / dst_cols;
  const int cc = (int)(i - r * dst_cols);
  dst[i] = cc < src_cols ? src[r * src_cols + cc] : 0.f;
}

int copy_cols(const float* src, float* dst, int rows, int src_cols, int dst_cols, hipStream_t st) {
  copy_cols_kernel<<<(unsigned)div_up((size_t)rows * dst_cols, (size_t)TB), TB, 0, st>>>(src, dst, rows, src_cols, dst_cols);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int lstm_step(const instag_deepspeech_weights* w, const float* xp0, const float* xp1, float* hseq, float* c, int S, int s,
              hipStream_t st) {
  const int t0 = s, t1 = S - 1 - s;
  lstm_step_kernel<<<(unsigned)(2 * w->cell / (TB / 64)), TB, 0, st>>>(w->wh, xp0, xp1, hseq, c, w->cell, w->forget_bias, t0,
                                                                    t1, s ? t0 - 1 : -1, s ? t1 + 1 : -1);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

const char* cell_error(const instag_deepspeech_weights* w) {
  if (!w) return "NULL weights";
  if (w->cell < 256 || w->cell % 256 || w->cell > MAX_CELL)
    return "cell must be a multiple of 256 in [256, INSTAG_DEEPSPEECH_MAX_CELL]";
  return nullptr;
}

const char* shape_error(const instag_deepspeech_weights* w) {
  if (const char* e = cell_error(w)) return e;
  if (w->n_in < 1 || w->n_in > 4096) return "n_in must be in [1, 4096]";
  if (w->hidden < 32 || w->hidden % 32 || w->hidden > 4096) return "hidden must be a multiple of 32 in [32, 4096]";
  if (w->n_out < 1 || w->n_out > 1024) return "n_out must be in [1, 1024]";
  if (!(w->clip > 0.f)) return "clip must be positive";
  return nullptr;
}

struct Plan {
  int S, R, k1, n6;                                       // steps, steps of a block, padded n_in and n_out
  size_t c, hseq, xpad, ha, hb, xp, total;                // offsets in floats
};

bool make_plan(const instag_deepspeech_weights* w, int S, int max_rows, Plan* p) {
  if (S < 1 || S > MAX_STEPS || max_rows < 1) return false;
  p->S = S;
  p->R = std::min(S, max_rows);
  p->k1 = (int)align_up((size_t)w->n_in, 32);
  p->n6 = (int)align_up((size_t)w->n_out, 4);
  const size_t rows = p->R == S ? (size_t)S : (size_t)2 * p->R, H = w->hidden;
  Arena a;
  p->c = a.take((size_t)2 * w->cell);
  p->hseq = a.take((size_t)S * 2 * w->cell);
  p->xpad = a.take(rows * p->k1);
  p->ha = a.take(rows * H);                                // h1, h3; behind the recurrence h5
  p->hb = a.take(rows * std::max(H, (size_t)p->n6));       // h2; behind the recurrence the padded logits
  p->xp = a.take((size_t)p->R * 8 * w->cell);
  p->total = a.off;
  return true;
}

constexpr const char* PLAN_ERROR = ": steps in [1, INSTAG_DEEPSPEECH_MAX_STEPS] and max_rows >= 1";

int dense(const float* a, const float* wt, const float* bias, float* d, int M, int K, int N, float clip, int tile,
          hipStream_t st) {
  GemmArgs g{};
  g.a = a; g.w = wt; g.bias = bias; g.d = d;
  g.M = M; g.rows = M; g.N = N; g.K = K; g.groups = 1; g.lda = K; g.ldd = N; g.clip = clip; g.blocked = 1;
  return launch_gemm(g, st, tile);
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_deepspeech_workspace_bytes(const instag_deepspeech_weights* w, int32_t steps, int32_t max_rows) {
  if (const char* e = shape_error(w)) {
    set_error(std::string("deepspeech_workspace_bytes: ") + e);
    return 0;
  }
  Plan p;
  if (!make_plan(w, steps, max_rows, &p)) {
    set_error(std::string("deepspeech_workspace_bytes") + PLAN_ERROR);
    return 0;
  }
  return p.total * sizeof(float);
}

size_t instag_deepspeech_taps_floats(const instag_deepspeech_weights* w, int32_t steps) {
  if (const char* e = shape_error(w)) {
    set_error(std::string("deepspeech_taps_floats: ") + e);
    return 0;
  }
  if (steps < 1 || steps > MAX_STEPS) {
    set_error(std::string("deepspeech_taps_floats") + PLAN_ERROR);
    return 0;
  }
  return (size_t)steps * ((size_t)4 * w->hidden + (size_t)2 * w->cell);
}

int instag_deepspeech_forward(const instag_deepspeech_weights* w, const float* x, int32_t steps, int32_t max_rows,
                              float* logits, void* workspace, size_t workspace_bytes, int32_t tile, float* taps,
                              instag_stream_t stream) {
  if (const char* e = shape_error(w)) {
    set_error(std::string("deepspeech_forward: ") + e);
    return INSTAG_E_ARG;
  }
  INSTAG_REQUIRE(x && logits && workspace, "deepspeech_forward: NULL tensor");
  INSTAG_REQUIRE(tile >= 0 && tile <= 3, "deepspeech_forward: tile must be 0..3");
  Plan p;
  INSTAG_REQUIRE(make_plan(w, steps, max_rows, &p), std::string("deepspeech_forward") + PLAN_ERROR);
  INSTAG_REQUIRE(w->w1 && w->b1 && w->w2 && w->b2 && w->w3 && w->b3 && w->wx && w->bx && w->wh && w->w5 && w->b5 && w->w6 &&
                     w->b6, "deepspeech_forward: NULL weight");
  INSTAG_REQUIRE(((uintptr_t)w->wh | (uintptr_t)workspace) % 16 == 0, "deepspeech_forward: wh and the workspace are 16-byte aligned");
  if (workspace_bytes < p.total * sizeof(float)) {
    set_error("deepspeech_forward: workspace smaller than instag_deepspeech_workspace_bytes(w, steps, max_rows)");
    return INSTAG_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int S = p.S, R = p.R, H = w->hidden, C4 = 4 * w->cell, C2 = 2 * w->cell;
  float *c = ws + p.c, *hseq = ws + p.hseq, *xpad = ws + p.xpad, *ha = ws + p.ha, *hb = ws + p.hb, *xp = ws + p.xp;
  float* tap[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};           // h1, h2, h3, lstm, h5
  if (taps) {
    tap[0] = taps;
    tap[1] = tap[0] + (size_t)S * H;
    tap[2] = tap[1] + (size_t)S * H;
    tap[3] = tap[2] + (size_t)S * H;
    tap[4] = tap[3] + (size_t)S * C2;
  }
  auto copy_tap = [&](float* dst, const float* src, size_t row, size_t rows, size_t cols) -> int {
    if (dst) INSTAG_CHECK_HIP(hipMemcpyAsync(dst + row * cols, src, rows * cols * sizeof(float), hipMemcpyDeviceToDevice, st));
    return INSTAG_OK;
  };

  INSTAG_CHECK_HIP(hipMemsetAsync(c, 0, (size_t)2 * w->cell * sizeof(float), st));
  const bool whole = R == S;
  for (int s0 = 0; s0 < S; s0 += R) {
    const int n = std::min(R, S - s0), s1 = s0 + n;
    const int rows = whole ? n : 2 * n;
    // the block's rows: [s0, s1), and behind them their mirror image [S - s1, S - s0) unless the block is the sequence
    INSTAG_TRY(copy_cols(x + (size_t)s0 * w->n_in, xpad, n, w->n_in, p.k1, st));
    if (!whole) INSTAG_TRY(copy_cols(x + (size_t)(S - s1) * w->n_in, xpad + (size_t)n * p.k1, n, w->n_in, p.k1, st));
    INSTAG_TRY(dense(xpad, w->w1, w->b1, ha, rows, p.k1, H, w->clip, tile, st));
    INSTAG_TRY(copy_tap(tap[0], ha, s0, n, H));
    INSTAG_TRY(dense(ha, w->w2, w->b2, hb, rows, H, H, w->clip, tile, st));
    INSTAG_TRY(copy_tap(tap[1], hb, s0, n, H));
    INSTAG_TRY(dense(hb, w->w3, w->b3, ha, rows, H, H, w->clip, tile, st));
    INSTAG_TRY(copy_tap(tap[2], ha, s0, n, H));
    {
      GemmArgs g{};                                          // xp[j][dir] = h3[dir's row j] wx[dir] + bx[dir]
      g.a = ha; g.w = w->wx; g.bias = w->bx; g.d = xp;
      g.M = n; g.rows = n; g.N = C4; g.K = H; g.groups = 2;
      g.a_group = whole ? 0 : (int64_t)n * H; g.lda = H; g.ldd = 2 * C4; g.blocked = 1;
      INSTAG_TRY(launch_gemm(g, st, tile));
    }
    // step s: forward row s is the block's row s - s0; backward row S - 1 - s is the mirror image's row s1 - 1 - s
    for (int s = s0; s < s1; ++s)
      INSTAG_TRY(lstm_step(w, xp + (size_t)(s - s0) * 2 * C4, xp + (size_t)(s1 - 1 - s) * 2 * C4 + C4, hseq, c, S, s, st));
  }
  INSTAG_TRY(copy_tap(tap[3], hseq, 0, S, C2));
  // layers 5 and 6 in blocks of the rows the buffers hold
  const int RT = whole ? S : 2 * R;
  for (int r0 = 0; r0 < S; r0 += RT) {
    const int n = std::min(RT, S - r0);
    INSTAG_TRY(dense(hseq + (size_t)r0 * C2, w->w5, w->b5, ha, n, C2, H, w->clip, tile, st));
    INSTAG_TRY(copy_tap(tap[4], ha, r0, n, H));
    INSTAG_TRY(dense(ha, w->w6, w->b6, hb, n, H, p.n6, 0.f, tile, st));
    INSTAG_TRY(copy_cols(hb, logits + (size_t)r0 * w->n_out, n, p.n6, w->n_out, st));
  }
  return INSTAG_OK;
}

int instag_deepspeech_lstm(const instag_deepspeech_weights* w, const float* xp, float* hseq, float* c, int32_t steps,
                           instag_stream_t stream) {
  if (const char* e = cell_error(w)) {
    set_error(std::string("deepspeech_lstm: ") + e);
    return INSTAG_E_ARG;
  }
  INSTAG_REQUIRE(xp && hseq && c && w->wh, "deepspeech_lstm: NULL tensor");
  INSTAG_REQUIRE(((uintptr_t)w->wh | (uintptr_t)hseq) % 16 == 0, "deepspeech_lstm: wh and hseq are 16-byte aligned");
  INSTAG_REQUIRE(steps >= 1 && steps <= MAX_STEPS, "deepspeech_lstm: steps in [1, INSTAG_DEEPSPEECH_MAX_STEPS]");
  hipStream_t st = (hipStream_t)stream;
  const size_t C4 = (size_t)4 * w->cell;
  INSTAG_CHECK_HIP(hipMemsetAsync(c, 0, (size_t)2 * w->cell * sizeof(float), st));
  for (int s = 0; s < steps; ++s)
    INSTAG_TRY(lstm_step(w, xp + (size_t)s * 2 * C4, xp + (size_t)(steps - 1 - s) * 2 * C4 + C4, hseq, c, steps, s, st));
  return INSTAG_OK;
}

}  // extern "C"
