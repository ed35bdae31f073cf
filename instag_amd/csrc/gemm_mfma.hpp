// A row-major GEMM on the f32-input MFMA (v_mfma_f32_32x32x2_f32) for the transformer of wav2vec.hip:
//
//   D[b][t][g N + n] = epilogue(sum_k A[b][g][t][k] W[g][k][n] + bias[g N + n])
//
// A row is the K contiguous floats at a + b a_batch + g a_group + t lda: rows may overlap in memory, which is how a
// convolution over time-major activations [T, C] (kernel k, stride s: lda = s C, K = k C) is this GEMM with nothing
// gathered.  W is [K][N] per group, n contiguous.  The rows of all batches are tiled jointly (m = b rows + t), the
// groups ride on blockIdx.z.  The epilogue works on the accumulator registers: + bias, erf-GELU, + residual (read at D's
// index; D may be the residual itself).  clip > 0 asks for the clipped ReLU min(max(v, 0), clip) of deepspeech.hip behind
// the bias; 0, what GemmArgs{} gives, leaves it out.  blocked (0 likewise) sums every K tile from zero and adds the tiles
// in order: with K = 4096 in one chain layer 5 of deepspeech.hip sat 5.5 x the fp32 CPU statement's own error from the
// fp64 values, and that network's time is its recurrence, not its GEMMs.
//
// The tile scheme is that of mfma_tile.hpp, in its in-place form.  As in conv_mfma.hpp the tile is chosen per launch to
// fill the chip and does not enter the arithmetic: an output element is one k-ordered FMA chain over all of K from 0
// (the MFMA accumulates in place, which also halves the accumulator registers against a partial sum per K tile),
// whatever tile it sat in.  K is a multiple of 32, N and lda multiples of 4 (the operands are staged with 16-byte
// loads); M and N may end inside a tile.
#pragma once
#include "mfma_tile.hpp"

namespace instag {
namespace {

struct GemmArgs {
  const float* a;
  const float* w;      // [groups][K][N]
  const float* bias;   // [groups * N]
  const float* res;    // indexed as d, or NULL
  float* d;
  int M, rows;         // rows in all (batches * rows) and per batch
  int N, K, groups;
  int64_t a_batch, a_group;
  int lda;
  int64_t d_batch;
  int ldd;
  int gelu;
  float clip;          // > 0: min(relu(.), clip) behind the bias
  int blocked;         // the blocked summation of mfma_tile.hpp in place of the one chain over K
};

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

// four waves as 2 x 2, each with WM x WN accumulators of 32 x 32: a workgroup owns 64 WM rows x 64 WN columns
template <int WM, int WN, bool BLOCKED = false>
__global__ void __launch_bounds__(TB) gemm_kernel(GemmArgs g) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int LDA_S = BM + 4;                       // the transposed A tile: k-major, padded against bank conflicts
  constexpr int NA = BM * BK / 4 / TB;                // float4 a thread stages per K tile
  constexpr int NB = BK * BN / 4 / TB;
  constexpr int BROWS = TB / (BN / 4);                // K rows of W one pass of the workgroup covers
  __shared__ float As[BK][LDA_S];
  __shared__ __attribute__((aligned(16))) float Bs[BK][BN];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, grp = blockIdx.z;
  const float* wt = g.w + (size_t)grp * g.K * g.N;

  // this thread's rows of A (k contiguous: 8 threads x float4 cover a K tile of one row)
  const int ar = t >> 3, ak = (t & 7) * 4;
  const float* arow[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = m0 + ar + 32 * i;
    arow[i] = nullptr;
    if (m < g.M) {
      const int b = m / g.rows, tt = m - b * g.rows;
      arow[i] = g.a + (int64_t)b * g.a_batch + (int64_t)grp * g.a_group + (int64_t)tt * g.lda + ak;
    }
  }
  const int bn = (t % (BN / 4)) * 4, bk = t / (BN / 4);
  const bool bv_ok = n0 + bn < g.N;                   // N is a multiple of 4: a float4 is inside or outside as a whole

  float4 ra[NA], rb[NB];
  auto load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
      ra[i] = arow[i] ? *reinterpret_cast<const float4*>(arow[i] + kt * BK) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      rb[i] = bv_ok ? *reinterpret_cast<const float4*>(wt + (size_t)(kt * BK + bk + BROWS * i) * g.N + n0 + bn)
                    : make_float4(0.f, 0.f, 0.f, 0.f);
  };

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = g.K / BK;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      As[ak + 0][ar + 32 * i] = ra[i].x;
      As[ak + 1][ar + 32 * i] = ra[i].y;
      As[ak + 2][ar + 32 * i] = ra[i].z;
      As[ak + 3][ar + 32 * i] = ra[i].w;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) *reinterpret_cast<float4*>(&Bs[bk + BROWS * i][bn]) = rb[i];
    __syncthreads();
    if (kt + 1 < nk) load(kt + 1);
    mfma_k_tile<WM, WN, BLOCKED>(As, Bs, wr * WM * 32, wc * WN * 32, lane, acc);
  }

  // D: column = n, row = m
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int n = n0 + (wc * WN + j) * 32 + (lane & 31);
    if (n >= g.N) continue;
    const int col = grp * g.N + n;
    const float bias = g.bias[col];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mfma_row(m0 + (wr * WM + i) * 32, r, lane);
        if (m >= g.M) continue;
        const int b = m / g.rows, tt = m - b * g.rows;
        const int64_t o = (int64_t)b * g.d_batch + (int64_t)tt * g.ldd + col;
        float v = acc[i][j][r] + bias;
        if (g.gelu) v = gelu_erf(v);
        if (g.clip > 0.f) v = fminf(fmaxf(v, 0.f), g.clip);
        if (g.res) v += g.res[o];
        g.d[o] = v;
      }
  }
}

template <int WM, int WN>
int launch_gemm_tile(const GemmArgs& g, hipStream_t st) {
  const dim3 grid((unsigned)div_up(g.M, 64 * WM), (unsigned)div_up(g.N, 64 * WN), (unsigned)g.groups);
  if (g.blocked)
    gemm_kernel<WM, WN, true><<<grid, TB, 0, st>>>(g);
  else
    gemm_kernel<WM, WN><<<grid, TB, 0, st>>>(g);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

inline bool gemm_ok(const GemmArgs& g) {
  return g.M >= 1 && g.rows >= 1 && g.M % g.rows == 0 && g.N >= 4 && g.N % 4 == 0 && g.K >= BK && g.K % BK == 0 &&
         g.lda % 4 == 0 && g.a_batch % 4 == 0 && g.a_group % 4 == 0 && g.groups >= 1 && g.groups <= 65535 &&
         div_up(g.N, 64) <= 65535;
}

// the largest tile that still gives every CU two workgroups (the arithmetic does not depend on the choice)
// tile: 0 = that choice, 1, 2, 3 = 64 x 64, 64 x 128, 128 x 128 (the tests hold them against each other bit for bit)
inline int launch_gemm(const GemmArgs& g, hipStream_t st, int tile = 0) {
  INSTAG_REQUIRE(gemm_ok(g), "gemm: K a multiple of 32, N, lda and the strides of A multiples of 4");
  auto blocks = [&](int wm, int wn) { return (int64_t)div_up(g.M, 64 * wm) * div_up(g.N, 64 * wn) * g.groups; };
  if (tile == 0) tile = blocks(2, 2) >= MIN_BLOCKS ? 3 : blocks(1, 2) >= MIN_BLOCKS ? 2 : 1;
  if (tile == 3) return launch_gemm_tile<2, 2>(g, st);
  if (tile == 2) return launch_gemm_tile<1, 2>(g, st);
  return launch_gemm_tile<1, 1>(g, st);
}

}  // namespace
}  // namespace instag
