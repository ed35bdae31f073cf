// What the kernels on the f32-input MFMA (v_mfma_f32_32x32x2_f32) share: lpips.hip, conv_mfma.hpp (parsing, teeth, the
// encoder's layers 1..10), gemm_mfma.hpp (wav2vec) and the encoder's tail.  Four waves per workgroup, K tiles of 32
// staged through two LDS tiles As[k][row] and Bs[k][column] with the next tile prefetched in registers, the epilogue on
// the accumulator registers.  The loop around a tile (sync, stage, sync, prefetch), the staging and the epilogue are
// each kernel's own; the MFMAs of one staged tile and the layout of their result are here.  (conv_mfma.hpp writes
// both out, for a measured reason given there; it takes the constants, the type and the rule below.)
//
// Blocked summation.  The MFMA is a k-ordered fp32 FMA chain.  The blocked form runs one chain of 32 terms from zero
// per K tile and adds the tiles in order.  One chain over the whole K (up to 4,800 terms in LPIPS) left the activations
// of its conv2..5 2.5 - 3x further from the fp64 values than the library convolutions are (1.1e-5 against 4e-6 at
// magnitudes of 7); the blocked form is at or below the library's error in every layer.  It matters where two pool
// inputs are within rounding of each other or a pre-activation is within rounding of zero: a backward pass then
// routes the gradient through another unit, an argmax picks another label.  The convolutions use it.  The GEMM of
// wav2vec accumulates in place (one chain over all of K: half the accumulator registers; its error is measured in
// DESIGN.md section 28).  Either way an output element's sum does not depend on the tile it sat in.
#pragma once
#include "common.hpp"

namespace instag {
namespace {

constexpr int TB = 256;
constexpr int BK = 32;
constexpr int MIN_BLOCKS = 512;    // two workgroups for each of the 256 CUs

using f32x16 = __attribute__((ext_vector_type(16))) float;

// The accumulator D of one 32 x 32 MFMA: lane holds column (lane & 31); its register r holds the row returned here, counted
// from row0, the tile's first row.  (row0 is added first so that the compiler folds r's constants into the addresses.)
__device__ __forceinline__ int mfma_row(int row0, int r, int lane) {
  return row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// One staged K tile: acc[i][j] += As[:, a0 + 32 i + 0..31]^T Bs[:, b0 + 32 j + 0..31], BK / 2 MFMAs per accumulator.
// BLOCKED: the tile's products are summed from zero and the partial sum is then added to acc (above).
template <int WM, int WN, bool BLOCKED, int LDA, int LDB>
__device__ __forceinline__ void mfma_k_tile(const float (&As)[BK][LDA], const float (&Bs)[BK][LDB], int a0, int b0,
                                            int lane, f32x16 (&acc)[WM][WN]) {
  f32x16 part[WM][WN];
  f32x16 (&sum)[WM][WN] = BLOCKED ? part : acc;
  if constexpr (BLOCKED) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < WN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[i][j][r] = 0.f;
  }
#pragma unroll
  for (int kk = 0; kk < BK / 2; ++kk) {
    const int k = kk * 2 + (lane >> 5);
    float av[WM], bv[WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) av[i] = As[k][a0 + i * 32 + (lane & 31)];
#pragma unroll
    for (int j = 0; j < WN; ++j) bv[j] = Bs[k][b0 + j * 32 + (lane & 31)];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < WN; ++j) sum[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], sum[i][j], 0, 0, 0);
  }
  if constexpr (BLOCKED) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < WN; ++j) acc[i][j] += part[i][j];
  }
}

}  // namespace
}  // namespace instag
