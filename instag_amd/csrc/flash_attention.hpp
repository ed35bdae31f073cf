// The streaming-softmax attention of hubert.hip (clips of up to 1024 rows) and sapiens.hip (3072 tokens a frame):
// ctx [B, T, H] = softmax(q k^T / 8) v per (segment, head of 64) of qkv [B, T, 3 H] (q | k | v).  The code depends on T
// through its loop bounds alone; each entry declares and checks a bound of its own.
//
// A (segment, head)'s scores are never stored (4 MB at 1000 rows, 36 MB at 3072): a
// workgroup owns 64 query rows and walks the keys in tiles of 64 with a running maximum m and sum l per row (the
// streaming softmax), rescaling l and the output on every tile.  Its four waves are 2 x 2: wave (wq, kh) owns the query
// rows 32 wq .. 32 wq + 31 and, of every tile, the keys 32 kh .. 32 kh + 31, with m, l and the output of its own keys;
// at the end the kh = 1 waves hand theirs over through LDS and the kh = 0 waves merge the two (first their own, then
// the other's) and store.  Four short waves per 64 rows instead of two long ones: a clip is a small problem (1024
// wave-sized pieces at B = 2), the kernel's time is one wave's, and a SIMD that holds two waves runs the softmax of one
// under the MFMAs of the other.  Both products are on v_mfma_f32_32x32x2_f32, transposed so that a lane owns ONE query
// row (mfma_tile.hpp: the accumulator's column):
//
//   S^T [key][query] = K Q^T    A = K from LDS (Kt[d][key]), B = Q^T: 32 registers, loaded once, pre-divided by 8;
//   O^T [d][query]   = V^T P^T  A = V^T from LDS (Vs[key][d]), B = P^T: the accumulator of S^T as it stands.
//
// The MFMA sums over its two k slots, lanes 0..31 feeding one and 32..63 the other, and the order of a sum's terms is
// ours to choose as long as A and B agree.  In S^T the slots take d = kk and kk + 32, so a lane's Q is 32 contiguous
// floats.  In O^T step r takes the keys whose scores the two half-waves hold in register r (mfma_row: (r & 3) +
// 8 (r >> 2), + 4 in the upper half), so P never moves between lanes.  A row's maximum is 16 fmaxf and one exchange
// with the other half-wave; its sum stays split over the two halves until the end; m, l and the rescale factor are
// per-lane scalars.  K and V tiles are shared by the four waves and staged through LDS with the next tile prefetched
// in registers: 35 KB whatever T is.
//
// Tails: keys at or beyond T are staged as zeros and their scores set to -inf before the maximum.  A wave skips a
// half tile that holds no key below T, so every half tile it works on has a finite maximum: m is finite from a wave's
// first half tile on, and exp2f(-inf) = 0 is the only special value that occurs -- in the first rescale, for masked
// keys, and in the merge for a kh = 1 wave that never saw a key (T <= 32), whose share is then 0 x 0.  The kh = 0 wave
// always has key 0.  Query rows at or beyond T compute on zeros and are not stored.  p = exp2f((s - m) log2 e): the
// subtraction is exact where it matters (s near m), the exponent is the library's.
// No atomics; a row's sums have one fixed order that depends on neither the batch nor the segment's place in it.
#pragma once
#include "transformer.hpp"

namespace instag {
namespace {

constexpr int QB = 64, KB = 64;                // query rows of a workgroup, keys of a tile
constexpr int LDK = KB + 1;                    // Kt[d][key]: the transposed staging writes of a wave fall on distinct banks
constexpr int LDV = HEAD_DIM + 8;              // Vs[key][d]: rows of 16-byte pieces; keys 4 apart are 32 banks apart
constexpr float LOG2E = 1.4426950408889634f;

__global__ void __launch_bounds__(TB) flash_attention_kernel(const float* __restrict__ qkv, float* __restrict__ ctx, int T,
                                                             int H) {
  __shared__ float Kt[HEAD_DIM][LDK];
  __shared__ __attribute__((aligned(16))) float Vs[KB][LDV];
  const int t = threadIdx.x, lane = t & 63, col = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), wq = wave & 1, kh = wave >> 1;
  const int head = blockIdx.y, b = blockIdx.z;
  const float* base = qkv + (size_t)b * T * 3 * H + head * HEAD_DIM;
  const int q = blockIdx.x * QB + wq * 32 + col;            // this lane's query row

  float qv[32];                                              // Q[q][32 hi + 0..31] / 8
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float4 v = q < T ? *reinterpret_cast<const float4*>(base + (size_t)q * 3 * H + 32 * hi + 4 * i)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    qv[4 * i + 0] = v.x * 0.125f;
    qv[4 * i + 1] = v.y * 0.125f;
    qv[4 * i + 2] = v.z * 0.125f;
    qv[4 * i + 3] = v.w * 0.125f;
  }

  // staging: thread t carries d4..d4 + 3 of the keys kr, kr + 16, kr + 32, kr + 48 of a tile
  const int d4 = (t & 15) * 4, kr = t >> 4;
  float4 rk[4], rv[4];
  auto load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = kt * KB + kr + 16 * i;
      const float* row = base + (size_t)key * 3 * H + d4;
      rk[i] = key < T ? *reinterpret_cast<const float4*>(row + H) : make_float4(0.f, 0.f, 0.f, 0.f);
      rv[i] = key < T ? *reinterpret_cast<const float4*>(row + 2 * H) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m = -INFINITY, l = 0.f;                              // l: this half-wave's share of the sum over the wave's keys

  const int nt = (T + KB - 1) / KB;
  load(0);
  for (int kt = 0; kt < nt; ++kt) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Kt[d4 + 0][kr + 16 * i] = rk[i].x;
      Kt[d4 + 1][kr + 16 * i] = rk[i].y;
      Kt[d4 + 2][kr + 16 * i] = rk[i].z;
      Kt[d4 + 3][kr + 16 * i] = rk[i].w;
      *reinterpret_cast<float4*>(&Vs[kr + 16 * i][d4]) = rv[i];
    }
    __syncthreads();
    if (kt + 1 < nt) load(kt + 1);
    const int k0 = kt * KB + 32 * kh;                        // this wave's keys of the tile: k0 .. k0 + 31
    if (k0 >= T) continue;                                   // (wave-uniform; only in the last tile)

    // S^T: s[r] = q . k / 8 for the key mfma_row(k0, r, lane)
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk)
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(Kt[kk + 32 * hi][32 * kh + col], qv[kk], s, 0, 0, 0);
    if (k0 + 32 > T) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (mfma_row(k0, r, lane) >= T) s[r] = -INFINITY;
    }
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);
    const float alpha = exp2f((m - m_new) * LOG2E);          // 0 on the wave's first half tile
    m = m_new;
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = exp2f((s[r] - m_new) * LOG2E);
      sum += s[r];
    }
    l = l * alpha + sum;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;

    // O^T += V^T P^T, the k slots of step r: the keys of register r in the two half-waves
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = mfma_row(32 * kh, r, lane);
      o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key][col], s[r], o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key][32 + col], s[r], o[1], 0, 0, 0);
    }
  }

  // the kh = 1 waves hand m, l and o over in the tiles' place: ml[wq][m | l][lane] in Kt, oo[wq][register][lane] in Vs
  __syncthreads();
  float* ml = &Kt[0][0] + wq * 128;
  float* oo = &Vs[0][0] + wq * 2048;
  static_assert(2 * 128 <= HEAD_DIM * LDK && 2 * 2048 <= KB * LDV, "the hand-over fits the tiles");
  if (kh == 1) {
    ml[lane] = m;
    ml[64 + lane] = l;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) oo[(16 * dt + r) * 64 + lane] = o[dt][r];
  }
  __syncthreads();
  if (kh == 1 || q >= T) return;
  // o[dt][r] is O[q][32 dt + mfma_row(0, r, lane)]: registers 4 g .. 4 g + 3 are four neighbours in d
  const float m1 = ml[lane], l1 = ml[64 + lane], mm = fmaxf(m, m1);
  const float f0 = exp2f((m - mm) * LOG2E), f1 = exp2f((m1 - mm) * LOG2E);
  const float lw = l * f0 + l1 * f1;
  const float inv = 1.f / (lw + __shfl_xor(lw, 32));
  float* dst = ctx + ((size_t)b * T + q) * H + head * HEAD_DIM;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float y[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int r = 4 * g + c;
        y[c] = (o[dt][r] * f0 + oo[(16 * dt + r) * 64 + lane] * f1) * inv;
      }
      *reinterpret_cast<float4*>(dst + 32 * dt + 8 * g + 4 * hi) = make_float4(y[0], y[1], y[2], y[3]);
    }
}

// ctx [B, T, H] = softmax(q k^T / 8) v per (segment, head) of qkv [B, T, 3 H]; the caller has checked the shape
int flash_attention(const float* qkv, float* ctx, int B, int T, int H, hipStream_t st) {
  flash_attention_kernel<<<dim3((unsigned)div_up(T, QB), (unsigned)(H / HEAD_DIM), (unsigned)B), TB, 0, st>>>(qkv, ctx, T, H);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag
