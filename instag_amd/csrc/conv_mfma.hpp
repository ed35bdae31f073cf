// The convolution of the pretrained networks (parsing.hip, teeth.hip, through conv_net.hpp) and of the AudioEncoder's
// layers 1..10 (ave_encoder.hip): an implicit GEMM on the f32-input MFMA in the tile scheme of mfma_tile.hpp, and its
// launchers.
//
// D[cout][m] with m = (frame, oy, ox) tiled jointly and k = (cin, ky, kx) gathered from NCHW activations; four waves of
// one or two accumulators of 32 x 32 each; blocked summation (mfma_tile.hpp); the per-channel scale and shift
// (BatchNorm folded, or (1, bias)), the residual read and the ReLU are applied to the accumulator registers.  The tile
// is chosen per launch to fill the chip and does not enter the arithmetic.
//
// EXT (landmarks.hip, the pre-activation blocks of FAN) adds, to the plain source only: a per-input-channel
// max(v pre_scale + pre_shift, 0) on the taps inside the image (the padding stays zero after it); an output written as a
// channel slice of a wider tensor with the residual read from the same slice, a second residual at half resolution and
// a contiguous copy of the value in front of the residuals; and a K that is no multiple of 32, the rows past it zero.
// Every kernel without EXT is the code it was: the options are behind `if constexpr`.
//
// Everything sits in an anonymous namespace: each file that includes this header compiles its own copy of the kernels
// it launches, under its own flags.
#pragma once
#include "mfma_tile.hpp"

namespace instag {
namespace {

constexpr int STEM_K = 147, STEM_K_PADDED = 160;     // the 7 x 7 stem of the parser
constexpr int STEM3_K = 27;                           // a 3 x 3 stem on uint8 frames: K = 27 padded to one tile of 32

// where the gathered operand comes from
enum ConvSource {
  SRC_GATHER = 0,     // fp32 activations through the general gather (two sources, nearest upsample, attention)
  SRC_PLAIN = 1,      // one fp32 source, nothing folded: a bit mask of the taps inside the image, one base offset
  SRC_U8 = 2,         // uint8 HWC frames through a normalisation table in LDS (KS == 7 always reads frames)
};

// ---- convolution as implicit GEMM --------------------------------------------------------------------------------------
struct ConvArgs {
  const float* in;        // [B, c_split, hi >> up, wi >> up]
  const float* in2;       // channels c_split .. cin - 1: [B, cin - c_split, hi >> up, wi >> up]; NULL: c_split == cin
  const uint8_t* frames;  // the stem: [B, hi, wi, 3]
  const float* mul;       // [B, cin]: the value becomes v * mul + (v | add_bc | add_sp); NULL: v
  const float* add_bc;    // [B, cin]
  const float* add_sp;    // [B, cin, hi >> up, wi >> up]
  const float* wt;        // [K][cout]
  const float* scale;     // [cout]
  const float* shift;
  const float* res;       // [B, cout, ho >> res_up, wo >> res_up] added before the ReLU, or NULL
  float* out;             // [B, cout, ho, wo]
  int B, cin, c_split, cout, hi, wi, ho, wo, stride_h, stride_w, up, self_add, relu;
  int res_up;             // 1: the residual is read at half resolution, res[c][oy >> 1][ox >> 1]
  float mean[3], stdev[3];  // SRC_U8 with KS == 3: the frame enters as (u - mean) / stdev
  int unit_table;         // KS == 7: the frame enters as u / 255, not through the parser's mean and deviation
  // read by the EXT kernels only
  const float* pre_scale;  // [cin]: a tap inside the image enters as max(v pre_scale + pre_shift, 0); NULL: v
  const float* pre_shift;
  const float* res2;      // a second residual at half resolution, [B, out_ch, ho / 2, wo / 2], added behind res, or NULL
  float* raw;             // [B, cout, ho, wo]: scale * conv + shift in front of the residuals and the ReLU, or NULL
  int out_ch, out_off;    // out, res and res2 have out_ch channels and this launch's are out_off ..; out_ch 0: cout, 0
};

// KS: 1, 3 (pad KS / 2) or 7 (the parser's stem).  32 WR output channels x 32 (4 / WR) WN positions per workgroup: four
// waves as WR x 4 / WR, each with WN accumulators of 32 x 32.  WR = 1 is for cout = 32, where 64 rows would idle half
// the MFMAs.
template <int KS, int WR, int WN, int SRC, bool EXT = false>
__global__ void __launch_bounds__(TB) conv_kernel(ConvArgs a) {
  constexpr bool PLAIN = SRC == SRC_PLAIN;
  static_assert(!EXT || PLAIN, "the extensions are the plain source's");
  constexpr bool STEM3 = KS == 3 && SRC == SRC_U8;
  static_assert(SRC != SRC_U8 || KS == 3 || KS == 7, "a stem is 3 x 3 or 7 x 7");
  static_assert(WR == 1 || WR == 2, "four waves as 1 x 4 or 2 x 2");
  constexpr int WC = 4 / WR, BM = 32 * WR, BN = 32 * WC * WN;
  constexpr int NA = BK * BM / TB, NB = BK * BN / TB;          // elements a thread stages per K tile
  constexpr int RA = TB / BM, RB = TB / BN;                    // K rows one pass of the workgroup covers
  constexpr int PAD = KS / 2;
  __shared__ float As[BK][BM];
  __shared__ float Bs[BK][BN];
  __shared__ float lut[(KS == 7 || STEM3) ? 3 * 256 : 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave / WC, wc = wave % WC;
  if constexpr (KS == 7) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdev[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int c = 0; c < 3; ++c)
      lut[c * 256 + t] = a.unit_table ? (float)t / 255.f : ((float)t / 255.f - mean[c]) / stdev[c];   // TB == 256
  } else if constexpr (STEM3) {
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c * 256 + t] = ((float)t - a.mean[c]) / a.stdev[c];       // TB == 256
  }
  const int HWo = a.ho * a.wo;
  const int N = a.B * HWo;
  const int n0 = blockIdx.x * BN, c0 = blockIdx.y * BM;
  const int ta = t % BM, ka = t / BM;
  const int tb = t % BN, kb = t / BN;
  // EXT: BN is a multiple of the wave, so a wave's lanes share kb; said to the compiler, the K index, its channel and tap
  // and the pre-activation's scale and shift become scalar work
  static_assert(!EXT || BN % 64 == 0, "a wave gathers one K row");
  const int kg = EXT ? __builtin_amdgcn_readfirstlane(kb) : kb;
  const int hs = a.hi >> a.up, ws = a.wi >> a.up;
  const int c2 = a.cin - a.c_split;

  // this thread's column of the gathered operand: one output position of one frame
  const int ng = n0 + tb;
  const bool nv = ng < N;
  int img = 0, oy = 0, ox = 0;
  if (nv) {
    img = ng / HWo;
    const int pos = ng - img * HWo;
    oy = pos / a.wo;
    ox = pos - oy * a.wo;
  }
  const int iy0 = oy * a.stride_h - PAD, ix0 = ox * a.stride_w - PAD;
  const bool wv = c0 + ta < a.cout;
  // PLAIN (one source, no upsample, no attention): bit r of `inside` = tap r = ky KS + kx lies inside the image
  uint32_t inside = 0;
  const int plane = a.hi * a.wi;
  int64_t off0 = 0;
  if constexpr (PLAIN) {
    static_assert(KS * KS <= 32, "one bit per tap");
    if (nv)
#pragma unroll
      for (int r = 0; r < KS * KS; ++r) {
        const int iy = iy0 + r / KS, ix = ix0 + r % KS;
        if (iy >= 0 && iy < a.hi && ix >= 0 && ix < a.wi) inside |= 1u << r;
      }
    off0 = (int64_t)img * a.cin * plane + iy0 * a.wi + ix0;
  }

  auto gather = [&](int k) -> float {
    const int ci = k / (KS * KS);
    const int r = k - ci * (KS * KS);
    const int ky = r / KS, kx = r - ky * KS;
    if constexpr (PLAIN) {
      if constexpr (EXT) {
        if (ci >= a.cin) return 0.f;                                         // the zero rows behind a K that is no multiple of 32
      }
      if (!((inside >> r) & 1u)) return 0.f;
      const float v = a.in[off0 + (ci * plane + ky * a.wi + kx)];
      if constexpr (EXT) {
        if (a.pre_scale) return fmaxf(fmaf(v, a.pre_scale[ci], a.pre_shift[ci]), 0.f);
      }
      return v;
    }
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (!nv || iy < 0 || iy >= a.hi || ix < 0 || ix >= a.wi) return 0.f;
    if constexpr (KS == 7) {
      if (k >= STEM_K) return 0.f;
      return lut[ci * 256 + a.frames[((size_t)(img * a.hi + iy) * a.wi + ix) * 3 + ci]];
    }
    if constexpr (STEM3) {
      if (k >= STEM3_K) return 0.f;
      return lut[ci * 256 + a.frames[((size_t)(img * a.hi + iy) * a.wi + ix) * 3 + ci]];
    }
    const int sy = iy >> a.up, sx = ix >> a.up;
    size_t idx;
    const float* src;
    if (ci < a.c_split) {
      src = a.in;
      idx = ((size_t)(img * a.c_split + ci) * hs + sy) * ws + sx;
    } else {
      src = a.in2;
      idx = ((size_t)(img * c2 + ci - a.c_split) * hs + sy) * ws + sx;
    }
    float v = src[idx];
    if (a.mul) {
      const int bc = img * a.cin + ci;
      const float other = a.self_add ? v : a.add_bc ? a.add_bc[bc] : a.add_sp[idx];
      v = v * a.mul[bc] + other;
    }
    return v;
  };

  float ra[NA], rb[NB];
  auto load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[i] = wv ? a.wt[(size_t)(kt * BK + ka + RA * i) * a.cout + c0 + ta] : 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) rb[i] = gather(kt * BK + kg + RB * i);
  };

  f32x16 acc[WN];
#pragma unroll
  for (int j = 0; j < WN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  // cin is a multiple of 32 everywhere but in the stems, whose K is padded with zero rows
  const int nk = KS == 7 ? STEM_K_PADDED / BK : STEM3 ? 1 : (a.cin * KS * KS + (EXT ? BK - 1 : 0)) / BK;
  if (KS == 7 || STEM3) __syncthreads();                                    // the table
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NA; ++i) As[ka + RA * i][ta] = ra[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) Bs[kb + RB * i][tb] = rb[i];
    __syncthreads();
    if (kt + 1 < nk) load(kt + 1);
    // mfma_tile.hpp's blocked K tile and, below, its row formula, written out: through mfma_k_tile and mfma_row the
    // compiler pairs the LDS reads differently and takes two registers fewer, and the plain 3 x 3 64 x 64 kernel was
    // measured 2.3 % slower (the parser's ten such layers: 1,570 us against 1,535 us)
    f32x16 part[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) part[j][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const float av = As[kk * 2 + (lane >> 5)][wr * 32 + (lane & 31)];
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        const float bv = Bs[kk * 2 + (lane >> 5)][(wc * WN + j) * 32 + (lane & 31)];
        part[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, part[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < WN; ++j) acc[j] += part[j];
  }

  // D: column = output position, row = output channel
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int nc = n0 + (wc * WN + j) * 32 + (lane & 31);
    if (nc >= N) continue;
    const int oimg = nc / HWo, opos = nc - oimg * HWo;
    const size_t obase = (size_t)oimg * a.cout * HWo + opos;
    if constexpr (EXT) {
      const int och = a.out_ch ? a.out_ch : a.cout;
      const size_t sbase = ((size_t)oimg * och + a.out_off) * HWo + opos;     // the slice's first channel at this position
      const int y = opos / a.wo, x = opos - y * a.wo, hplane = HWo >> 2;
      const size_t hbase = ((size_t)oimg * och + a.out_off) * hplane + (size_t)(y >> 1) * (a.wo >> 1) + (x >> 1);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = c0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (co >= a.cout) continue;
        float v = fmaf(acc[j][r], a.scale[co], a.shift[co]);
        if (a.raw) a.raw[obase + (size_t)co * HWo] = v;
        const size_t o = sbase + (size_t)co * HWo;
        if (a.res) v += a.res[o];
        if (a.res2) v += a.res2[hbase + (size_t)co * hplane];
        a.out[o] = a.relu ? fmaxf(v, 0.f) : v;
      }
      continue;
    }
    // the half-resolution residual (ho and wo even): plane size HWo / 4, position (oy >> 1, ox >> 1)
    size_t rbase = 0;
    int rplane = 0;
    if (a.res_up) {
      const int y = opos / a.wo, x = opos - y * a.wo;
      rplane = HWo >> 2;
      rbase = (size_t)oimg * a.cout * rplane + (size_t)(y >> 1) * (a.wo >> 1) + (x >> 1);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = c0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (co >= a.cout) continue;
      const size_t o = obase + (size_t)co * HWo;
      float v = fmaf(acc[j][r], a.scale[co], a.shift[co]);
      if (a.res) v += a.res_up ? a.res[rbase + (size_t)co * rplane] : a.res[o];
      a.out[o] = a.relu ? fmaxf(v, 0.f) : v;
    }
  }
}

template <int KS, int WR, int WN, int SRC, bool EXT = false>
int launch_conv_kernel(const ConvArgs& a, hipStream_t st) {
  const int N = a.B * a.ho * a.wo;
  const dim3 grid((unsigned)div_up(N, 32 * (4 / WR) * WN), (unsigned)div_up(a.cout, 32 * WR));
  conv_kernel<KS, WR, WN, SRC, EXT><<<grid, TB, 0, st>>>(a);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

// the 64-row tile, the source read off the arguments
template <int KS, int WN>
int launch_conv_tile(const ConvArgs& a, hipStream_t st) {
  if constexpr (KS == 7) {
    return launch_conv_kernel<KS, 2, WN, SRC_U8>(a, st);
  } else {
    if constexpr (KS == 3) {
      if (a.frames) return launch_conv_kernel<KS, 2, WN, SRC_U8>(a, st);
    }
    if (!a.in2 && !a.mul && !a.up) return launch_conv_kernel<KS, 2, WN, SRC_PLAIN>(a, st);
    return launch_conv_kernel<KS, 2, WN, SRC_GATHER>(a, st);
  }
}

// the largest tile that still gives every CU two workgroups (the arithmetic does not depend on the choice)
template <int KS>
int launch_conv(const ConvArgs& a, hipStream_t st) {
  const int N = a.B * a.ho * a.wo;
  if (div_up(N, 128) * div_up(a.cout, 64) >= MIN_BLOCKS) return launch_conv_tile<KS, 2>(a, st);
  return launch_conv_tile<KS, 1>(a, st);
}

// the EXT kernel (KS 1 or 3, stride 1 or 2, the plain source): the 32-row tile for cout = 32, else the 64-row one, and
// the wide tile where it still gives every CU two workgroups
template <int KS>
int launch_conv_ext(const ConvArgs& a, hipStream_t st) {
  const int N = a.B * a.ho * a.wo;
  if (a.cout <= 32) {
    if (div_up(N, 256) >= MIN_BLOCKS) return launch_conv_kernel<KS, 1, 2, SRC_PLAIN, true>(a, st);
    return launch_conv_kernel<KS, 1, 1, SRC_PLAIN, true>(a, st);
  }
  if (div_up(N, 128) * div_up(a.cout, 64) >= MIN_BLOCKS) return launch_conv_kernel<KS, 2, 2, SRC_PLAIN, true>(a, st);
  return launch_conv_kernel<KS, 2, 1, SRC_PLAIN, true>(a, st);
}

}  // namespace
}  // namespace instag
