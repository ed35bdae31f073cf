// The convolution of the pretrained networks (parsing.hip, teeth.hip): an implicit GEMM on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32), the 3 x 3 max-pool behind their stems, what their entry points share on the host (ConvNet,
// frames_ok) and the per-pixel interpolation and argmax of their label kernels.
//
// D[cout][m] with m = (frame, oy, ox) tiled jointly and k = (cin, ky, kx) gathered from NCHW activations; four waves of
// one or two accumulators of 32 x 32 each; K tiles of 32 added in order; the per-channel scale and shift (BatchNorm
// folded, or (1, bias)), the residual read and the ReLU are applied to the accumulator registers.  The tile is chosen per
// launch to fill the chip and does not enter the arithmetic: an output element is one k-ordered FMA chain per K tile,
// the tiles summed in order, whatever tile it sat in.
//
// Everything sits in an anonymous namespace: each file that includes this header compiles its own copy of the kernels
// it launches, under its own flags.
#pragma once
#include "common.hpp"

namespace instag {
namespace {

constexpr int TB = 256;
constexpr int BK = 32;
constexpr int STEM_K = 147, STEM_K_PADDED = 160;     // the 7 x 7 stem of the parser
constexpr int STEM3_K = 27;                           // a 3 x 3 stem on uint8 frames: K = 27 padded to one tile of 32
constexpr int MIN_BLOCKS = 512;    // two workgroups for each of the 256 CUs

using f32x16 = __attribute__((ext_vector_type(16))) float;

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
  int B, cin, c_split, cout, hi, wi, ho, wo, stride, up, self_add, relu;
  int res_up;             // 1: the residual is read at half resolution, res[c][oy >> 1][ox >> 1]
  float mean[3], stdev[3];  // SRC_U8 with KS == 3: the frame enters as (u - mean) / stdev
};

// KS: 1, 3 (pad KS / 2) or 7 (the parser's stem).  64 output channels x 64 WN positions per workgroup, four waves as
// 2 x 2, each with WN accumulators of 32 x 32.
template <int KS, int WN, int SRC>
__global__ void __launch_bounds__(TB) conv_kernel(ConvArgs a) {
  constexpr bool PLAIN = SRC == SRC_PLAIN;
  constexpr bool STEM3 = KS == 3 && SRC == SRC_U8;
  static_assert(SRC != SRC_U8 || KS == 3 || KS == 7, "a stem is 3 x 3 or 7 x 7");
  constexpr int BM = 64, BN = 64 * WN;
  constexpr int NA = BK * BM / TB, NB = BK * BN / TB;          // elements a thread stages per K tile
  constexpr int RA = TB / BM, RB = TB / BN;                    // K rows one pass of the workgroup covers
  constexpr int PAD = KS / 2;
  __shared__ float As[BK][BM];
  __shared__ float Bs[BK][BN];
  __shared__ float lut[(KS == 7 || STEM3) ? 3 * 256 : 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  if constexpr (KS == 7) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdev[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c * 256 + t] = ((float)t / 255.f - mean[c]) / stdev[c];   // TB == 256
  } else if constexpr (STEM3) {
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c * 256 + t] = ((float)t - a.mean[c]) / a.stdev[c];       // TB == 256
  }
  const int HWo = a.ho * a.wo;
  const int N = a.B * HWo;
  const int n0 = blockIdx.x * BN, c0 = blockIdx.y * BM;
  const int ta = t % BM, ka = t / BM;
  const int tb = t % BN, kb = t / BN;
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
  const int iy0 = oy * a.stride - PAD, ix0 = ox * a.stride - PAD;
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
      if (!((inside >> r) & 1u)) return 0.f;
      return a.in[off0 + (ci * plane + ky * a.wi + kx)];
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
    for (int i = 0; i < NB; ++i) rb[i] = gather(kt * BK + kb + RB * i);
  };

  f32x16 acc[WN], part[WN];
#pragma unroll
  for (int j = 0; j < WN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  // cin is a multiple of 32 everywhere but in the stems, whose K is padded with zero rows
  const int nk = KS == 7 ? STEM_K_PADDED / BK : STEM3 ? 1 : a.cin * KS * KS / BK;
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

  // D: column (lane & 31) = output position, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = output channel
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int nc = n0 + (wc * WN + j) * 32 + (lane & 31);
    if (nc >= N) continue;
    const int oimg = nc / HWo, opos = nc - oimg * HWo;
    const size_t obase = (size_t)oimg * a.cout * HWo + opos;
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

template <int KS, int WN>
int launch_conv_tile(const ConvArgs& a, hipStream_t st) {
  const int N = a.B * a.ho * a.wo;
  const dim3 grid((unsigned)div_up(N, 64 * WN), (unsigned)div_up(a.cout, 64));
  if constexpr (KS == 3) {
    if (a.frames) {
      conv_kernel<KS, WN, SRC_U8><<<grid, TB, 0, st>>>(a);
      INSTAG_CHECK_LAUNCH();
      return INSTAG_OK;
    }
  }
  if (KS != 7 && !a.in2 && !a.mul && !a.up) {
    conv_kernel<KS, WN, (KS != 7 ? SRC_PLAIN : SRC_U8)><<<grid, TB, 0, st>>>(a);
  } else {
    conv_kernel<KS, WN, (KS != 7 ? SRC_GATHER : SRC_U8)><<<grid, TB, 0, st>>>(a);
  }
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

// the largest tile that still gives every CU two workgroups (the arithmetic does not depend on the choice)
template <int KS>
int launch_conv(const ConvArgs& a, hipStream_t st) {
  const int N = a.B * a.ho * a.wo;
  if (div_up(N, 128) * div_up(a.cout, 64) >= MIN_BLOCKS) return launch_conv_tile<KS, 2>(a, st);
  return launch_conv_tile<KS, 1>(a, st);
}

// ---- 3 x 3 max-pool, stride 2, pad 1 -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) maxpool_kernel(const float* in, float* out, int planes, int hi, int wi, int ho,
                                                     int wo) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)planes * ho * wo) return;
  const int x = (int)(i % wo), y = (int)((i / wo) % ho);
  const size_t p = i / ((size_t)wo * ho);
  const float* src = in + p * hi * wi;
  float m = -INFINITY;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = 2 * y + dy, xx = 2 * x + dx;
      if (yy >= 0 && yy < hi && xx >= 0 && xx < wi) m = fmaxf(m, src[(size_t)yy * wi + xx]);
    }
  out[i] = m;
}

// ---- what the networks' entry points share on the host ----------------------------------------------------------------
// A batch of frames a network takes.  The last bound keeps every map below 2^31 elements: the largest has 256 channels
// at stride 4 (teeth) or, the same number, 64 channels at stride 2 (parsing).
inline bool frames_ok(int B, int H, int W) {
  return B >= 1 && H >= 64 && W >= 64 && H % 32 == 0 && W % 32 == 0 && H <= 4096 && W <= 4096 &&
         (size_t)B * 16 * H * W < ((size_t)1 << 31);
}
constexpr const char* FRAMES_OK = ": B >= 1, H and W multiples of 32 in [64, 4096], B * 16 * H * W < 2^31";

// The convolutions of one forward pass: layer l of the weight struct's three arrays on B frames.
struct ConvNet {
  const float* const* w;
  const float* const* scale;
  const float* const* shift;
  int B;
  hipStream_t st;

  // the first of n layers with a NULL pointer, or -1
  int null_layer(int n) const {
    for (int l = 0; l < n; ++l)
      if (!w[l] || !scale[l] || !shift[l]) return l;
    return -1;
  }

  // act(scale * conv_ks(in) + shift [+ res]) with pad ks / 2; `extra` carries what else the gather or the epilogue folds in
  int operator()(int layer, int ks, const float* in, int cin, int hi, int wi, int stride, int cout, float* out,
                 const float* res, int relu, ConvArgs extra = ConvArgs{}) const {
    ConvArgs c = extra;
    c.in = in; c.wt = w[layer]; c.scale = scale[layer]; c.shift = shift[layer]; c.res = res; c.out = out;
    c.B = B; c.cin = cin; c.cout = cout; c.hi = hi; c.wi = wi; c.stride = stride; c.relu = relu;
    if (!c.in2) c.c_split = cin;
    c.ho = (hi + 2 * (ks / 2) - ks) / stride + 1;
    c.wo = (wi + 2 * (ks / 2) - ks) / stride + 1;
    return ks == 1 ? launch_conv<1>(c, st) : ks == 3 ? launch_conv<3>(c, st) : launch_conv_tile<7, 2>(c, st);
  }

  // the 3 x 3 max-pool behind a stem: [B * ch, hi, wi] -> [B * ch, hi / 2, wi / 2]
  int maxpool(const float* in, float* out, int ch, int hi, int wi) const {
    const size_t n = (size_t)B * ch * (hi / 2) * (wi / 2);
    maxpool_kernel<<<(unsigned)div_up(n, (size_t)TB), TB, 0, st>>>(in, out, B * ch, hi, wi, hi / 2, wi / 2);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  }
};

// ---- the label of one pixel ----------------------------------------------------------------------------------------------
// The bilinear interpolation of the C planes src [C, hs, ws] at the source position of pixel (py, px) of an H x W grid,
// and the first maximum over them.  ALIGN_CORNERS: the position is dst (hs - 1) / (H - 1); otherwise
// (dst + 0.5) hs / H - 0.5 clamped at 0.
template <bool ALIGN_CORNERS>
__device__ inline int bilinear_argmax(const float* src, int C, int hs, int ws, int H, int W, int py, int px) {
  float fy, fx;
  if constexpr (ALIGN_CORNERS) {
    fy = (H > 1 ? (float)(hs - 1) / (float)(H - 1) : 0.f) * (float)py;
    fx = (W > 1 ? (float)(ws - 1) / (float)(W - 1) : 0.f) * (float)px;
  } else {
    fy = fmaxf(((float)py + 0.5f) * ((float)hs / (float)H) - 0.5f, 0.f);
    fx = fmaxf(((float)px + 0.5f) * ((float)ws / (float)W) - 0.5f, 0.f);
  }
  const int y0 = min((int)fy, hs - 1), x0 = min((int)fx, ws - 1);
  const int y1 = min(y0 + 1, hs - 1), x1 = min(x0 + 1, ws - 1);
  float ly = fy - (float)y0, lx = fx - (float)x0;
  if constexpr (ALIGN_CORNERS) {
    ly = fminf(fmaxf(ly, 0.f), 1.f);
    lx = fminf(fmaxf(lx, 0.f), 1.f);
  }
  const float hy = 1.f - ly, hx = 1.f - lx;
  float best = 0.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float* p = src + (size_t)c * hs * ws;
    const float v = hy * (hx * p[y0 * ws + x0] + lx * p[y0 * ws + x1]) + ly * (hx * p[y1 * ws + x0] + lx * p[y1 * ws + x1]);
    if (c == 0 || v > best) { best = v; arg = c; }             // the first maximum
  }
  return arg;
}

}  // namespace
}  // namespace instag
