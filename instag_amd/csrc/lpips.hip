// LPIPS (AlexNet, eval mode) of square patches cut in place from an image and its target: forward and the gradient
// with respect to the image, fp32 (include/instag_hip.h, "LPIPS patch loss").
//
// Convolutions are implicit GEMMs on the f32-input MFMA (v_mfma_f32_32x32x2_f32): D[cout][m] = sum_k W[cout][k] X[k][m]
// with m = (image, oy, ox) and k = (cin, ky, kx) gathered from NCHW activations, 64 x 64 x 32 tiles, four waves of one
// 32 x 32 accumulator each (the tile scheme of mfma_tile.hpp).  The MFMA is a k-ordered fp32 FMA chain -- run per K
// tile of 32 and the tiles added in order (mfma_tile.hpp: blocked summation) -- and every other sum below runs in a
// fixed order (no float atomics), so two runs give the same bits.  The data gradient of the stride-1 layers is the
// same kernel on flipped, transposed weights (prepared by the caller); conv1 (stride 4, three input channels) has a
// gather kernel.
//
// The patch size lives in device memory: every kernel derives the patch count and the layer extents from it, buffers
// and grids are sized for the worst case of the declared range [p_min, p_max], and workgroups beyond the live extent
// exit.  A captured launch sequence therefore serves every patch size of its range; a value outside the range makes
// every kernel exit without touching memory.
#include "mfma_tile.hpp"

namespace instag {
namespace {

constexpr int NTAP = 5;

struct Geo {
  const int32_t* p_dev;
  int H, W, pmin, pmax, nstack;      // nstack > 0: the inputs are [nstack,3,p,p] stacks of patches, not a [3,H,W] image
};

struct Dims { int p, n, h1, q1, q2; bool ok; };

__host__ __device__ inline Dims dims_of(int p, int H, int W, int nstack) {
  Dims d;
  d.p = p;
  d.n = nstack > 0 ? nstack : (H / p) * (W / p);
  d.h1 = (p - 7) / 4 + 1;            // conv1: k11 s4 p2
  d.q1 = (d.h1 - 3) / 2 + 1;         // max-pool 3 s2 (conv2 keeps the extent)
  d.q2 = (d.q1 - 3) / 2 + 1;         // max-pool 3 s2 (conv3..5 keep the extent)
  d.ok = true;
  return d;
}

__device__ __forceinline__ Dims get_dims(const Geo& g) {
  const int p = *g.p_dev;
  if (p < g.pmin || p > g.pmax) { Dims d{}; d.ok = false; return d; }
  return dims_of(p, g.H, g.W, g.nstack);
}

template <int SEL> __device__ __forceinline__ int ext(const Dims& d) {
  return SEL == 0 ? d.p : SEL == 1 ? d.h1 : SEL == 2 ? d.q1 : d.q2;
}
__device__ __forceinline__ int tap_ext(const Dims& d, int tap) { return tap == 0 ? d.h1 : tap == 1 ? d.q1 : d.q2; }
__host__ __device__ inline int tap_channels(int tap) {
  return tap == 0 ? 64 : tap == 1 ? 192 : tap == 2 ? 384 : 256;
}

__device__ __forceinline__ float shift_of(int c) { return c == 0 ? -.030f : c == 1 ? -.088f : -.188f; }
__device__ __forceinline__ float scale_of(int c) { return c == 0 ? .458f : c == 1 ? .448f : .450f; }

// ---- convolution as implicit GEMM -----------------------------------------------------------------------------------
enum Epilogue { EPI_RELU = 0, EPI_MASKADD = 1, EPI_PLAIN = 2 };

struct ConvArgs {
  Geo geo;
  const float* in;      // [images, Cin, e, e]; the first layer: the image (or the stack of x patches)
  const float* in2;     // the first layer: the target
  const float* wt;      // [Kpad][Cout]
  const float* bias;    // EPI_RELU
  const float* act;     // EPI_MASKADD: the forward activation the output is the gradient of
  float* out;           // [images, Cout, e', e']  (EPI_MASKADD: holds the tap gradient on entry)
  const int32_t* rect;  // first layer: lips rectangle (r0, r1, c0, c1) or NULL
  const float* bg;
  int Cin, Cout, Kreal, Kpad, both;
};

template <int KH, int S, int PAD, int EIN, int EOUT, int EPI, bool FIRST>
__global__ void __launch_bounds__(TB) conv_kernel(ConvArgs a) {
  __shared__ float As[BK][64];
  __shared__ float Bs[BK][64];
  const Dims d = get_dims(a.geo);
  if (!d.ok) return;
  const int ih = ext<EIN>(d), oh = ext<EOUT>(d);
  const int imgs = a.both ? 2 * d.n : d.n;
  const int HWo = oh * oh;
  const int M = imgs * HWo;
  const int m0 = blockIdx.x * 64;
  if (m0 >= M) return;
  const int c0 = blockIdx.y * 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  const int tm = t & 63, kr = t >> 6;

  // this thread's column of the gathered operand: one output position
  const int mg = m0 + tm;
  const bool mv = mg < M;
  int img = 0, oy = 0, ox = 0;
  if (mv) {
    img = mg / HWo;
    const int pos = mg - img * HWo;
    oy = pos / oh;
    ox = pos - oy * oh;
  }
  const float* src = a.in;
  int Y0 = 0, X0 = 0, r0 = 0, r1 = 0, q0 = 0, q1 = 0;
  if (FIRST) {
    int pi = img;
    if (img >= d.n) { pi = img - d.n; src = a.in2; }
    if (a.geo.nstack > 0) {
      src += (size_t)pi * 3 * d.p * d.p;
    } else {
      const int ppr = a.geo.W / d.p;
      Y0 = (pi / ppr) * d.p;
      X0 = (pi % ppr) * d.p;
      if (a.rect) { r0 = a.rect[0]; r1 = a.rect[1]; q0 = a.rect[2]; q1 = a.rect[3]; }
    }
  } else {
    src += (size_t)img * a.Cin * ih * ih;
  }
  const int iy0 = oy * S - PAD, ix0 = ox * S - PAD;

  auto gather = [&](int k) -> float {
    if (!mv || k >= a.Kreal) return 0.f;
    const int ci = k / (KH * KH);
    const int r = k - ci * (KH * KH);
    const int ky = r / KH, kx = r - ky * KH;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (iy < 0 || iy >= ih || ix < 0 || ix >= ih) return 0.f;
    if (FIRST) {
      float v;
      if (a.geo.nstack > 0) {                                   // a stack holds the criterion's input itself
        v = src[((size_t)ci * d.p + iy) * d.p + ix];
      } else {
        const int Y = Y0 + iy, X = X0 + ix;
        v = (Y >= r0 && Y < r1 && X >= q0 && X < q1) ? a.bg[ci] : src[((size_t)ci * a.geo.H + Y) * a.geo.W + X];
        v = v * 2.f - 1.f;
      }
      return (v - shift_of(ci)) / scale_of(ci);
    }
    return src[((size_t)ci * ih + iy) * ih + ix];
  };

  float ra[8], rb[8];
  auto load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = kt * BK + kr + 4 * i;
      ra[i] = a.wt[(size_t)k * a.Cout + c0 + tm];
      rb[i] = gather(k);
    }
  };

  f32x16 acc[1][1];                                            // mfma_k_tile takes [WM][WN] accumulators
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[0][0][i] = 0.f;
  const int nk = a.Kpad / BK;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      As[kr + 4 * i][tm] = ra[i];
      Bs[kr + 4 * i][tm] = rb[i];
    }
    __syncthreads();
    if (kt + 1 < nk) load(kt + 1);
    mfma_k_tile<1, 1, true>(As, Bs, wr * 32, wc * 32, lane, acc);
  }

  // D: column = output position, row = output channel
  const int mc = m0 + wc * 32 + (lane & 31);
  if (mc >= M) return;
  const int oimg = mc / HWo, opos = mc - oimg * HWo;
  const size_t obase = (size_t)oimg * a.Cout * HWo + opos;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = mfma_row(c0 + wr * 32, r, lane);
    const size_t o = obase + (size_t)co * HWo;
    float v = acc[0][0][r];
    if (EPI == EPI_RELU) {
      v = fmaxf(v + a.bias[co], 0.f);
    } else if (EPI == EPI_MASKADD) {
      v = a.act[o] > 0.f ? v + a.out[o] : 0.f;
    }
    a.out[o] = v;
  }
}

// ---- max-pool 3 s2 ---------------------------------------------------------------------------------------------------
// forward over the 2n images of x and y; the position of the (first) maximum is kept for the n images of x
template <int EIN, int EOUT>
__global__ void __launch_bounds__(TB) pool_forward_kernel(Geo geo, const float* __restrict__ in, float* __restrict__ out,
                                                          uint8_t* __restrict__ idx, int C) {
  const Dims d = get_dims(geo);
  if (!d.ok) return;
  const int ei = ext<EIN>(d), eo = ext<EOUT>(d);
  const size_t total = (size_t)2 * d.n * C * eo * eo;
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % eo), oy = (int)((i / eo) % eo);
  const size_t ic = i / ((size_t)eo * eo);                       // image * C + channel
  const float* src = in + ic * ei * ei + (size_t)(2 * oy) * ei + 2 * ox;
  float best = src[0];
  int bi = 0;
#pragma unroll
  for (int j = 1; j < 9; ++j) {
    const float v = src[(j / 3) * ei + (j % 3)];
    if (v > best) { best = v; bi = j; }
  }
  out[i] = best;
  if (ic < (size_t)d.n * C) idx[i] = (uint8_t)bi;
}

// g[img, c, y, x] = act > 0 ? (sum of the pooled gradients whose window chose (y, x)) + g : 0    (the n images of x)
template <int EIN, int EOUT>
__global__ void __launch_bounds__(TB) pool_backward_kernel(Geo geo, const float* __restrict__ act,
                                                           const float* __restrict__ pg, const uint8_t* __restrict__ idx,
                                                           float* __restrict__ g, int C) {
  const Dims d = get_dims(geo);
  if (!d.ok) return;
  const int ei = ext<EIN>(d), eo = ext<EOUT>(d);
  const size_t total = (size_t)d.n * C * ei * ei;
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % ei), y = (int)((i / ei) % ei);
  const size_t ic = i / ((size_t)ei * ei);
  float s = 0.f;
  const int oy0 = max(0, (y - 1) / 2), oy1 = min(eo - 1, y / 2);
  const int ox0 = max(0, (x - 1) / 2), ox1 = min(eo - 1, x / 2);
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      const size_t o = ic * eo * eo + (size_t)oy * eo + ox;
      if ((int)idx[o] == (y - 2 * oy) * 3 + (x - 2 * ox)) s += pg[o];
    }
  g[i] = act[i] > 0.f ? s + g[i] : 0.f;
}

// ---- tap stage: normalise, difference, lin, spatial mean ------------------------------------------------------------
struct TapArgs {
  Geo geo;
  const float* act[NTAP];   // [2n, C, e, e]: x then y
  const float* lin[NTAP];   // [C]
  float* grad[NTAP];        // backward: [n, C, e, e]
  float* tapval;            // [NTAP][n_max]
  const float* g;           // backward: upstream gradient (of the mean, or one per patch)
  int n_max, g_per_patch;
};

__device__ __forceinline__ float block_sum(float v, float* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = TB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  return s[0];
}

__global__ void __launch_bounds__(TB) tap_forward_kernel(TapArgs a) {
  __shared__ float s[TB];
  const Dims d = get_dims(a.geo);
  if (!d.ok) return;
  const int patch = blockIdx.x, tap = blockIdx.y;
  if (patch >= d.n) return;
  const int e = tap_ext(d, tap), HW = e * e, C = tap_channels(tap);
  const float* fx = a.act[tap] + (size_t)patch * C * HW;
  const float* fy = a.act[tap] + (size_t)(patch + d.n) * C * HW;
  const float* w = a.lin[tap];
  float acc = 0.f;
  for (int pos = threadIdx.x; pos < HW; pos += TB) {
    float sx = 0.f, sy = 0.f;
    for (int c = 0; c < C; ++c) {
      const float vx = fx[(size_t)c * HW + pos], vy = fy[(size_t)c * HW + pos];
      sx += vx * vx;
      sy += vy * vy;
    }
    sx = sqrtf(sx) + 1e-10f;
    sy = sqrtf(sy) + 1e-10f;
    float v = 0.f;
    for (int c = 0; c < C; ++c) {
      const float dd = fx[(size_t)c * HW + pos] / sx - fy[(size_t)c * HW + pos] / sy;
      v += w[c] * (dd * dd);
    }
    acc += v;
  }
  const float tot = block_sum(acc, s);
  if (threadIdx.x == 0) a.tapval[tap * a.n_max + patch] = tot / (float)HW;
}

// per_patch[i] = sum of the five taps; mean = sum_i per_patch[i] / n
__global__ void __launch_bounds__(TB) finalize_kernel(Geo geo, const float* __restrict__ tapval, int n_max,
                                                      float* __restrict__ per_patch, float* __restrict__ mean_out) {
  __shared__ float s[TB];
  const Dims d = get_dims(geo);
  if (!d.ok) return;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_max; i += TB) {
    float v = 0.f;
    if (i < d.n) {
      for (int tap = 0; tap < NTAP; ++tap) v += tapval[tap * n_max + i];
      acc += v;
    }
    per_patch[i] = v;
  }
  const float tot = block_sum(acc, s);
  if (threadIdx.x == 0 && mean_out) mean_out[0] = tot / (float)d.n;
}

// gradient of the tap stage with respect to fx (ny is constant); the last tap applies its own ReLU mask, the others
// are masked where the gradient arriving from the next layer is added
__global__ void __launch_bounds__(TB) tap_backward_kernel(TapArgs a) {
  const Dims d = get_dims(a.geo);
  if (!d.ok) return;
  const int patch = blockIdx.x, tap = blockIdx.y;
  if (patch >= d.n) return;
  const int e = tap_ext(d, tap), HW = e * e, C = tap_channels(tap);
  const float* fx = a.act[tap] + (size_t)patch * C * HW;
  const float* fy = a.act[tap] + (size_t)(patch + d.n) * C * HW;
  const float* w = a.lin[tap];
  float* go = a.grad[tap] + (size_t)patch * C * HW;
  const float gp = (a.g_per_patch ? a.g[patch] : a.g[0] / (float)d.n) / (float)HW;
  for (int pos = threadIdx.x; pos < HW; pos += TB) {
    float qx = 0.f, qy = 0.f;
    for (int c = 0; c < C; ++c) {
      const float vx = fx[(size_t)c * HW + pos], vy = fy[(size_t)c * HW + pos];
      qx += vx * vx;
      qy += vy * vy;
    }
    const float rx = sqrtf(qx);
    const float sx = rx + 1e-10f, sy = sqrtf(qy) + 1e-10f;
    float dot = 0.f;                                            // sum_c dn_c fx_c
    for (int c = 0; c < C; ++c) {
      const float vx = fx[(size_t)c * HW + pos];
      const float dn = gp * 2.f * w[c] * (vx / sx - fy[(size_t)c * HW + pos] / sy);
      dot += dn * vx;
    }
    const float k2 = rx > 0.f ? dot / (rx * sx * sx) : 0.f;
    for (int c = 0; c < C; ++c) {
      const float vx = fx[(size_t)c * HW + pos];
      const float dn = gp * 2.f * w[c] * (vx / sx - fy[(size_t)c * HW + pos] / sy);
      float gv = dn / sx - vx * k2;
      if (tap == NTAP - 1 && !(vx > 0.f)) gv = 0.f;
      go[(size_t)c * HW + pos] = gv;
    }
  }
}

// ---- conv1 data gradient: gather over the (<= 3 x 3) kernel taps that reach a pixel, scattered into the image ---------
// One workgroup handles pixels of one phase (y % 4, x % 4) of one patch, so the weight addresses are uniform.
struct Conv1BwdArgs {
  Geo geo;
  const float* g1;      // [n, 64, h1, h1]
  const float* w1;      // [64, 3, 11, 11]
  const int32_t* rect;
  float* dimage;        // [3, H, W], or [nstack, 3, p, p]
  int n_max;            // workgroups with blockIdx.z == n_max write the zeros of the dropped remainder
};

__global__ void __launch_bounds__(TB) conv1_backward_kernel(Conv1BwdArgs a) {
  const Dims d = get_dims(a.geo);
  if (!d.ok) return;
  const int patch = blockIdx.z;
  if (patch == a.n_max) {
    if (a.geo.nstack > 0) return;
    // the rows and columns no patch covers (the patch kernels write every pixel of the live area)
    const int H = a.geo.H, W = a.geo.W, Hl = (H / d.p) * d.p, Wl = (W / d.p) * d.p;
    const int nthreads = gridDim.x * gridDim.y * TB;
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * TB + threadIdx.x; i < 3 * H * W; i += nthreads) {
      const int X = i % W, Y = (i / W) % H;
      if (Y >= Hl || X >= Wl) a.dimage[i] = 0.f;
    }
    return;
  }
  if (patch >= d.n) return;
  const int A = (d.p + 3) / 4;
  const int id = blockIdx.x * TB + threadIdx.x;
  const int ya = id / A, xb = id - ya * A;
  const int py = blockIdx.y >> 2, px = blockIdx.y & 3;
  const int y = 4 * ya + py, x = 4 * xb + px;
  if (y >= d.p || x >= d.p) return;
  const int h1 = d.h1, HW = h1 * h1;
  const int ky0 = (py + 2) & 3, kx0 = (px + 2) & 3;
  // output rows / columns that see this pixel through kernel tap ky0 + 4 j: (y + 2 - ky) / 4
  int off[9];
  bool ok[9];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ky = ky0 + 4 * j, kx = kx0 + 4 * i;
      const int ny = y + 2 - ky, nx = x + 2 - kx;
      const int oy = ny >> 2, ox = nx >> 2;
      ok[j * 3 + i] = ky < 11 && kx < 11 && ny >= 0 && nx >= 0 && oy < h1 && ox < h1;
      off[j * 3 + i] = oy * h1 + ox;
    }
  const float* g = a.g1 + (size_t)patch * 64 * HW;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
  for (int co = 0; co < 64; ++co) {
    const float* wc = a.w1 + (size_t)co * 363;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int ky = ky0 + 4 * j, kx = kx0 + 4 * i;
        if (ky < 11 && kx < 11) {                               // (uniform over the workgroup)
          const float gv = ok[j * 3 + i] ? g[(size_t)co * HW + off[j * 3 + i]] : 0.f;
          const int wi = ky * 11 + kx;
          acc0 += gv * wc[wi];
          acc1 += gv * wc[121 + wi];
          acc2 += gv * wc[242 + wi];
        }
      }
  }
  const float in_scale = a.geo.nstack > 0 ? 1.f : 2.f;          // d(v * 2 - 1) / dv of the image form
  const float r0 = acc0 / scale_of(0) * in_scale, r1 = acc1 / scale_of(1) * in_scale, r2 = acc2 / scale_of(2) * in_scale;
  if (a.geo.nstack > 0) {
    float* o = a.dimage + (size_t)patch * 3 * d.p * d.p + (size_t)y * d.p + x;
    o[0] = r0;
    o[(size_t)d.p * d.p] = r1;
    o[(size_t)2 * d.p * d.p] = r2;
    return;
  }
  const int ppr = a.geo.W / d.p;
  const int Y = (patch / ppr) * d.p + y, X = (patch % ppr) * d.p + x;
  const bool filled = a.rect && Y >= a.rect[0] && Y < a.rect[1] && X >= a.rect[2] && X < a.rect[3];
  const size_t plane = (size_t)a.geo.H * a.geo.W;
  float* o = a.dimage + (size_t)Y * a.geo.W + X;
  o[0] = filled ? 0.f : r0;
  o[plane] = filled ? 0.f : r1;
  o[2 * plane] = filled ? 0.f : r2;
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct Plan {
  int n_max = 0;
  size_t a[NTAP] = {0, 0, 0, 0, 0};    // n * C * e^2 per tap, worst case
  size_t pl[2] = {0, 0};               // n * C * e^2 of the two pooled maps
  size_t m[3] = {0, 0, 0};             // n * e^2 at h1, q1, q2
  // offsets in floats
  size_t act[NTAP], pool[2], idx[2], grad[NTAP], pgrad[2], tapval, total;
};

int make_plan(int H, int W, int pmin, int pmax, int nstack, Plan* out, const char* who) {
  INSTAG_REQUIRE(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, std::string(who) + ": bad image size");
  INSTAG_REQUIRE(pmin >= 31, std::string(who) + ": a patch below 31 pixels leaves no room for the second pool window");
  INSTAG_REQUIRE(pmax >= pmin && pmax <= 1024, std::string(who) + ": bad patch-size range");
  INSTAG_REQUIRE(nstack >= 0 && nstack <= 65534, std::string(who) + ": bad patch count");
  INSTAG_REQUIRE(nstack > 0 || (H >= pmin && W >= pmin), std::string(who) + ": the image is smaller than one patch");
  Plan pl;
  for (int p = pmin; p <= pmax; ++p) {
    const Dims d = dims_of(p, H, W, nstack);
    if (d.n < 1) continue;
    pl.n_max = std::max(pl.n_max, d.n);
    const int e[NTAP] = {d.h1, d.q1, d.q2, d.q2, d.q2};
    for (int t = 0; t < NTAP; ++t) pl.a[t] = std::max(pl.a[t], (size_t)d.n * tap_channels(t) * e[t] * e[t]);
    pl.pl[0] = std::max(pl.pl[0], (size_t)d.n * 64 * d.q1 * d.q1);
    pl.pl[1] = std::max(pl.pl[1], (size_t)d.n * 192 * d.q2 * d.q2);
    pl.m[0] = std::max(pl.m[0], (size_t)d.n * d.h1 * d.h1);
    pl.m[1] = std::max(pl.m[1], (size_t)d.n * d.q1 * d.q1);
    pl.m[2] = std::max(pl.m[2], (size_t)d.n * d.q2 * d.q2);
  }
  INSTAG_REQUIRE(pl.n_max <= 65534, std::string(who) + ": too many patches");
  Arena ws;
  for (int t = 0; t < NTAP; ++t) pl.act[t] = ws.take(2 * pl.a[t]);
  for (int t = 0; t < 2; ++t) pl.pool[t] = ws.take(2 * pl.pl[t]);
  for (int t = 0; t < 2; ++t) pl.idx[t] = ws.take((pl.pl[t] + 3) / 4);
  for (int t = 0; t < NTAP; ++t) pl.grad[t] = ws.take(pl.a[t]);
  for (int t = 0; t < 2; ++t) pl.pgrad[t] = ws.take(pl.pl[t]);
  pl.tapval = ws.take((size_t)NTAP * pl.n_max);
  pl.total = ws.off;
  INSTAG_REQUIRE(2 * pl.a[0] <= 0x7fffffffull && 2 * pl.a[1] <= 0x7fffffffull, std::string(who) + ": problem too large");
  *out = pl;
  return INSTAG_OK;
}

int check_p(int p_host, int H, int W, int pmin, int pmax, int nstack, const char* who) {
  if (p_host < 0) return INSTAG_OK;          // not known on the host (a captured launch): the kernels guard the range
  INSTAG_REQUIRE(p_host >= pmin && p_host <= pmax, std::string(who) + ": patch size outside the declared range");
  INSTAG_REQUIRE(nstack > 0 || (H >= p_host && W >= p_host), std::string(who) + ": the image is smaller than one patch");
  return INSTAG_OK;
}

bool weights_complete(const instag_lpips_weights* w) {
  if (!w) return false;
  for (int i = 0; i < NTAP; ++i)
    if (!w->wf[i] || !w->bias[i] || !w->wb[i] || !w->lin[i]) return false;
  return true;
}

template <typename K>
int launch_conv(K kernel, const ConvArgs& a, size_t m_max, hipStream_t st) {
  dim3 grid((unsigned)div_up(m_max, (size_t)64), (unsigned)(a.Cout / 64));
  kernel<<<grid, TB, 0, st>>>(a);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_lpips_workspace_bytes(int32_t H, int32_t W, int32_t p_min, int32_t p_max, int32_t n_stack) {
  Plan pl;
  if (make_plan(H, W, p_min, p_max, n_stack, &pl, "lpips_workspace_bytes") != INSTAG_OK) return 0;
  return pl.total * sizeof(float);
}

int instag_lpips_max_patches(int32_t H, int32_t W, int32_t p_min, int32_t p_max, int32_t n_stack) {
  Plan pl;
  if (make_plan(H, W, p_min, p_max, n_stack, &pl, "lpips_max_patches") != INSTAG_OK) return 0;
  return pl.n_max;
}

int instag_lpips_forward(const instag_lpips_weights* w, const float* image, const float* gt, const int32_t* p_dev,
                         int32_t p_host, const int32_t* rect, const float* bg, int32_t H, int32_t W, int32_t p_min,
                         int32_t p_max, int32_t n_stack, void* workspace, size_t workspace_bytes, float* per_patch,
                         float* mean_out, instag_stream_t stream) {
  INSTAG_REQUIRE(weights_complete(w) && image && gt && p_dev && workspace && per_patch, "lpips_forward: NULL tensor");
  INSTAG_REQUIRE(!rect || bg, "lpips_forward: NULL background for the lips rectangle");
  Plan pl;
  if (int rc = make_plan(H, W, p_min, p_max, n_stack, &pl, "lpips_forward")) return rc;
  if (int rc = check_p(p_host, H, W, p_min, p_max, n_stack, "lpips_forward")) return rc;
  INSTAG_REQUIRE(workspace_bytes >= pl.total * sizeof(float), "lpips_forward: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const Geo geo{p_dev, H, W, p_min, p_max, n_stack};

  ConvArgs c{};
  c.geo = geo;
  c.both = 1;
  // conv1 + ReLU (reads the image and the target in place)
  c.in = image; c.in2 = gt; c.rect = n_stack > 0 ? nullptr : rect; c.bg = bg;
  c.wt = w->wf[0]; c.bias = w->bias[0]; c.out = ws + pl.act[0];
  c.Cin = 3; c.Cout = 64; c.Kreal = 363; c.Kpad = 384;
  if (int rc = launch_conv(conv_kernel<11, 4, 2, 0, 1, EPI_RELU, true>, c, 2 * pl.m[0], st)) return rc;
  pool_forward_kernel<1, 2><<<(unsigned)div_up(2 * pl.pl[0], (size_t)TB), TB, 0, st>>>(
      geo, ws + pl.act[0], ws + pl.pool[0], (uint8_t*)(ws + pl.idx[0]), 64);
  INSTAG_CHECK_LAUNCH();
  c.rect = nullptr; c.in2 = nullptr;
  c.in = ws + pl.pool[0]; c.wt = w->wf[1]; c.bias = w->bias[1]; c.out = ws + pl.act[1];
  c.Cin = 64; c.Cout = 192; c.Kreal = c.Kpad = 1600;
  if (int rc = launch_conv(conv_kernel<5, 1, 2, 2, 2, EPI_RELU, false>, c, 2 * pl.m[1], st)) return rc;
  pool_forward_kernel<2, 3><<<(unsigned)div_up(2 * pl.pl[1], (size_t)TB), TB, 0, st>>>(
      geo, ws + pl.act[1], ws + pl.pool[1], (uint8_t*)(ws + pl.idx[1]), 192);
  INSTAG_CHECK_LAUNCH();
  const int cin[3] = {192, 384, 256}, cout[3] = {384, 256, 256};
  for (int l = 0; l < 3; ++l) {
    c.in = l == 0 ? ws + pl.pool[1] : ws + pl.act[1 + l];
    c.wt = w->wf[2 + l]; c.bias = w->bias[2 + l]; c.out = ws + pl.act[2 + l];
    c.Cin = cin[l]; c.Cout = cout[l]; c.Kreal = c.Kpad = cin[l] * 9;
    if (int rc = launch_conv(conv_kernel<3, 1, 1, 3, 3, EPI_RELU, false>, c, 2 * pl.m[2], st)) return rc;
  }
  TapArgs t{};
  t.geo = geo;
  for (int i = 0; i < NTAP; ++i) { t.act[i] = ws + pl.act[i]; t.lin[i] = w->lin[i]; }
  t.tapval = ws + pl.tapval;
  t.n_max = pl.n_max;
  tap_forward_kernel<<<dim3((unsigned)pl.n_max, NTAP), TB, 0, st>>>(t);
  INSTAG_CHECK_LAUNCH();
  finalize_kernel<<<1, TB, 0, st>>>(geo, ws + pl.tapval, pl.n_max, per_patch, mean_out);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_lpips_backward(const instag_lpips_weights* w, const int32_t* p_dev, int32_t p_host, const int32_t* rect,
                          const float* g, int32_t g_per_patch, int32_t H, int32_t W, int32_t p_min, int32_t p_max,
                          int32_t n_stack, void* workspace, size_t workspace_bytes, float* dimage,
                          instag_stream_t stream) {
  INSTAG_REQUIRE(weights_complete(w) && p_dev && g && workspace && dimage, "lpips_backward: NULL tensor");
  Plan pl;
  if (int rc = make_plan(H, W, p_min, p_max, n_stack, &pl, "lpips_backward")) return rc;
  if (int rc = check_p(p_host, H, W, p_min, p_max, n_stack, "lpips_backward")) return rc;
  INSTAG_REQUIRE(workspace_bytes >= pl.total * sizeof(float), "lpips_backward: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const Geo geo{p_dev, H, W, p_min, p_max, n_stack};

  TapArgs t{};
  t.geo = geo;
  for (int i = 0; i < NTAP; ++i) { t.act[i] = ws + pl.act[i]; t.lin[i] = w->lin[i]; t.grad[i] = ws + pl.grad[i]; }
  t.g = g;
  t.g_per_patch = g_per_patch;
  t.n_max = pl.n_max;
  tap_backward_kernel<<<dim3((unsigned)pl.n_max, NTAP), TB, 0, st>>>(t);
  INSTAG_CHECK_LAUNCH();

  ConvArgs c{};
  c.geo = geo;
  c.both = 0;
  // conv5, conv4: the gradient arrives at a tapped ReLU output without a pool in between
  const int co5[2] = {256, 256}, ci5[2] = {256, 384};
  for (int l = 0; l < 2; ++l) {
    c.in = ws + pl.grad[4 - l]; c.wt = w->wb[4 - l]; c.act = ws + pl.act[3 - l]; c.out = ws + pl.grad[3 - l];
    c.Cin = co5[l]; c.Cout = ci5[l]; c.Kreal = c.Kpad = co5[l] * 9;
    if (int rc = launch_conv(conv_kernel<3, 1, 1, 3, 3, EPI_MASKADD, false>, c, pl.m[2], st)) return rc;
  }
  c.act = nullptr;
  c.in = ws + pl.grad[2]; c.wt = w->wb[2]; c.out = ws + pl.pgrad[1];
  c.Cin = 384; c.Cout = 192; c.Kreal = c.Kpad = 384 * 9;
  if (int rc = launch_conv(conv_kernel<3, 1, 1, 3, 3, EPI_PLAIN, false>, c, pl.m[2], st)) return rc;
  pool_backward_kernel<2, 3><<<(unsigned)div_up(pl.a[1], (size_t)TB), TB, 0, st>>>(
      geo, ws + pl.act[1], ws + pl.pgrad[1], (const uint8_t*)(ws + pl.idx[1]), ws + pl.grad[1], 192);
  INSTAG_CHECK_LAUNCH();
  c.in = ws + pl.grad[1]; c.wt = w->wb[1]; c.out = ws + pl.pgrad[0];
  c.Cin = 192; c.Cout = 64; c.Kreal = c.Kpad = 192 * 25;
  if (int rc = launch_conv(conv_kernel<5, 1, 2, 2, 2, EPI_PLAIN, false>, c, pl.m[1], st)) return rc;
  pool_backward_kernel<1, 2><<<(unsigned)div_up(pl.a[0], (size_t)TB), TB, 0, st>>>(
      geo, ws + pl.act[0], ws + pl.pgrad[0], (const uint8_t*)(ws + pl.idx[0]), ws + pl.grad[0], 64);
  INSTAG_CHECK_LAUNCH();

  INSTAG_REQUIRE(n_stack > 0 || (long long)3 * H * W <= 0x7fffffffll, "lpips_backward: image too large");
  Conv1BwdArgs b{geo, ws + pl.grad[0], w->wb[0], n_stack > 0 ? nullptr : rect, dimage, pl.n_max};
  const int A = (p_max + 3) / 4;
  conv1_backward_kernel<<<dim3((unsigned)div_up(A * A, TB), 16, (unsigned)pl.n_max + 1), TB, 0, st>>>(b);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
