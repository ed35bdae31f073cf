// What the entry points of the pretrained convolution networks (parsing.hip, teeth.hip) share around the convolution of
// conv_mfma.hpp: the 3 x 3 max-pool behind their stems, the frame-shape predicate, ConvNet (layer index -> ConvArgs ->
// launch) and the per-pixel interpolation and argmax of their label kernels.
#pragma once
#include "conv_mfma.hpp"

namespace instag {
namespace {

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
    c.B = B; c.cin = cin; c.cout = cout; c.hi = hi; c.wi = wi; c.stride_h = c.stride_w = stride; c.relu = relu;
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
