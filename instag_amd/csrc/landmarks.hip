// Face landmarks (the reference's data_utils/process.py:54-85 calls the face_alignment package): FAN-2D-4 in eval mode,
// fp32, forward only, with the crop in front of it and the decode behind it (include/instag_landmarks.h; the network,
// its layer order and the arithmetic around it are stated in instag_amd/landmarks.py).
//
//   crop          one thread per pixel of the S x S crop: the box's centre and scale and the inverse transform in fp64, the
//                 (br - ul) image read straight off the frame (zero outside it), the bilinear resize in integers.  One
//                 launch; the (br - ul) image never exists.
//   the stem      the 7 x 7 stride-2 convolution of conv_mfma.hpp on the uint8 crop, the table u / 255.
//   ConvBlock     pre-activation: each of its three 3 x 3 convolutions reads max(v pre_scale + pre_shift, 0) in the gather
//                 (the padding zero AFTER it), writes its slice of the concatenation with its slice of the residual added
//                 in the epilogue, and leaves a contiguous copy without the residual for the next convolution to read.
//                 No cat, no add.  A downsample (BN, ReLU, 1 x 1) writes the whole output first, which the three slices
//                 then read as their residual in place.
//   hourglass     up1 + nearest_x2(low) is folded: the low path runs first and b1's three convolutions read it as a second
//                 residual at half resolution, behind the first ((cat + x) + up(low), the statement's order).  The 2 x 2
//                 average pools are a small kernel of their own: folded into the gather they would read four values per
//                 tap, nine times over, and the pooled map is also the block's residual.
//   al            K = 68, the rows up to 96 zero: the kernel's K loop rounds up and the gather returns zero past cin.
//   decode        one wave per (face, landmark): the first maximum, the two sign tests, the back-transform in fp64 and
//                 the truncation.
// 194 convolutions, 17 pools, no atomics, every sum a k-ordered chain per K tile of 32 with the tiles added in order: a
// face's bits depend neither on its batch nor on the tile.  The file is compiled with -ffp-contract=off: the fp64
// transform is the statement's operation by operation (an FMA would round once where it rounds twice and could move a
// truncation); the convolution's FMAs are explicit and stay.
#include "common.hpp"
#include "conv_mfma.hpp"
#include "instag_landmarks.h"

namespace instag {
namespace {

constexpr int NLAYER = INSTAG_LANDMARKS_LAYERS, NPTS = INSTAG_LANDMARKS_POINTS, NSTACK = INSTAG_LANDMARKS_STACKS;
constexpr int CH = 256;                          // the trunk's channels
static_assert(NLAYER == 12 + 4 * 44 + 3 * 2, "landmarks.LAYERS");

// order of instag_landmarks_weights (instag_amd/landmarks.py: LAYERS).  A ConvBlock is conv1, conv2, conv3[, downsample].
enum Layer { L_CONV1 = 0, L_CONV2 = 1, L_CONV3 = 5, L_CONV4 = 8, L_STACK = 12, STACK_LAYERS = 46 };
// within a stack: b1_l at 6 (4 - l), b2_l behind it, l = 4 .. 1
enum StackLayer { S_B2_PLUS = 24, S_B3 = 27, S_TOP = 39, S_LAST = 42, S_L = 43, S_BL = 44, S_AL = 45 };

bool has_pre(int layer) {
  if (layer < L_STACK) return layer != L_CONV1;
  return (layer - L_STACK) % STACK_LAYERS < S_LAST;
}

// ---- the box: centre, scale, inverse transform -------------------------------------------------------------------------
struct BoxMap {
  double cx, cy, h;
  bool ok;
};

__device__ inline BoxMap box_map(const float* box) {
  const double x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
  const double lim = (double)INSTAG_LANDMARKS_MAX_COORD;
  BoxMap m;
  m.ok = fabs(x1) <= lim && fabs(y1) <= lim && fabs(x2) <= lim && fabs(y2) <= lim;      // false for NaN
  const double w = x2 - x1, hg = y2 - y1;
  m.cx = x2 - w / 2.0;
  m.cy = y2 - hg / 2.0 - 0.12 * hg;
  m.h = 200.0 * ((w + hg) / 195.0);
  return m;
}

// transform(p, center, scale, res, invert = True) along one axis, truncated toward zero
__device__ inline int inverse(double p, double c, double h, double res) { return (int)(p * h / res + c - h / 2.0); }

// ---- crop ----------------------------------------------------------------------------------------------------------------
// one axis of the integer resize: output index o of S from n source pixels -> the two clamped indices and the second's
// weight out of 512
__device__ inline void resize_axis(int o, int n, int S, int& i0, int& i1, int& w1) {
  const int64_t num = (int64_t)(2 * o + 1) * n - S, den = 2 * S;             // the source position is num / den
  const int64_t fl = num >= 0 ? num / den : -((-num + den - 1) / den);
  w1 = (int)(((num - fl * den) * 512 + S) / den);
  i0 = (int)min(max(fl, (int64_t)0), (int64_t)n - 1);
  i1 = (int)min(max(fl + 1, (int64_t)0), (int64_t)n - 1);
}

__global__ void __launch_bounds__(TB) crop_kernel(const uint8_t* frames, int N, int H, int W, const float* boxes,
                                                  const int32_t* frame_index, int B, int S, uint8_t* crops) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)B * S * S) return;
  const int ox = (int)(i % S), oy = (int)((i / S) % S), b = (int)(i / ((size_t)S * S));
  const BoxMap m = box_map(boxes + 4 * b);
  const int f = frame_index ? frame_index[b] : b;
  int sum[3] = {0, 0, 0};
  if (m.ok && f >= 0 && f < N) {
    const int ulx = inverse(1.0, m.cx, m.h, 256.0), uly = inverse(1.0, m.cy, m.h, 256.0);
    const int cw = inverse(256.0, m.cx, m.h, 256.0) - ulx, ch = inverse(256.0, m.cy, m.h, 256.0) - uly;
    if (cw >= 1 && ch >= 1) {
      int y[2], x[2], wy, wx;
      resize_axis(oy, ch, S, y[0], y[1], wy);
      resize_axis(ox, cw, S, x[0], x[1], wx);
      const int wys[2] = {512 - wy, wy}, wxs[2] = {512 - wx, wx};
      const uint8_t* frame = frames + (size_t)f * H * W * 3;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int fy = y[a] + uly, fx = x[c] + ulx;
          if (fy < 0 || fy >= H || fx < 0 || fx >= W) continue;
          const uint8_t* px = frame + ((size_t)fy * W + fx) * 3;
          const int wgt = wys[a] * wxs[c];
#pragma unroll
          for (int k = 0; k < 3; ++k) sum[k] += wgt * (int)px[k];
        }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) crops[i * 3 + k] = (uint8_t)((sum[k] + (1 << 17)) >> 18);
}

// ---- decode --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) decode_kernel(const float* heat, const float* boxes, int B, int R, float* lms) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  if (pair >= B * NPTS) return;                                            // the whole wave
  const int n = R * R;                                                      // >= 256
  const float* hm = heat + (size_t)pair * n;
  float best = hm[lane];
  int arg = lane;
  for (int i = lane + 64; i < n; i += 64) {
    const float v = hm[i];
    if (v > best) { best = v; arg = i; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oa = __shfl_xor(arg, off);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  if (lane != 0) return;
  const int b = pair / NPTS;
  const BoxMap m = box_map(boxes + 4 * b);
  float* out = lms + (size_t)pair * 2;
  if (!m.ok) {
    out[0] = out[1] = __builtin_nanf("");
    return;
  }
  const int py = arg / R, px = arg - py * R;
  double x = (double)(px + 1), y = (double)(py + 1);
  if (px > 0 && px < R - 1 && py > 0 && py < R - 1) {
    const float dx = hm[arg + 1] - hm[arg - 1], dy = hm[arg + R] - hm[arg - R];
    x += dx > 0.f ? 0.25 : dx < 0.f ? -0.25 : 0.0;
    y += dy > 0.f ? 0.25 : dy < 0.f ? -0.25 : 0.0;
  }
  out[0] = (float)inverse(x - 0.5, m.cx, m.h, (double)R);
  out[1] = (float)inverse(y - 0.5, m.cy, m.h, (double)R);
}

// ---- 2 x 2 average pool --------------------------------------------------------------------------------------------------
// in [planes, 2 ho, 2 wo] -> out [planes, ho, wo]
__global__ void __launch_bounds__(TB) avgpool_kernel(const float* in, float* out, size_t total, int ho, int wo) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % wo), y = (int)((i / wo) % ho);
  const size_t p = i / ((size_t)wo * ho);
  const float* s = in + (p * 2 * ho + 2 * y) * 2 * wo + 2 * x;
  out[i] = (((s[0] + s[1]) + s[2 * wo]) + s[2 * wo + 1]) * 0.25f;
}

// ---- workspace -----------------------------------------------------------------------------------------------------------
// p = (S / 4)^2 positions of one face at the trunk's resolution.  Floats per face: about 2,000 p (32 MiB at S = 256).
struct Layout {
  size_t m[3];           // the trunk's maps in rotation: 256 p each (m[0] first holds the stem's 64 channels at S / 2)
  size_t wide;           // conv2's output, 128 channels at S / 2: 512 p
  size_t t1, t2;         // a block's first and second convolution without the residual: 256 p, 128 p
  size_t heat;           // 68 p
  size_t q[4][3];        // the hourglass below the trunk, level j at (S / 8) >> j: pooled / low3, low1, low2
  size_t total;
};

bool shape_ok(int B, int S) {
  return B >= 1 && B <= INSTAG_LANDMARKS_MAX_BATCH && S >= INSTAG_LANDMARKS_MIN_SIDE && S <= INSTAG_LANDMARKS_MAX_SIDE &&
         S % INSTAG_LANDMARKS_SIDE_MULTIPLE == 0;
}
constexpr const char* SHAPE_OK = ": 1 <= B <= INSTAG_LANDMARKS_MAX_BATCH, S a multiple of 64 in [64, 512]";

Layout layout(int B, int S) {
  Layout l;
  const size_t p = (size_t)B * (S / 4) * (S / 4);
  Arena a;
  for (int i = 0; i < 3; ++i) l.m[i] = a.take(CH * p);
  l.wide = a.take(512 * p);
  l.t1 = a.take(256 * p);
  l.t2 = a.take(128 * p);
  l.heat = a.take(NPTS * p);
  for (int j = 0; j < 4; ++j)
    for (int k = 0; k < 3; ++k) l.q[j][k] = a.take(CH * (p >> (2 * j + 2)));
  l.total = a.off;
  return l;
}

// ---- the network ---------------------------------------------------------------------------------------------------------
struct Net {
  const instag_landmarks_weights* w;
  int B;
  hipStream_t st;
  float *t1, *t2;
  float* q[4][3];

  // out slice = act(scale conv_ks(pre(in)) + shift + res + up(res2)); e carries res, res2, raw, the slice and relu
  int conv(int layer, int ks, const float* in, int cin, int h, int wd, int cout, float* out, ConvArgs e) const {
    e.in = in; e.wt = w->w[layer]; e.scale = w->scale[layer]; e.shift = w->shift[layer]; e.out = out;
    e.pre_scale = w->pre_scale[layer]; e.pre_shift = w->pre_shift[layer];
    e.B = B; e.cin = e.c_split = cin; e.cout = cout; e.hi = e.ho = h; e.wi = e.wo = wd; e.stride_h = e.stride_w = 1;
    return ks == 1 ? launch_conv_ext<1>(e, st) : launch_conv_ext<3>(e, st);
  }

  // ConvBlock(cin, cout) at h x wd: x -> out (+ res2 at half resolution)
  int block(int layer, const float* x, int cin, int cout, int h, int wd, float* out, const float* res2) const {
    ConvArgs e{};
    e.res = x;
    if (cin != cout) {
      INSTAG_TRY(conv(layer + 3, 1, x, cin, h, wd, cout, out, ConvArgs{}));
      e.res = out;                                                           // read and written by the same thread
    }
    e.res2 = res2; e.out_ch = cout;
    e.raw = t1; e.out_off = 0;
    INSTAG_TRY(conv(layer, 3, x, cin, h, wd, cout / 2, out, e));
    e.raw = t2; e.out_off = cout / 2;
    INSTAG_TRY(conv(layer + 1, 3, t1, cout / 2, h, wd, cout / 4, out, e));
    e.raw = nullptr; e.out_off = 3 * cout / 4;
    return conv(layer + 2, 3, t2, cout / 4, h, wd, cout / 4, out, e);
  }

  // [B ch, 2 ho, 2 wo] -> [B ch, ho, wo]
  int pool(const float* in, float* out, int ch, int ho, int wo) const {
    const size_t n = (size_t)B * ch * ho * wo;
    avgpool_kernel<<<(unsigned)div_up(n, (size_t)TB), TB, 0, st>>>(in, out, n, ho, wo);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  }

  // HourGlass level l (4 .. 1) of the stack whose layers start at `base`: x at h x wd -> out
  int hourglass(int base, int l, const float* x, int h, int wd, float* out) const {
    const int j = 4 - l, hh = h / 2, wh = wd / 2;
    INSTAG_TRY(pool(x, q[j][0], CH, hh, wh));
    INSTAG_TRY(block(base + 6 * j + 3, q[j][0], CH, CH, hh, wh, q[j][1], nullptr));
    if (l > 1) {
      INSTAG_TRY(hourglass(base, l - 1, q[j][1], hh, wh, q[j][2]));
    } else {
      INSTAG_TRY(block(base + S_B2_PLUS, q[j][1], CH, CH, hh, wh, q[j][2], nullptr));
    }
    INSTAG_TRY(block(base + S_B3 + 3 * (l - 1), q[j][2], CH, CH, hh, wh, q[j][0], nullptr));
    return block(base + 6 * j, x, CH, CH, h, wd, out, q[j][0]);
  }
};

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_landmarks_workspace_bytes(int32_t B, int32_t S) {
  if (!shape_ok(B, S)) {
    set_error(std::string("landmarks_workspace_bytes") + SHAPE_OK);
    return 0;
  }
  return layout(B, S).total * sizeof(float);
}

int instag_landmarks_crop(const uint8_t* frames, int32_t N, int32_t H, int32_t W, const float* boxes,
                          const int32_t* frame_index, int32_t B, int32_t S, uint8_t* crops, instag_stream_t stream) {
  INSTAG_REQUIRE(frames && boxes && crops, "landmarks_crop: NULL tensor");
  INSTAG_REQUIRE(shape_ok(B, S), std::string("landmarks_crop") + SHAPE_OK);
  INSTAG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && H <= INSTAG_LANDMARKS_MAX_FRAME && W <= INSTAG_LANDMARKS_MAX_FRAME,
                 "landmarks_crop: N >= 1, H and W in [1, INSTAG_LANDMARKS_MAX_FRAME]");
  INSTAG_REQUIRE(frame_index || N == B, "landmarks_crop: without frame_index there is one frame per box");
  const size_t n = (size_t)B * S * S;
  crop_kernel<<<(unsigned)div_up(n, (size_t)TB), TB, 0, (hipStream_t)stream>>>(frames, N, H, W, boxes, frame_index, B, S,
                                                                              crops);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_landmarks_conv(const float* in, const float* w, const float* scale, const float* shift, const float* pre_scale,
                          const float* pre_shift, const float* res, const float* res2, float* raw, float* out, int32_t B,
                          int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t ks, int32_t out_ch, int32_t out_off,
                          int32_t relu, int32_t tile, instag_stream_t stream) {
  INSTAG_REQUIRE(in && w && scale && shift && out, "landmarks_conv: NULL tensor");
  INSTAG_REQUIRE((pre_scale != nullptr) == (pre_shift != nullptr), "landmarks_conv: pre_scale and pre_shift go together");
  INSTAG_REQUIRE(B >= 1 && B <= INSTAG_LANDMARKS_MAX_BATCH && cin >= 1 && cin <= 1024 && out_ch >= 1 && out_ch <= 1024 &&
                     H >= 1 && H <= 256 && W >= 1 && W <= 256,
                 "landmarks_conv: B in [1, INSTAG_LANDMARKS_MAX_BATCH], cin and out_ch in [1, 1024], H and W in [1, 256]");
  INSTAG_REQUIRE(cout >= 1 && out_off >= 0 && out_off + cout <= out_ch, "landmarks_conv: the slice leaves out_ch");
  INSTAG_REQUIRE(ks == 1 || ks == 3, "landmarks_conv: ks 1 or 3");
  INSTAG_REQUIRE(tile >= 0 && tile <= 2, "landmarks_conv: tile 0, 1 or 2");
  INSTAG_REQUIRE(!res2 || (H % 2 == 0 && W % 2 == 0), "landmarks_conv: res2 needs even H and W");
  ConvArgs e{};
  e.in = in; e.wt = w; e.scale = scale; e.shift = shift; e.pre_scale = pre_scale; e.pre_shift = pre_shift;
  e.res = res; e.res2 = res2; e.raw = raw; e.out = out; e.out_ch = out_ch; e.out_off = out_off; e.relu = relu;
  e.B = B; e.cin = e.c_split = cin; e.cout = cout; e.hi = e.ho = H; e.wi = e.wo = W; e.stride_h = e.stride_w = 1;
  hipStream_t st = (hipStream_t)stream;
  if (tile == 0) return ks == 1 ? launch_conv_ext<1>(e, st) : launch_conv_ext<3>(e, st);
  if (cout <= 32) {
    if (tile == 1) return ks == 1 ? launch_conv_kernel<1, 1, 1, SRC_PLAIN, true>(e, st) : launch_conv_kernel<3, 1, 1, SRC_PLAIN, true>(e, st);
    return ks == 1 ? launch_conv_kernel<1, 1, 2, SRC_PLAIN, true>(e, st) : launch_conv_kernel<3, 1, 2, SRC_PLAIN, true>(e, st);
  }
  if (tile == 1) return ks == 1 ? launch_conv_kernel<1, 2, 1, SRC_PLAIN, true>(e, st) : launch_conv_kernel<3, 2, 1, SRC_PLAIN, true>(e, st);
  return ks == 1 ? launch_conv_kernel<1, 2, 2, SRC_PLAIN, true>(e, st) : launch_conv_kernel<3, 2, 2, SRC_PLAIN, true>(e, st);
}

int instag_landmarks_decode(const float* heatmaps, const float* boxes, int32_t B, int32_t R, float* landmarks,
                            instag_stream_t stream) {
  INSTAG_REQUIRE(heatmaps && boxes && landmarks, "landmarks_decode: NULL tensor");
  INSTAG_REQUIRE(B >= 1 && B <= 65535 && R >= 16 && R <= 128 && R % 16 == 0,
                 "landmarks_decode: B in [1, 65535], R a multiple of 16 in [16, 128]");
  decode_kernel<<<(unsigned)div_up(B * NPTS, TB / 64), TB, 0, (hipStream_t)stream>>>(heatmaps, boxes, B, R, landmarks);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_landmarks_forward(const instag_landmarks_weights* w, const uint8_t* crops, int32_t B, int32_t S,
                             int32_t all_stacks, float* heatmaps, void* workspace, size_t workspace_bytes,
                             instag_stream_t stream) {
  INSTAG_REQUIRE(w && crops && heatmaps && workspace, "landmarks_forward: NULL tensor");
  for (int l = 0; l < NLAYER; ++l) {
    INSTAG_REQUIRE(w->w[l] && w->scale[l] && w->shift[l], "landmarks_forward: NULL weight of layer " + std::to_string(l));
    INSTAG_REQUIRE((w->pre_scale[l] != nullptr) == has_pre(l) && (w->pre_shift[l] != nullptr) == has_pre(l),
                   "landmarks_forward: the pre-activation of layer " + std::to_string(l) + " is missing or unexpected");
  }
  INSTAG_REQUIRE(shape_ok(B, S), std::string("landmarks_forward") + SHAPE_OK);
  const Layout L = layout(B, S);
  if (workspace_bytes < L.total * sizeof(float)) {
    set_error("landmarks_forward: workspace too small");
    return INSTAG_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* base = (float*)workspace;
  Net net{w, B, st, base + L.t1, base + L.t2, {}};
  for (int j = 0; j < 4; ++j)
    for (int k = 0; k < 3; ++k) net.q[j][k] = base + L.q[j][k];
  float* m[3] = {base + L.m[0], base + L.m[1], base + L.m[2]};
  float *wide = base + L.wide, *heat = base + L.heat;
  const int h2 = S / 2, h4 = S / 4;

  // conv1 + bn1 + ReLU on the uint8 crop, then conv2, the pool, conv3, conv4
  {
    ConvArgs c{};
    c.frames = crops; c.unit_table = 1;
    c.wt = w->w[L_CONV1]; c.scale = w->scale[L_CONV1]; c.shift = w->shift[L_CONV1]; c.out = m[0];
    c.B = B; c.cin = c.c_split = 3; c.cout = 64; c.hi = c.wi = S; c.ho = c.wo = h2; c.stride_h = c.stride_w = 2; c.relu = 1;
    INSTAG_TRY((launch_conv_tile<7, 2>(c, st)));
  }
  INSTAG_TRY(net.block(L_CONV2, m[0], 64, 128, h2, h2, wide, nullptr));
  INSTAG_TRY(net.pool(wide, m[1], 128, h4, h4));
  INSTAG_TRY(net.block(L_CONV3, m[1], 128, 128, h4, h4, m[2], nullptr));
  INSTAG_TRY(net.block(L_CONV4, m[2], 128, CH, h4, h4, m[0], nullptr));

  int prev = 0;
  for (int i = 0; i < NSTACK; ++i) {
    const int sb = L_STACK + i * STACK_LAYERS, a = (prev + 1) % 3, b = (prev + 2) % 3;
    INSTAG_TRY(net.hourglass(sb, 4, m[prev], h4, h4, m[a]));
    INSTAG_TRY(net.block(sb + S_TOP, m[a], CH, CH, h4, h4, m[b], nullptr));
    ConvArgs e{};
    e.relu = 1;
    INSTAG_TRY(net.conv(sb + S_LAST, 1, m[b], CH, h4, h4, CH, m[a], e));
    // l{i}: the heatmaps, to the caller and (while a stack follows) to the workspace for al{i}
    ConvArgs hm{};
    float* out = heat;
    if (all_stacks) {
      hm.out_ch = NSTACK * NPTS; hm.out_off = i * NPTS;
      hm.raw = i < NSTACK - 1 ? heat : nullptr;
      out = heatmaps;
    } else if (i == NSTACK - 1) {
      out = heatmaps;
    }
    INSTAG_TRY(net.conv(sb + S_L, 1, m[a], CH, h4, h4, NPTS, out, hm));
    if (i == NSTACK - 1) break;
    // previous + bl{i}(ll) + al{i}(heatmaps), in this order
    ConvArgs r{};
    r.res = m[prev];
    INSTAG_TRY(net.conv(sb + S_BL, 1, m[a], CH, h4, h4, CH, m[b], r));
    r.res = m[b];
    INSTAG_TRY(net.conv(sb + S_AL, 1, heat, NPTS, h4, h4, CH, m[b], r));
    prev = b;
  }
  return INSTAG_OK;
}

}  // extern "C"
