// Face parsing (data_utils/face_parsing/test.py:72-106, model.py, resnet.py): BiSeNet(19) over ResNet-18 in eval mode,
// fp32, forward only, from uint8 frames to labels and the colour map of parsing/<i>.png (include/instag_hip.h, "Face
// parsing").
//
// BatchNorm arrives folded into a per-channel (scale, shift) pair (instag_amd/convnet.py: device_pack), so a
// convolution block is act(scale * conv(x) + shift [+ residual]).
//   convolutions  conv_mfma.hpp (shared with teeth.hip): implicit GEMM on the f32-input MFMA (v_mfma_f32_32x32x2_f32):
//                 D[cout][m] with m = (frame, oy, ox) tiled jointly -- at 1/32 resolution a frame has a few hundred
//                 positions and the batch is what fills the tile -- and k = (cin, ky, kx) gathered from NCHW activations.
//                 Four waves of one or two accumulators of 32 x 32 each; scale, shift, the residual read and the ReLU are
//                 applied to the accumulator registers.  The tile is chosen per launch to fill the chip and does not
//                 enter the arithmetic.
//   the stem      7 x 7, stride 2, K = 147 padded to 160: the same kernel, its gather reads the uint8 HWC frame through
//                 a 3 x 256 table of (u / 255 - mean) / std built in LDS (the padding is zero AFTER normalisation, so
//                 the normalisation is not folded into the weights); no fp32 input tensor exists.
//   data movement the nearest x2 upsample, the channel attention and the broadcast / spatial add in front of
//                 conv_head32 / conv_head16 (in[c][y >> 1][x >> 1] * att[c] + add), the cat of ffm (two pointers) and
//                 feat * a + feat in front of conv_out are part of the consumer's gather.
//   pools         the four global average pools are one wave per (frame, channel): 64 strided partial sums in index
//                 order, then a fixed xor tree.  The [B,C] products and sigmoids behind them are one wave per output, summed alike.
//   final stage   one thread per output pixel: the align_corners bilinear interpolation of the 19 logits at 1/8
//                 resolution, the first-maximum argmax, the colour table, the nearest resize.
// Every sum is a k-ordered FMA chain per K tile of 32 with the tiles added in order, there are no atomics, and an output
// element reads nothing but its own frame: a frame's outputs do not depend on the batch, the chunk or the tile it sat
// in, and two runs give the same bits.
#include "common.hpp"
#include "conv_net.hpp"

namespace instag {
namespace {

constexpr int NLAYER = 32;
constexpr int NCLS = 19;

// order of instag_parsing_weights (instag_amd/parsing.py: LAYERS)
enum Layer {
  L_STEM = 0, L_LAYER1 = 1, L_LAYER2 = 5, L_LAYER3 = 10, L_LAYER4 = 15, L_ARM32 = 20, L_ARM16 = 21, L_HEAD32 = 22,
  L_HEAD16 = 23, L_FFM = 24, L_OUT_MID = 25, L_OUT = 26, L_AVG = 27, L_ATT32 = 28, L_ATT16 = 29, L_FFM1 = 30, L_FFM2 = 31,
};

// ---- global average pool: one wave per (frame, channel) ------------------------------------------------------------------
__global__ void __launch_bounds__(TB) pool_kernel(const float* in, float* out, int planes, int n) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  if (p >= planes) return;                                     // whole waves leave together
  const float* src = in + (size_t)p * n;
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s += src[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) out[p] = s / (float)n;
}

// ---- [B, cin] x [cout, cin]^T: one wave per output -------------------------------------------------------------------------
enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2 };

// wt [cout][cin]; 64 strided partial FMA chains in index order, then a fixed xor tree
__global__ void __launch_bounds__(TB) fc_kernel(const float* in, const float* wt, const float* scale, const float* shift,
                                                float* out, int B, int cin, int cout, int act) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  if (i >= B * cout) return;                                   // whole waves leave together
  const int b = i / cout, co = i - b * cout;
  const float* x = in + (size_t)b * cin;
  const float* wrow = wt + (size_t)co * cin;
  float s = 0.f;
  for (int k = lane; k < cin; k += 64) s = fmaf(x[k], wrow[k], s);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (lane != 0) return;
  float v = fmaf(s, scale[co], shift[co]);
  if (act == ACT_RELU) v = fmaxf(v, 0.f);
  if (act == ACT_SIGMOID) v = 1.f / (1.f + expf(-v));
  out[i] = v;
}

// ---- upsample + argmax + colour table + resize ----------------------------------------------------------------------------
__device__ inline void colour_of(int c, uint8_t* rgb) {
  uint8_t r = 0, g = 0, b = 255;                                // head: 1-10, 12, 13, 18
  if (c == 0) { r = 255; g = 255; }
  else if (c == 11) { r = 100; g = 100; b = 100; }
  else if (c == 14 || c == 15) { g = 255; b = 0; }
  else if (c == 16) { r = 255; b = 0; }
  else if (c == 17) { b = 0; }
  rgb[0] = r; rgb[1] = g; rgb[2] = b;
}

// logits [B,19,h8,w8] -> for every pixel of the [B,oh,ow] grid the label of source pixel (min(y H / oh, H - 1), ...)
__global__ void __launch_bounds__(TB) label_kernel(const float* logits, int B, int H, int W, int h8, int w8, int oh,
                                                   int ow, uint8_t* labels, uint8_t* colours) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)B * oh * ow) return;
  const int x = (int)(i % ow), y = (int)((i / ow) % oh);
  const int b = (int)(i / ((size_t)ow * oh));
  const int py = min((int)(((int64_t)y * H) / oh), H - 1), px = min((int)(((int64_t)x * W) / ow), W - 1);
  const int arg = bilinear_argmax<true>(logits + (size_t)b * NCLS * h8 * w8, NCLS, h8, w8, H, W, py, px);
  if (labels) labels[i] = (uint8_t)arg;
  if (colours) colour_of(arg, colours + i * 3);
}

int launch_labels(const float* logits, int B, int H, int W, int oh, int ow, uint8_t* labels, uint8_t* colours,
                  hipStream_t st) {
  // labels live on the [H,W] grid, colours on [oh,ow]: one launch when the two coincide
  if (labels && colours && oh == H && ow == W) {
    label_kernel<<<(unsigned)div_up((size_t)B * H * W, (size_t)TB), TB, 0, st>>>(logits, B, H, W, H / 8, W / 8, H, W, labels,
                                                                               colours);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  }
  if (labels) {
    label_kernel<<<(unsigned)div_up((size_t)B * H * W, (size_t)TB), TB, 0, st>>>(logits, B, H, W, H / 8, W / 8, H, W, labels,
                                                                               nullptr);
    INSTAG_CHECK_LAUNCH();
  }
  if (colours) {
    label_kernel<<<(unsigned)div_up((size_t)B * oh * ow, (size_t)TB), TB, 0, st>>>(logits, B, H, W, H / 8, W / 8, oh, ow,
                                                                                 nullptr, colours);
    INSTAG_CHECK_LAUNCH();
  }
  return INSTAG_OK;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------
struct Layout {
  size_t stem, tmp[3], feat8, feat16, feat32;
  // behind the max-pool nothing reads the stem's output: these share its room
  size_t arm32, arm16, cp16, cp8, fuse, mid, logits;
  size_t pool32, avg, parm32, att32, parm16, att16, pffm, hid, attffm;
  size_t total;                                                // floats
};

Layout layout(int B, int H, int W) {
  Layout l;
  const size_t b = (size_t)B;
  const size_t p2 = (size_t)(H / 2) * (W / 2), p4 = p2 / 4, p8 = p4 / 4, p16 = p8 / 4, p32 = p16 / 4;
  Arena a;
  l.stem = a.take(b * 64 * p2);
  const size_t after_stem = a.off;
  a.off = l.stem;
  l.arm32 = a.take(b * 128 * p32);
  l.arm16 = a.take(b * 128 * p16);
  l.cp16 = a.take(b * 128 * p16);
  l.cp8 = a.take(b * 128 * p8);
  l.fuse = a.take(b * 256 * p8);
  l.mid = a.take(b * 256 * p8);
  l.logits = a.take(b * NCLS * p8);
  a.off = std::max(a.off, after_stem);                             // (they fit: 19.5 p4 + ... < 256 p4)
  for (int i = 0; i < 3; ++i) l.tmp[i] = a.take(b * 64 * p4);
  l.feat8 = a.take(b * 128 * p8);
  l.feat16 = a.take(b * 256 * p16);
  l.feat32 = a.take(b * 512 * p32);
  l.pool32 = a.take(b * 512);
  l.avg = a.take(b * 128);
  l.parm32 = a.take(b * 128);
  l.att32 = a.take(b * 128);
  l.parm16 = a.take(b * 128);
  l.att16 = a.take(b * 128);
  l.pffm = a.take(b * 256);
  l.hid = a.take(b * 64);
  l.attffm = a.take(b * 256);
  l.total = a.off;
  return l;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_parsing_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (!frames_ok(B, H, W)) {
    set_error(std::string("parsing_workspace_bytes") + FRAMES_OK);
    return 0;
  }
  return layout(B, H, W).total * sizeof(float);
}

int instag_parsing_labels(const float* logits8, int32_t B, int32_t H, int32_t W, int32_t out_h, int32_t out_w,
                          uint8_t* labels, uint8_t* colours, instag_stream_t stream) {
  INSTAG_REQUIRE(logits8 && (labels || colours), "parsing_labels: NULL tensor");
  INSTAG_REQUIRE(B >= 1 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && H <= 4096 && W <= 4096 && B <= 65535,
                 "parsing_labels: B in [1, 65535], H and W multiples of 8 in [8, 4096]");
  INSTAG_REQUIRE(!colours || (out_h >= 1 && out_w >= 1 && out_h <= 8192 && out_w <= 8192),
                 "parsing_labels: out_h and out_w in [1, 8192]");
  return launch_labels(logits8, B, H, W, out_h, out_w, labels, colours, (hipStream_t)stream);
}

int instag_parsing_forward(const instag_parsing_weights* w, const uint8_t* frames, int32_t B, int32_t H, int32_t W,
                           int32_t out_h, int32_t out_w, float* logits8, uint8_t* labels, uint8_t* colours,
                           void* workspace, size_t workspace_bytes, instag_stream_t stream) {
  INSTAG_REQUIRE(w && frames && workspace, "parsing_forward: NULL tensor");
  INSTAG_REQUIRE(logits8 || labels || colours, "parsing_forward: no output asked for");
  const ConvNet conv{w->w, w->scale, w->shift, B, (hipStream_t)stream};
  const int null_layer = conv.null_layer(NLAYER);
  INSTAG_REQUIRE(null_layer < 0, "parsing_forward: NULL weight of layer " + std::to_string(null_layer));
  INSTAG_REQUIRE(frames_ok(B, H, W), std::string("parsing_forward") + FRAMES_OK);
  INSTAG_REQUIRE(!colours || (out_h >= 1 && out_w >= 1 && out_h <= 8192 && out_w <= 8192),
                 "parsing_forward: out_h and out_w in [1, 8192]");
  const Layout L = layout(B, H, W);
  if (workspace_bytes < L.total * sizeof(float)) {
    set_error("parsing_forward: workspace too small");
    return INSTAG_E_SPACE;
  }
  hipStream_t st = conv.st;
  float* base = (float*)workspace;
  auto at = [&](size_t off) { return base + off; };
  const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8, h16 = H / 16, w16 = W / 16,
            h32 = H / 32, w32 = W / 32;


  // the stem and the max-pool
  {
    ConvArgs e{};
    e.frames = frames;
    INSTAG_TRY(conv(L_STEM, 7, nullptr, 3, H, W, 2, 64, at(L.stem), nullptr, 1, e));
    INSTAG_TRY(conv.maxpool(at(L.stem), at(L.tmp[0]), 64, h2, w2));
  }

  // the eight residual blocks: relu(shortcut + bn2(conv2(relu(bn1(conv1 x)))))
  float* tmp[3] = {at(L.tmp[0]), at(L.tmp[1]), at(L.tmp[2])};
  auto pick = [&](const float* a0, const float* a1, const float* a2) -> float* {
    for (float* t : tmp)
      if (t != a0 && t != a1 && t != a2) return t;
    return nullptr;
  };
  const float* x = tmp[0];
  int layer = L_LAYER1, ch = 64, hx = h4, wx = w4;
  float* const stage_out[4] = {nullptr, at(L.feat8), at(L.feat16), at(L.feat32)};
  for (int stage = 0; stage < 4; ++stage) {
    const int cout = 64 << stage;
    for (int blk = 0; blk < 2; ++blk) {
      const bool down = blk == 0 && stage > 0;
      const int stride = down ? 2 : 1;
      const int ho = hx / stride, wo = wx / stride;
      float* t1 = pick(x, nullptr, nullptr);
      INSTAG_TRY(conv(layer, 3, x, ch, hx, wx, stride, cout, t1, nullptr, 1));
      const float* res = x;
      float* out;
      if (down) {
        float* t2 = pick(x, t1, nullptr);
        INSTAG_TRY(conv(layer + 2, 1, x, ch, hx, wx, 2, cout, t2, nullptr, 0));
        res = t2;
        out = pick(t1, t2, nullptr);                           // x itself is not read again
      } else {
        out = pick(x, t1, nullptr);
      }
      if (blk == 1 && stage_out[stage]) out = stage_out[stage];
      INSTAG_TRY(conv(layer + 1, 3, t1, cout, ho, wo, 1, cout, out, res, 1));
      layer += down ? 3 : 2;
      x = out; ch = cout; hx = ho; wx = wo;
    }
  }
  const float *feat8 = at(L.feat8), *feat16 = at(L.feat16), *feat32 = at(L.feat32);

  auto pool = [&](const float* in, float* out, int planes, int n) -> int {
    pool_kernel<<<(unsigned)div_up(planes, TB / 64), TB, 0, st>>>(in, out, planes, n);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  };
  auto fc = [&](int l, const float* in, float* out, int cin, int cout, int act) -> int {
    fc_kernel<<<(unsigned)div_up(B * cout, TB / 64), TB, 0, st>>>(in, w->w[l], w->scale[l], w->shift[l], out, B, cin, cout, act);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  };

  // context path
  INSTAG_TRY(pool(feat32, at(L.pool32), B * 512, h32 * w32));
  INSTAG_TRY(fc(L_AVG, at(L.pool32), at(L.avg), 512, 128, ACT_RELU));
  INSTAG_TRY(conv(L_ARM32, 3, feat32, 512, h32, w32, 1, 128, at(L.arm32), nullptr, 1));
  INSTAG_TRY(pool(at(L.arm32), at(L.parm32), B * 128, h32 * w32));
  INSTAG_TRY(fc(L_ATT32, at(L.parm32), at(L.att32), 128, 128, ACT_SIGMOID));
  {
    ConvArgs e{};
    e.up = 1; e.mul = at(L.att32); e.add_bc = at(L.avg);
    INSTAG_TRY(conv(L_HEAD32, 3, at(L.arm32), 128, h16, w16, 1, 128, at(L.cp16), nullptr, 1, e));
  }
  INSTAG_TRY(conv(L_ARM16, 3, feat16, 256, h16, w16, 1, 128, at(L.arm16), nullptr, 1));
  INSTAG_TRY(pool(at(L.arm16), at(L.parm16), B * 128, h16 * w16));
  INSTAG_TRY(fc(L_ATT16, at(L.parm16), at(L.att16), 128, 128, ACT_SIGMOID));
  {
    ConvArgs e{};
    e.up = 1; e.mul = at(L.att16); e.add_sp = at(L.cp16);
    INSTAG_TRY(conv(L_HEAD16, 3, at(L.arm16), 128, h8, w8, 1, 128, at(L.cp8), nullptr, 1, e));
  }

  // feature fusion and the output head
  {
    ConvArgs e{};
    e.in2 = at(L.cp8); e.c_split = 128;
    INSTAG_TRY(conv(L_FFM, 1, feat8, 256, h8, w8, 1, 256, at(L.fuse), nullptr, 1, e));
  }
  INSTAG_TRY(pool(at(L.fuse), at(L.pffm), B * 256, h8 * w8));
  INSTAG_TRY(fc(L_FFM1, at(L.pffm), at(L.hid), 256, 64, ACT_RELU));
  INSTAG_TRY(fc(L_FFM2, at(L.hid), at(L.attffm), 64, 256, ACT_SIGMOID));
  {
    ConvArgs e{};
    e.mul = at(L.attffm); e.self_add = 1;
    INSTAG_TRY(conv(L_OUT_MID, 3, at(L.fuse), 256, h8, w8, 1, 256, at(L.mid), nullptr, 1, e));
  }
  float* logits = logits8 ? logits8 : at(L.logits);
  INSTAG_TRY(conv(L_OUT, 1, at(L.mid), 256, h8, w8, 1, NCLS, logits, nullptr, 0));

  if (labels || colours) return launch_labels(logits, B, H, W, out_h, out_w, labels, colours, st);
  return INSTAG_OK;
}

}  // extern "C"
