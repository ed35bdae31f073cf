// Teeth segmentation (data_utils/easyportrait/create_teeth_mask.py with the fpn-fp config; the vendored mmseg's
// backbones/resnet.py, necks/fpn.py, decode_heads/fpn_head.py, segmentors/encoder_decoder.py): ResNetV1c-50, FPN and
// FPNHead in eval mode, fp32, forward only, from uint8 frames to the labels and the teeth mask of teeth_mask/<i>.npy
// (include/instag_hip.h, "Teeth segmentation").
//
// BatchNorm arrives folded into a per-channel (scale, shift) pair and a bias as (1, bias) (instag_amd/convnet.py:
// device_pack), so every one of the 71 convolutions is act(scale * conv(x) + shift [+ residual]).
//   convolutions  conv_mfma.hpp, the kernel parsing.hip runs: implicit GEMM on the f32-input MFMA, D[cout][m] with
//                 m = (frame, oy, ox) tiled jointly, K tiles of 32 added in order, the epilogue on the accumulators.
//   the stem      3 x 3, stride 2, K = 27 padded to 32: the gather reads the uint8 HWC frame through a 3 x 256 table of
//                 (u - mean) / std built in LDS (the padding is zero AFTER normalisation); no fp32 input tensor exists.
//   bottlenecks   relu(bn3(conv3(..)) + identity) is the residual read of conv3's epilogue.
//   the neck      the top-down path lat[i-1] += nearest_x2(lat[i]) is the lateral 1 x 1 convolution's epilogue reading
//                 its residual at half resolution, the laterals run in order 3, 2, 1, 0.
//   the head      the x2 bilinear upsamples (align_corners = False: source (dst + 0.5) / 2 - 0.5 clamped at 0, weights
//                 1/4 and 3/4) are one small kernel of their own -- a bilinear gather inside the 3 x 3 convolution would
//                 read four values per tap --, and the last upsample of a level adds its result to the running sum of
//                 the levels in the same pass, in level order 0, 1, 2, 3.
//   final stage   one thread per output pixel: the bilinear interpolation (align_corners = False) of the C logits at 1/4
//                 resolution, the first-maximum argmax, the label and / or label == 7.
// Every sum is a k-ordered FMA chain per K tile of 32 with the tiles added in order, there are no atomics, and an output
// element reads nothing but its own frame: a frame's outputs do not depend on the batch, the chunk or the tile it sat
// in, and two runs give the same bits.
#include "common.hpp"
#include "conv_net.hpp"

namespace instag {
namespace {

constexpr int NLAYER = 71;
constexpr int MIN_CLS = 8, MAX_CLS = 32;
constexpr int TEETH = 7;
constexpr float MEAN[3] = {143.55267075f, 132.96705975f, 126.94924335f};
constexpr float STDEV[3] = {60.2625333f, 60.32740275f, 59.30988645f};
constexpr int BLOCKS[4] = {3, 4, 6, 3};

// order of instag_teeth_weights (instag_amd/teeth.py: LAYERS)
enum Layer { L_STEM = 0, L_LAYER1 = 3, L_LATERAL = 55, L_FPN = 59, L_HEAD = 63, L_SEG = 70 };

// ---- x2 bilinear upsample (align_corners = False), optionally added to `add` -------------------------------------------
// in [planes, h, w] -> out [planes, 2h, 2w] = (add ? add : 0) + up(in); out may be add
__global__ void __launch_bounds__(TB) upsample2_kernel(const float* in, const float* add, float* out, int planes, int h,
                                                       int w) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  const int ho = 2 * h, wo = 2 * w;
  if (i >= (size_t)planes * ho * wo) return;
  const int x = (int)(i % wo), y = (int)((i / wo) % ho);
  const size_t p = i / ((size_t)wo * ho);
  const float fy = fmaxf(0.5f * (float)y - 0.25f, 0.f), fx = fmaxf(0.5f * (float)x - 0.25f, 0.f);
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float* src = in + p * h * w;
  const float v = hy * (hx * src[y0 * w + x0] + lx * src[y0 * w + x1]) + ly * (hx * src[y1 * w + x0] + lx * src[y1 * w + x1]);
  out[i] = add ? add[i] + v : v;
}

// ---- upsample + argmax -----------------------------------------------------------------------------------------------
// logits [B,C,h4,w4] -> labels and / or mask [B,H,W]
__global__ void __launch_bounds__(TB) teeth_label_kernel(const float* logits, int B, int H, int W, int C, int h4, int w4,
                                                         uint8_t* labels, uint8_t* mask) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)B * H * W) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const int b = (int)(i / ((size_t)W * H));
  const int arg = bilinear_argmax<false>(logits + (size_t)b * C * h4 * w4, C, h4, w4, H, W, y, x);
  if (labels) labels[i] = (uint8_t)arg;
  if (mask) mask[i] = arg == TEETH ? 1 : 0;
}

int launch_labels(const float* logits, int B, int H, int W, int C, uint8_t* labels, uint8_t* mask, hipStream_t st) {
  teeth_label_kernel<<<(unsigned)div_up((size_t)B * H * W, (size_t)TB), TB, 0, st>>>(logits, B, H, W, C, H / 4, W / 4,
                                                                                    labels, mask);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------
// p4 = (H / 4) (W / 4) positions of one frame at stride 4.  Floats per frame: 1600 p4 (100 MiB at 512 x 512).
struct Layout {
  size_t stem_a, stem_b, stem_c;     // the stem's 32, 32 and 64 channels at stride 2: 128, 128, 256 p4
  size_t pool;                       // 64 p4
  size_t big[2];                     // with stem_c the three block outputs in flight: 256 p4 each
  size_t feat[4];                    // the stage outputs: 256, 128, 64, 32 p4
  size_t logits;                     // 32 p4
  // behind the max-pool stem_a / stem_b hold a bottleneck's conv1 / conv2 outputs (at most 128 p4); behind the backbone
  // stem_c and big[0] hold the laterals, big[1] and stem_a the neck's outputs, stem_b the head's sum, pool its temporaries
  size_t total;                      // floats
};

Layout layout(int B, int H, int W) {
  Layout l;
  const size_t bp4 = (size_t)B * (H / 4) * (W / 4);
  Arena a;
  l.stem_a = a.take(128 * bp4);
  l.stem_b = a.take(128 * bp4);
  l.stem_c = a.take(256 * bp4);
  l.pool = a.take(64 * bp4);
  l.big[0] = a.take(256 * bp4);
  l.big[1] = a.take(256 * bp4);
  for (int s = 0; s < 4; ++s) l.feat[s] = a.take((256 >> s) * bp4);
  l.logits = a.take(MAX_CLS * bp4);
  l.total = a.off;
  return l;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_teeth_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (!frames_ok(B, H, W)) {
    set_error(std::string("teeth_workspace_bytes") + FRAMES_OK);
    return 0;
  }
  return layout(B, H, W).total * sizeof(float);
}

int instag_teeth_labels(const float* logits4, int32_t B, int32_t H, int32_t W, int32_t C, uint8_t* labels, uint8_t* mask,
                        instag_stream_t stream) {
  INSTAG_REQUIRE(logits4 && (labels || mask), "teeth_labels: NULL tensor");
  INSTAG_REQUIRE(B >= 1 && H >= 4 && W >= 4 && H % 4 == 0 && W % 4 == 0 && H <= 4096 && W <= 4096 && B <= 65535,
                 "teeth_labels: B in [1, 65535], H and W multiples of 4 in [4, 4096]");
  INSTAG_REQUIRE(C >= MIN_CLS && C <= MAX_CLS, "teeth_labels: C in [8, 32]");
  return launch_labels(logits4, B, H, W, C, labels, mask, (hipStream_t)stream);
}

int instag_teeth_forward(const instag_teeth_weights* w, const uint8_t* frames, int32_t B, int32_t H, int32_t W, int32_t C,
                         float* logits4, uint8_t* labels, uint8_t* mask, void* workspace, size_t workspace_bytes,
                         instag_stream_t stream) {
  INSTAG_REQUIRE(w && frames && workspace, "teeth_forward: NULL tensor");
  INSTAG_REQUIRE(logits4 || labels || mask, "teeth_forward: no output asked for");
  const ConvNet conv{w->w, w->scale, w->shift, B, (hipStream_t)stream};
  const int null_layer = conv.null_layer(NLAYER);
  INSTAG_REQUIRE(null_layer < 0, "teeth_forward: NULL weight of layer " + std::to_string(null_layer));
  INSTAG_REQUIRE(frames_ok(B, H, W), std::string("teeth_forward") + FRAMES_OK);
  INSTAG_REQUIRE(C >= MIN_CLS && C <= MAX_CLS, "teeth_forward: C in [8, 32]");
  const Layout L = layout(B, H, W);
  if (workspace_bytes < L.total * sizeof(float)) {
    set_error("teeth_forward: workspace too small");
    return INSTAG_E_SPACE;
  }
  hipStream_t st = conv.st;
  float* base = (float*)workspace;
  auto at = [&](size_t off) { return base + off; };
  const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4;
  const size_t bp4 = (size_t)B * h4 * w4;

  auto up2 = [&](const float* in, const float* add, float* out, int ch, int h, int wd) -> int {
    const size_t n = (size_t)B * ch * h * wd * 4;
    upsample2_kernel<<<(unsigned)div_up(n, (size_t)TB), TB, 0, st>>>(in, add, out, B * ch, h, wd);
    INSTAG_CHECK_LAUNCH();
    return INSTAG_OK;
  };

  // the deep stem and the max-pool
  {
    ConvArgs e{};
    e.frames = frames;
    for (int c = 0; c < 3; ++c) { e.mean[c] = MEAN[c]; e.stdev[c] = STDEV[c]; }
    INSTAG_TRY(conv(L_STEM, 3, nullptr, 3, H, W, 2, 32, at(L.stem_a), nullptr, 1, e));
    INSTAG_TRY(conv(L_STEM + 1, 3, at(L.stem_a), 32, h2, w2, 1, 32, at(L.stem_b), nullptr, 1));
    INSTAG_TRY(conv(L_STEM + 2, 3, at(L.stem_b), 32, h2, w2, 1, 64, at(L.stem_c), nullptr, 1));
    INSTAG_TRY(conv.maxpool(at(L.stem_c), at(L.pool), 64, h2, w2));
  }

  // the sixteen bottlenecks: relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + identity), the stride on conv2
  float* big[3] = {at(L.stem_c), at(L.big[0]), at(L.big[1])};
  auto pick = [&](const float* a0, const float* a1) -> float* {
    for (float* t : big)
      if (t != a0 && t != a1) return t;
    return nullptr;
  };
  float *mid1 = at(L.stem_a), *mid2 = at(L.stem_b);
  const float* x = at(L.pool);
  int layer = L_LAYER1, ch = 64, hx = h4, wx = w4;
  for (int stage = 0; stage < 4; ++stage) {
    const int planes = 64 << stage, cout = 4 * planes;
    for (int blk = 0; blk < BLOCKS[stage]; ++blk) {
      const int stride = blk == 0 && stage > 0 ? 2 : 1;
      const int ho = hx / stride, wo = wx / stride;
      INSTAG_TRY(conv(layer, 1, x, ch, hx, wx, 1, planes, mid1, nullptr, 1));
      INSTAG_TRY(conv(layer + 1, 3, mid1, planes, hx, wx, stride, planes, mid2, nullptr, 1));
      const float* res = x;
      if (blk == 0) {
        float* down = pick(x, nullptr);
        INSTAG_TRY(conv(layer + 3, 1, x, ch, hx, wx, stride, cout, down, nullptr, 0));
        res = down;
      }
      float* out = blk == BLOCKS[stage] - 1 ? at(L.feat[stage]) : pick(x, res);
      INSTAG_TRY(conv(layer + 2, 1, mid2, planes, ho, wo, 1, cout, out, res, 1));
      layer += blk == 0 ? 4 : 3;
      x = out; ch = cout; hx = ho; wx = wo;
    }
  }

  // the neck: laterals top-down (level i - 1 reads the finished level i at half resolution), then the 3 x 3 convolutions
  float* lat[4] = {at(L.stem_c), at(L.big[0]), at(L.big[0]) + 64 * bp4, at(L.big[0]) + 80 * bp4};
  float* fpn[4] = {at(L.big[1]), at(L.stem_a), at(L.stem_a) + 64 * bp4, at(L.stem_a) + 80 * bp4};
  for (int i = 3; i >= 0; --i) {
    ConvArgs e{};
    e.res_up = i < 3;
    INSTAG_TRY(conv(L_LATERAL + i, 1, at(L.feat[i]), 256 << i, h4 >> i, w4 >> i, 1, 256, lat[i], i < 3 ? lat[i + 1] : nullptr,
                   0, e));
  }
  for (int i = 0; i < 4; ++i)
    INSTAG_TRY(conv(L_FPN + i, 3, lat[i], 256, h4 >> i, w4 >> i, 1, 256, fpn[i], nullptr, 0));

  // the head: level i runs max(1, i) times (conv + BN + ReLU [+ x2 upsample]); the levels are summed in order at stride 4
  float* sum = at(L.stem_b);
  float *t0 = at(L.pool), *t1 = at(L.pool) + 32 * bp4;
  INSTAG_TRY(conv(L_HEAD, 3, fpn[0], 256, h4, w4, 1, 128, sum, nullptr, 1));
  int hl = L_HEAD + 1;
  for (int i = 1; i < 4; ++i) {
    const float* in = fpn[i];
    int cin = 256, h = h4 >> i, wd = w4 >> i;
    for (int k = 0; k < i; ++k) {
      INSTAG_TRY(conv(hl++, 3, in, cin, h, wd, 1, 128, t0, nullptr, 1));
      if (k == i - 1) {
        INSTAG_TRY(up2(t0, sum, sum, 128, h, wd));
      } else {
        INSTAG_TRY(up2(t0, nullptr, t1, 128, h, wd));
      }
      in = t1; cin = 128; h *= 2; wd *= 2;
    }
  }
  float* logits = logits4 ? logits4 : at(L.logits);
  INSTAG_TRY(conv(L_SEG, 1, sum, 128, h4, w4, 1, C, logits, nullptr, 0));

  if (labels || mask) return launch_labels(logits, B, H, W, C, labels, mask, st);
  return INSTAG_OK;
}

}  // extern "C"
