// AudioEncoder of the 'ave' audio extractor (scene/motion_net.py:8-25, 102-129), eval mode, fp32, forward only: thirteen
// blocks ReLU(BN(conv(x) + b) [+ x]) that turn a [1,80,16] mel window into a 512-vector (include/instag_hip.h, "AudioEncoder").
//
// BatchNorm arrives folded into a per-channel (scale, shift) pair (instag_amd/ave_encoder.py: device_pack), so a block
// is relu(scale * conv_nobias(x) + shift [+ x]).
//   layer 0      (1 -> 32, K = 9): VALU, fused with the window gather: it reads mel[T,80] at starts[i] (transposed
//                access), or a stack of [n,1,80,16] windows, so the windows are never materialised.
//   layers 1..10 the convolution kernel of conv_mfma.hpp (plain source, 3 x 3, a stride per axis): D[cout][m] with
//                m = (window, oy, ox) tiled jointly -- from layer 6 on a window has at most 54 pixels and the batch is
//                what fills the tile.  The residual is the layer's own input; two activation buffers alternate.  The
//                tile is 32 x 128 for the 32-channel layers and 64 x 64 for the others.
//   layers 11+12 are 1x1 spatial, [B,2304] x [2304,512] and [B,512] x [512,512]: one launch, a workgroup keeps the 512
//                channels of its 32 windows in LDS between the two products and its weights in registers.
// Every sum is a k-ordered FMA chain per K tile of 32 with the tiles added in order (mfma_tile.hpp: blocked summation),
// there are no atomics, and an output element reads nothing but its own window: a window's 512 values do not depend on the
// batch, the chunk or the tile column it sat in, and two runs give the same bits.
#include "conv_mfma.hpp"

namespace instag {
namespace {

constexpr int NLAYER = 13;
constexpr int MAX_BATCH = 256;
constexpr int MEL = 80, WIN = 16, PIX0 = MEL * WIN;      // a window is [80 bands][16 frames]
constexpr int C0 = 32;                                   // channels of layers 0..2: the largest activation, 32 x 80 x 16

struct LayerDesc { int cin, cout, sh, sw, residual, hi, wi, ho, wo; };
// layers 1..10 (3x3, pad 1); extents for an [80,16] window: floor((h + 2 - 3) / s) + 1
constexpr LayerDesc LAYERS[10] = {
    {32, 32, 1, 1, 1, 80, 16, 80, 16},  {32, 32, 1, 1, 1, 80, 16, 80, 16},  {32, 64, 3, 1, 0, 80, 16, 27, 16},
    {64, 64, 1, 1, 1, 27, 16, 27, 16},  {64, 64, 1, 1, 1, 27, 16, 27, 16},  {64, 128, 3, 3, 0, 27, 16, 9, 6},
    {128, 128, 1, 1, 1, 9, 6, 9, 6},    {128, 128, 1, 1, 1, 9, 6, 9, 6},    {128, 256, 3, 2, 0, 9, 6, 3, 3},
    {256, 256, 1, 1, 1, 3, 3, 3, 3},
};

// ---- layer 0: window gather + 3x3 convolution of one channel, VALU ----------------------------------------------------
struct FirstArgs {
  const float* src;          // mel [T,80] (starts != NULL) or windows [n,1,80,16]
  const int32_t* starts;     // [n] first mel frame of each window, or NULL
  const float* w;            // [32][9]
  const float* scale;
  const float* shift;
  float* out;                // [n,32,80,16]
  int T, n;
};

__global__ void __launch_bounds__(TB) first_layer_kernel(FirstArgs a) {
  __shared__ float ws[C0 * 9], sc[C0], sf[C0];
  for (int i = threadIdx.x; i < C0 * 9; i += TB) ws[i] = a.w[i];
  if (threadIdx.x < C0) { sc[threadIdx.x] = a.scale[threadIdx.x]; sf[threadIdx.x] = a.shift[threadIdx.x]; }
  __syncthreads();
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= a.n * PIX0) return;
  const int b = i / PIX0, pos = i - b * PIX0;
  const int y = pos / WIN, x = pos - y * WIN;            // y: mel band, x: frame of the window
  // window[y][x] = mel[start + x][y], or windows[b][0][y][x]; frames outside [0, T) read as zero (a valid start has none)
  const int st = a.starts ? a.starts[b] : 0;
  float v[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int yy = y + j / 3 - 1, xx = x + j % 3 - 1;
    const bool ok = yy >= 0 && yy < MEL && xx >= 0 && xx < WIN;
    if (a.starts) {
      const int tt = st + xx;
      v[j] = ok && tt >= 0 && tt < a.T ? a.src[(size_t)tt * MEL + yy] : 0.f;
    } else {
      v[j] = ok ? a.src[(size_t)b * PIX0 + yy * WIN + xx] : 0.f;
    }
  }
  float* o = a.out + (size_t)b * C0 * PIX0 + pos;
  for (int c = 0; c < C0; ++c) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 9; ++j) s = fmaf(v[j], ws[c * 9 + j], s);
    o[(size_t)c * PIX0] = fmaxf(fmaf(s, sc[c], sf[c]), 0.f);
  }
}

// ---- layers 11 and 12 in one launch -----------------------------------------------------------------------------------
constexpr int TAIL_TB = 512;                // eight waves of 64 output channels each
constexpr int TAIL_BN = 32;                 // windows per workgroup
constexpr int K11 = 2304, CT = 512;
constexpr int LDS_PAD = 33;
constexpr int TAIL_LDS = (BK + CT) * LDS_PAD * (int)sizeof(float);

struct TailArgs {
  const float* in;      // [B, 2304] = layer 10's [B,256,3,3]
  const float* w11;     // [2304][512]
  const float* s11; const float* h11;
  const float* w12;     // [512][512]
  const float* s12; const float* h12;
  float* out;           // [B, 512]
  int B;
};

__global__ void __launch_bounds__(TAIL_TB) tail_kernel(TailArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float (*Bs)[LDS_PAD] = reinterpret_cast<float (*)[LDS_PAD]>(smem);                     // [BK][33]
  float (*Hs)[LDS_PAD] = reinterpret_cast<float (*)[LDS_PAD]>(smem + BK * LDS_PAD);      // [512][33]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b0 = blockIdx.x * TAIL_BN;
  const int ch0 = wave * 64;
  const int col = lane & 31, half = lane >> 5;
  const int kkb = t & 31, bb = t >> 5;                         // staging of the windows' operand: k fastest

  f32x16 acc[2], part[2];
  float ra[2][BK / 2], rn[2][BK / 2], rb[2];

  auto load_a = [&](const float* w, int kt, float (&r)[2][BK / 2]) {
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j) r[j][kk] = w[(size_t)(kt * BK + kk * 2 + half) * CT + ch0 + j * 32 + col];
  };
  auto load_b = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int b = b0 + bb + 16 * i;
      rb[i] = b < a.B ? a.in[(size_t)b * K11 + kt * BK + kkb] : 0.f;
    }
  };
  auto zero = [](f32x16& v) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
  };

  // layer 11: H[512][32 windows] = relu(scale * W11^T X + shift), kept in LDS
  zero(acc[0]); zero(acc[1]);
  load_a(a.w11, 0, ra);
  load_b(0);
  constexpr int NK11 = K11 / BK;
  for (int kt = 0; kt < NK11; ++kt) {
    __syncthreads();
    Bs[kkb][bb] = rb[0];
    Bs[kkb][bb + 16] = rb[1];
    __syncthreads();
    if (kt + 1 < NK11) { load_a(a.w11, kt + 1, rn); load_b(kt + 1); }
    zero(part[0]); zero(part[1]);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const float bv = Bs[kk * 2 + half][col];
      part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[0][kk], bv, part[0], 0, 0, 0);
      part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[1][kk], bv, part[1], 0, 0, 0);
    }
    acc[0] += part[0];
    acc[1] += part[1];
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) { ra[0][kk] = rn[0][kk]; ra[1][kk] = rn[1][kk]; }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = mfma_row(ch0 + j * 32, r, lane);
      Hs[co][col] = fmaxf(fmaf(acc[j][r], a.s11[co], a.h11[co]), 0.f);
    }
  __syncthreads();

  // layer 12: the windows' operand is H itself
  zero(acc[0]); zero(acc[1]);
  load_a(a.w12, 0, ra);
  constexpr int NK12 = CT / BK;
  for (int kt = 0; kt < NK12; ++kt) {
    if (kt + 1 < NK12) load_a(a.w12, kt + 1, rn);
    zero(part[0]); zero(part[1]);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const float bv = Hs[kt * BK + kk * 2 + half][col];
      part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[0][kk], bv, part[0], 0, 0, 0);
      part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[1][kk], bv, part[1], 0, 0, 0);
    }
    acc[0] += part[0];
    acc[1] += part[1];
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) { ra[0][kk] = rn[0][kk]; ra[1][kk] = rn[1][kk]; }
  }
  const int b = b0 + col;
  if (b >= a.B) return;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = mfma_row(ch0 + j * 32, r, lane);
      a.out[(size_t)b * CT + co] = fmaxf(fmaf(acc[j][r], a.s12[co], a.h12[co]), 0.f);
    }
}

size_t buffer_floats(int batch) { return align_up((size_t)batch * C0 * PIX0, 64); }

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

int instag_ave_encoder_max_batch(void) { return MAX_BATCH; }

size_t instag_ave_encoder_workspace_bytes(int32_t batch) {
  if (batch < 1 || batch > MAX_BATCH) {
    set_error("ave_encoder_workspace_bytes: batch must be in [1, instag_ave_encoder_max_batch()]");
    return 0;
  }
  return 2 * buffer_floats(batch) * sizeof(float);
}

int instag_ave_encoder_forward(const instag_ave_encoder_weights* w, const float* mel, int32_t T,
                               const int32_t* starts_dev, int32_t n, float* out, void* workspace,
                               size_t workspace_bytes, instag_stream_t stream) {
  INSTAG_REQUIRE(w && mel && out && workspace, "ave_encoder_forward: NULL tensor");
  for (int l = 0; l < NLAYER; ++l)
    INSTAG_REQUIRE(w->w[l] && w->scale[l] && w->shift[l], "ave_encoder_forward: NULL weight of layer " + std::to_string(l));
  INSTAG_REQUIRE(n >= 1 && n <= MAX_BATCH, "ave_encoder_forward: n must be in [1, instag_ave_encoder_max_batch()]");
  INSTAG_REQUIRE(!starts_dev || (T >= WIN && T <= (1 << 24)), "ave_encoder_forward: a mel of fewer than 16 frames holds no window");
  INSTAG_REQUIRE(workspace_bytes >= 2 * buffer_floats(n) * sizeof(float), "ave_encoder_forward: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* buf[2] = {(float*)workspace, (float*)workspace + buffer_floats(n)};

  FirstArgs f{mel, starts_dev, w->w[0], w->scale[0], w->shift[0], buf[0], T, n};
  first_layer_kernel<<<(unsigned)div_up(n * PIX0, TB), TB, 0, st>>>(f);
  INSTAG_CHECK_LAUNCH();

  int cur = 0;
  for (int l = 1; l <= 10; ++l) {
    const LayerDesc& d = LAYERS[l - 1];
    ConvArgs c{};
    c.in = buf[cur]; c.wt = w->w[l]; c.scale = w->scale[l]; c.shift = w->shift[l]; c.out = buf[cur ^ 1];
    c.res = d.residual ? buf[cur] : nullptr;                     // cin == cout and the extents are kept
    c.B = n; c.cin = c.c_split = d.cin; c.cout = d.cout; c.hi = d.hi; c.wi = d.wi; c.ho = d.ho; c.wo = d.wo;
    c.stride_h = d.sh; c.stride_w = d.sw; c.relu = 1;
    // 32 x 128 where cout == 32 (64 rows would idle half the MFMAs on the two largest activations), else 64 x 64
    if (d.cout == 32) {
      INSTAG_TRY((launch_conv_kernel<3, 1, 1, SRC_PLAIN>(c, st)));
    } else {
      INSTAG_TRY((launch_conv_kernel<3, 2, 1, SRC_PLAIN>(c, st)));
    }
    cur ^= 1;
  }

  if (int rc = set_max_dynamic_lds((const void*)tail_kernel, TAIL_LDS)) return rc;
  TailArgs ta{buf[cur], w->w[11], w->scale[11], w->shift[11], w->w[12], w->scale[12], w->shift[12], out, n};
  tail_kernel<<<(unsigned)div_up(n, TAIL_BN), TAIL_TB, TAIL_LDS, st>>>(ta);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
