// Sapiens normal / depth network (include/instag_sapiens.h), fp32, forward only: uint8 frames -> [B, C, H, W].
//
// The backbone is the transformer of transformer.hpp (the layer loop HuBERT and wav2vec run, LayerNorm eps 1e-6) with
// the streaming-softmax attention of flash_attention.hpp at 3072 tokens.  This file's own part:
//
//   patch_rows_kernel   reads the uint8 frame, resizes it to the network's input on exact integers, normalises and
//                       writes the token-major patch rows [B T][768]; the Conv2d's padding of 2 is the value 0.  The
//                       projection is then one GEMM per frame (K = 768) with pos_embed as the epilogue's residual.
//   deconv              ConvTranspose2d(4, 2, 1) as its four output phases.  Output pixel (2 m + py, 2 n + px) takes the
//                       inputs (m + py - 1 + v, n + px - 1 + u), u, v in {0, 1}, under the weights
//                       (3 - py - 2 v, 3 - px - 2 u).  Over a zero-bordered NHWC copy P the two horizontal taps are
//                       2 cin contiguous floats, so a phase's vertical tap v is ONE GEMM over overlapping rows (a "batch"
//                       is a row m of the map: a_batch = (w + 2) cin, lda = cin, K = 2 cin) that writes every second
//                       pixel of every second output row (d_batch = 2 rows, ldd = 2 cout); v = 1 adds to v = 0 through
//                       the residual.  Eight launches per frame and layer, nothing gathered, no column buffer: the
//                       alternative, one GEMM to 16 cout columns and a gather, needs 16 cout floats per INPUT pixel,
//                       i.e. 4 x the layer's output, on top of it.  The output goes straight into the next layer's
//                       zero-bordered buffer.
//   instance norm+SiLU  per (frame, channel) over the map: fp64 sums of x and x^2 over chunks of 1024 pixels (a thread
//                       sums its pixels in order, the four threads of a channel are added in order), the chunks are
//                       added in order, mean and 1 / sqrt(var + 1e-5) stay fp64 and (x - mean) is taken in fp64, so a
//                       channel with a large mean keeps its spread.  x^2 of an fp32 value is exact in fp64.  In place.
//   finish_kernel       bilinear read of raw [B, h, w, 4] at H x W, n / (|n| + 1e-5) for three channels, planar store.
//
// The 1 x 1 convolutions are plain GEMMs over NHWC rows; the last one's 3 or 1 columns are padded to 4.
// No atomics; every sum has one fixed order; a frame's arithmetic depends on neither the batch nor the GEMM tile.
#include "flash_attention.hpp"
#include "instag_sapiens.h"

namespace instag {
namespace {

constexpr int MAX_T = INSTAG_SAPIENS_MAX_TOKENS;
constexpr int MAX_HEAD = INSTAG_SAPIENS_MAX_HEAD;
constexpr int MAX_WIDTH = INSTAG_SAPIENS_MAX_WIDTH;
constexpr int PATCH = 16, PATCH_PAD = 2, PATCH_K = 3 * PATCH * PATCH;      // 768
constexpr int MAX_SIDE = 16384;
constexpr float VIT_LN_EPS = 1e-6f;
constexpr double IN_EPS = 1e-5;
constexpr int IN_CHUNK = 1024;                                            // pixels of one partial sum
constexpr int RAW_C = 4;
constexpr int MAX_BATCH = 4096;
constexpr size_t MAX_MAP = (size_t)1 << 36;                                 // floats of one stage: its kernels' grids fit

struct Norm3 {
  float mean[3], std[3];
};

// ---- front end ----------------------------------------------------------------------------------------------------------
// source index and weight (of 2048) of destination pixel d on an axis resized from S to D pixels: the centre
// (d + 1/2) S / D - 1/2 as the exact fraction num / (2 D); below 0 and from S - 1 on the index is clamped, weight 0
__device__ __forceinline__ void resize_tap(int d, int S, int D, int* i0, int* i1, int* w1) {
  const int64_t num = (int64_t)(2 * d + 1) * S - D, den = 2 * (int64_t)D;
  if (num < 0) {
    *i0 = *i1 = 0;
    *w1 = 0;
    return;
  }
  const int s = (int)(num / den);
  if (s >= S - 1) {
    *i0 = *i1 = S - 1;
    *w1 = 0;
    return;
  }
  *i0 = s;
  *i1 = s + 1;
  *w1 = (int)(((num - s * den) * 2048 + D) / den);         // the fraction in 1/2048, rounded half up
}

__global__ void __launch_bounds__(TB) patch_rows_kernel(const uint8_t* __restrict__ frames, float* __restrict__ rows, int B,
                                                        int H, int W, int in_h, int in_w, int gh, int gw, Norm3 nm) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  const int T = gh * gw;
  if (i >= (size_t)B * T * PATCH_K) return;
  const int k = (int)(i % PATCH_K), tok = (int)((i / PATCH_K) % T), b = (int)(i / ((size_t)PATCH_K * T));
  const int c = k >> 8, ky = (k >> 4) & 15, kx = k & 15;
  const int y = (tok / gw) * PATCH + ky - PATCH_PAD, x = (tok % gw) * PATCH + kx - PATCH_PAD;
  float v = 0.f;
  if (y >= 0 && y < in_h && x >= 0 && x < in_w) {
    int y0, y1, wy, x0, x1, wx;
    resize_tap(y, H, in_h, &y0, &y1, &wy);
    resize_tap(x, W, in_w, &x0, &x1, &wx);
    const uint8_t* f = frames + (size_t)b * H * W * 3 + c;
    const int p00 = f[((size_t)y0 * W + x0) * 3], p01 = f[((size_t)y0 * W + x1) * 3];
    const int p10 = f[((size_t)y1 * W + x0) * 3], p11 = f[((size_t)y1 * W + x1) * 3];
    const int sum = (2048 - wy) * ((2048 - wx) * p00 + wx * p01) + wy * ((2048 - wx) * p10 + wx * p11);
    v = ((float)((sum + (1 << 21)) >> 22) - nm.mean[c]) / nm.std[c];
  }
  rows[i] = v;
}

// ---- maps with and without a zero border: src [B, h, w, C] with border sp -> dst with border dp ----------------------------
__global__ void __launch_bounds__(TB) copy_map_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int h,
                                                      int w, int C, int sp, int dp) {
  const int hd = h + 2 * dp, wd = w + 2 * dp, ws = w + 2 * sp;
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)B * hd * wd * C) return;
  const int c = (int)(i % C), x = (int)((i / C) % wd) - dp, y = (int)((i / ((size_t)C * wd)) % hd) - dp;
  const int b = (int)(i / ((size_t)C * wd * hd));
  dst[i] = (x >= 0 && x < w && y >= 0 && y < h)
               ? src[(((size_t)b * (h + 2 * sp) + y + sp) * ws + x + sp) * C + c] : 0.f;
}

// ---- InstanceNorm + SiLU over x [B, h, w, C] with a border of p pixels ------------------------------------------------------
__global__ void __launch_bounds__(TB) norm_partial_kernel(const float* __restrict__ x, double* __restrict__ partial, int h,
                                                          int w, int C, int p) {
  __shared__ double red[2][4][64];
  const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const int chunk = blockIdx.x, c = blockIdx.y * 64 + cl, b = blockIdx.z, N = h * w, wp = w + 2 * p;
  const float* base = x + (size_t)b * (h + 2 * p) * wp * C;
  double s = 0.0, ss = 0.0;
  if (c < C) {
    const int end = min(N, (chunk + 1) * IN_CHUNK);
    for (int q = chunk * IN_CHUNK + pl; q < end; q += 4) {
      const int yy = q / w, xx = q - yy * w;
      const double v = (double)base[((size_t)(yy + p) * wp + xx + p) * C + c];
      s += v;
      ss += v * v;
    }
  }
  red[0][pl][cl] = s;
  red[1][pl][cl] = ss;
  __syncthreads();
  if (pl == 0 && c < C) {
    double* out = partial + (((size_t)b * gridDim.x + chunk) * C + c) * 2;
    out[0] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
    out[1] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
  }
}

__global__ void __launch_bounds__(TB) norm_stats_kernel(const double* __restrict__ partial, double* __restrict__ stats, int B,
                                                        int chunks, int C, int N) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  double s = 0.0, ss = 0.0;
  for (int k = 0; k < chunks; ++k) {
    const double* in = partial + (((size_t)b * chunks + k) * C + c) * 2;
    s += in[0];
    ss += in[1];
  }
  const double mean = s / N, var = fmax(ss / N - mean * mean, 0.0);
  stats[2 * (size_t)i] = mean;
  stats[2 * (size_t)i + 1] = 1.0 / sqrt(var + IN_EPS);
}

__global__ void __launch_bounds__(TB) norm_apply_kernel(float* __restrict__ x, const double* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int B, int h, int w, int C, int p) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)B * h * w * C) return;
  const int c = (int)(i % C), xx = (int)((i / C) % w), yy = (int)((i / ((size_t)C * w)) % h);
  const int b = (int)(i / ((size_t)C * w * h));
  float* at = x + (((size_t)b * (h + 2 * p) + yy + p) * (w + 2 * p) + xx + p) * C + c;
  const double* st = stats + 2 * ((size_t)b * C + c);
  float y = (float)(((double)*at - st[0]) * st[1]);
  if (gamma) y = y * gamma[c] + beta[c];
  *at = y / (1.f + expf(-y));
}

// ---- finish: raw [B, h, w, 4] -> out [B, C, H, W] -----------------------------------------------------------------------------
__device__ __forceinline__ void bilinear_tap(int d, float scale, int S, int* i0, int* i1, float* l1) {
  const float src = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.f);
  *i0 = min((int)src, S - 1);
  *i1 = min(*i0 + 1, S - 1);
  *l1 = src - (float)*i0;
}

__global__ void __launch_bounds__(TB) finish_kernel(const float* __restrict__ raw, float* __restrict__ out, int B, int h, int w,
                                                    int C, int H, int W, float sy, float sx) {
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= (size_t)B * H * W) return;
  const int X = (int)(i % W), Y = (int)((i / W) % H), b = (int)(i / ((size_t)W * H));
  int y0, y1, x0, x1;
  float ly, lx;
  bilinear_tap(Y, sy, h, &y0, &y1, &ly);
  bilinear_tap(X, sx, w, &x0, &x1, &lx);
  const float4* m = reinterpret_cast<const float4*>(raw) + (size_t)b * h * w;
  const float4 a = m[(size_t)y0 * w + x0], bb = m[(size_t)y0 * w + x1], c = m[(size_t)y1 * w + x0], d = m[(size_t)y1 * w + x1];
  const float hy = 1.f - ly, hx = 1.f - lx;
  float v[3] = {hy * (hx * a.x + lx * bb.x) + ly * (hx * c.x + lx * d.x),
                hy * (hx * a.y + lx * bb.y) + ly * (hx * c.y + lx * d.y),
                hy * (hx * a.z + lx * bb.z) + ly * (hx * c.z + lx * d.z)};
  if (C == 3) {
    const float inv = 1.f / (sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-5f);
    v[0] *= inv;
    v[1] *= inv;
    v[2] *= inv;
  }
  for (int ch = 0; ch < C; ++ch) out[(((size_t)b * C + ch) * H + Y) * W + X] = v[ch];
}

// ---- host -----------------------------------------------------------------------------------------------------------------
inline int grid_of(int in) { return (in + 2 * PATCH_PAD - PATCH) / PATCH + 1; }

const char* shape_error(const instag_sapiens_weights* w) {
  if (!w) return "NULL weights";
  if (w->heads < 1 || w->hidden != w->heads * HEAD_DIM) return "hidden / heads must be 64";
  if (w->hidden > MAX_ROW) return "hidden must be at most 1024";
  if (w->intermediate < 32 || w->intermediate % 32 || w->intermediate > 65536) return "intermediate must be a multiple of 32";
  if (w->layers < 1 || w->layers > INSTAG_SAPIENS_MAX_LAYERS) return "layers must be in [1, INSTAG_SAPIENS_MAX_LAYERS]";
  if (w->in_h < PATCH - 2 * PATCH_PAD || w->in_w < PATCH - 2 * PATCH_PAD || w->in_h > MAX_SIDE || w->in_w > MAX_SIDE)
    return "in_h and in_w must be in [12, 16384]";
  if ((int64_t)grid_of(w->in_h) * grid_of(w->in_w) > MAX_T) return "more than INSTAG_SAPIENS_MAX_TOKENS tokens";
  if (w->n_deconv < 1 || w->n_deconv > MAX_HEAD || w->n_conv < 0 || w->n_conv > MAX_HEAD)
    return "n_deconv in [1, INSTAG_SAPIENS_MAX_HEAD], n_conv in [0, INSTAG_SAPIENS_MAX_HEAD]";
  for (int j = 0; j < w->n_deconv; ++j)
    if (w->deconv_c[j] < 32 || w->deconv_c[j] % 32 || w->deconv_c[j] > MAX_WIDTH)
      return "a deconv width must be a multiple of 32, at most INSTAG_SAPIENS_MAX_WIDTH";
  for (int j = 0; j < w->n_conv; ++j)
    if (w->conv_c[j] < 32 || w->conv_c[j] % 32 || w->conv_c[j] > MAX_WIDTH)
      return "a conv width must be a multiple of 32, at most INSTAG_SAPIENS_MAX_WIDTH";
  if (w->out_channels != 1 && w->out_channels != 3) return "out_channels must be 1 or 3";
  for (int c = 0; c < 3; ++c)
    if (!(w->std[c] > 0.f)) return "std must be positive";
  return nullptr;
}

struct Plan {
  int gh, gw, T, h, w;                        // the token grid and the head's output map
  int sh[2 * MAX_HEAD + 1], sw[2 * MAX_HEAD + 1], sc[2 * MAX_HEAD + 1], sp[2 * MAX_HEAD + 1];   // head stage s: map, width, border
  int chunks;                                 // of the largest map
  size_t feat, rows, hh, x, qkv, ctx, ff;     // offsets in floats
  size_t buf[2], raw, partial, stats, total;
};

// false: the batch is refused
bool make_plan(const instag_sapiens_weights* w, int B, Plan* p) {
  p->gh = grid_of(w->in_h);
  p->gw = grid_of(w->in_w);
  p->T = p->gh * p->gw;
  const int nd = w->n_deconv, nc = w->n_conv;
  p->h = p->gh << nd;
  p->w = p->gw << nd;
  if (B < 1 || B > MAX_BATCH || (int64_t)B * p->h * p->w > INT32_MAX) return false;
  // stage 0: the bordered features; 1 .. nd: the deconvs' outputs (bordered but the last); then the convs'
  size_t size[2] = {0, 0};
  int max_c = 0;
  for (int s = 0; s <= nd + nc; ++s) {
    p->sh[s] = s <= nd ? p->gh << s : p->h;
    p->sw[s] = s <= nd ? p->gw << s : p->w;
    p->sc[s] = s == 0 ? w->hidden : s <= nd ? w->deconv_c[s - 1] : w->conv_c[s - nd - 1];
    p->sp[s] = s < nd ? 1 : 0;
    const size_t n = (size_t)B * (p->sh[s] + 2 * p->sp[s]) * (p->sw[s] + 2 * p->sp[s]) * p->sc[s];
    if (n > MAX_MAP) return false;
    size[s & 1] = std::max(size[s & 1], n);
    if (s) max_c = std::max(max_c, p->sc[s]);
  }
  p->chunks = (int)div_up((int64_t)p->h * p->w, (int64_t)IN_CHUNK);
  const size_t H = w->hidden, rows = (size_t)B * p->T;
  Arena a;
  p->feat = a.take(rows * H);
  const size_t region = a.off;
  p->rows = a.take(rows * PATCH_K);
  p->hh = a.take(rows * H);
  p->x = a.take(rows * H);
  p->qkv = a.take(rows * 3 * H);
  p->ctx = a.take(rows * H);
  p->ff = a.take(rows * w->intermediate);
  const size_t backbone_end = a.off;
  a.off = region;                                        // the head works where the backbone did: only feat outlives it
  p->buf[0] = a.take(size[0]);
  p->buf[1] = a.take(size[1]);
  p->raw = a.take((size_t)B * p->h * p->w * RAW_C);
  p->partial = a.take((size_t)B * p->chunks * max_c * 2 * 2);      // doubles, counted in floats
  p->stats = a.take((size_t)B * max_c * 2 * 2);
  p->total = std::max(a.off, backbone_end);
  return true;
}

size_t taps_floats(const instag_sapiens_weights* w, int B, const Plan& p) {
  size_t n = (size_t)(2 + 2 * w->layers) * B * p.T * w->hidden;
  for (int s = 1; s <= w->n_deconv + w->n_conv; ++s) n += (size_t)B * p.sh[s] * p.sw[s] * p.sc[s];
  return n + (size_t)B * p.h * p.w * RAW_C;
}

bool entry_plan(const char* fn, const instag_sapiens_weights* w, int batch, Plan* p) {
  const std::string who = std::string("sapiens_") + fn;
  if (const char* e = shape_error(w)) {
    set_error(who + ": " + e);
    return false;
  }
  if (!make_plan(w, batch, p)) {
    set_error(who + ": batch in [1, 4096], batch x the output map below 2^31 pixels and a stage below 2^36 floats");
    return false;
  }
  return true;
}

int patch_rows(const uint8_t* frames, int B, int H, int W, int in_h, int in_w, const Norm3& nm, float* rows, hipStream_t st) {
  const int gh = grid_of(in_h), gw = grid_of(in_w);
  const size_t n = (size_t)B * gh * gw * PATCH_K;
  patch_rows_kernel<<<(unsigned)div_up(n, (size_t)TB), TB, 0, st>>>(frames, rows, B, H, W, in_h, in_w, gh, gw, nm);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int copy_map(const float* src, float* dst, int B, int h, int w, int C, int sp, int dp, hipStream_t st) {
  const size_t n = (size_t)B * (h + 2 * dp) * (w + 2 * dp) * C;
  copy_map_kernel<<<(unsigned)div_up(n, (size_t)TB), TB, 0, st>>>(src, dst, B, h, w, C, sp, dp);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

// P [B, h + 2, w + 2, cin] with a zero border -> out [B, 2 h + 2 op, 2 w + 2 op, cout], interior only (file comment)
int deconv(const float* P, const float* wt, const float* zeros, float* out, int op, int B, int h, int w, int cin, int cout,
           int tile, hipStream_t st) {
  const int wp = w + 2, owp = 2 * w + 2 * op;
  const size_t in_frame = (size_t)(h + 2) * wp * cin, out_frame = (size_t)(2 * h + 2 * op) * owp * cout;
  for (int b = 0; b < B; ++b)
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px)
        for (int v = 0; v < 2; ++v) {
          GemmArgs g{};
          g.a = P + b * in_frame + ((size_t)(py + v) * wp + px) * cin;
          g.w = wt + (size_t)((py * 2 + px) * 2 + v) * 2 * cin * cout;
          g.bias = zeros;
          g.d = out + b * out_frame + ((size_t)(py + op) * owp + px + op) * cout;
          g.res = v ? g.d : nullptr;
          g.M = h * w; g.rows = w; g.N = cout; g.K = 2 * cin; g.groups = 1;
          g.a_batch = (int64_t)wp * cin; g.lda = cin;
          g.d_batch = (int64_t)2 * owp * cout; g.ldd = 2 * cout;
          INSTAG_TRY(launch_gemm(g, st, tile));
        }
  return INSTAG_OK;
}

int instance_norm_silu(float* x, int p, int B, int h, int w, int C, const float* gamma, const float* beta, double* partial,
                       double* stats, hipStream_t st) {
  const int N = h * w, chunks = (int)div_up(N, IN_CHUNK);
  norm_partial_kernel<<<dim3((unsigned)chunks, (unsigned)div_up(C, 64), (unsigned)B), TB, 0, st>>>(x, partial, h, w, C, p);
  INSTAG_CHECK_LAUNCH();
  norm_stats_kernel<<<(unsigned)div_up(B * C, TB), TB, 0, st>>>(partial, stats, B, chunks, C, N);
  INSTAG_CHECK_LAUNCH();
  norm_apply_kernel<<<(unsigned)div_up((size_t)B * N * C, (size_t)TB), TB, 0, st>>>(x, stats, gamma, beta, B, h, w, C, p);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int finish(const float* raw, int B, int h, int w, int C, int H, int W, float* out, hipStream_t st) {
  finish_kernel<<<(unsigned)div_up((size_t)B * H * W, (size_t)TB), TB, 0, st>>>(raw, out, B, h, w, C, H, W,
                                                                               (float)h / (float)H, (float)w / (float)W);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int require_weights(const instag_sapiens_weights* w, int mode) {
  const std::string who = "sapiens_forward";
  if (mode != 2) {
    INSTAG_REQUIRE(w->patch_w && w->patch_b && w->pos_embed && w->enc_ln_g && w->enc_ln_b,
                   who + ": NULL weight outside the layers");
    for (int l = 0; l < w->layers; ++l)
      INSTAG_REQUIRE(w->ln1_g[l] && w->ln1_b[l] && w->qkv_w[l] && w->qkv_b[l] && w->out_w[l] && w->out_b[l] && w->ln2_g[l] &&
                         w->ln2_b[l] && w->ff1_w[l] && w->ff1_b[l] && w->ff2_w[l] && w->ff2_b[l],
                     who + ": NULL weight in layer " + std::to_string(l));
  }
  if (mode != 1) {
    INSTAG_REQUIRE(w->seg_w && w->seg_b && w->zeros, who + ": NULL weight in the head");
    for (int j = 0; j < w->n_deconv; ++j)
      INSTAG_REQUIRE(w->deconv_w[j] && !w->deconv_g[j] == !w->deconv_b[j],
                     who + ": deconv " + std::to_string(j) + " needs its weight, and its norm both gain and shift or neither");
    for (int j = 0; j < w->n_conv; ++j)
      INSTAG_REQUIRE(w->conv_w[j] && w->conv_bias[j] && !w->conv_g[j] == !w->conv_beta[j],
                     who + ": conv " + std::to_string(j) + " needs weight and bias, and its norm both gain and shift or neither");
  }
  return INSTAG_OK;
}

int run(const instag_sapiens_weights* w, const Plan& p, const uint8_t* frames, int B, int H, int W, int mode, float* out,
        float* raw, float* features, float* ws, int tile, float* taps, hipStream_t st) {
  const int Hd = w->hidden, T = p.T, M = B * T, nd = w->n_deconv, nc = w->n_conv;
  size_t tap_off = 0;
  auto tap = [&](const float* src, size_t count) -> int {
    if (taps) {
      INSTAG_CHECK_HIP(hipMemcpyAsync(taps + tap_off, src, count * sizeof(float), hipMemcpyDeviceToDevice, st));
      tap_off += count;
    }
    return INSTAG_OK;
  };
  float* feat = features ? features : ws + p.feat;

  if (mode != 2) {
    float *rows = ws + p.rows, *h = ws + p.hh;
    Norm3 nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = w->mean[c], nm.std[c] = w->std[c];
    INSTAG_TRY(patch_rows(frames, B, H, W, w->in_h, w->in_w, nm, rows, st));
    for (int b = 0; b < B; ++b)       // per frame: the residual is read at D's index, and pos_embed is one frame's
      INSTAG_TRY(linear(rows + (size_t)b * T * PATCH_K, w->patch_w, w->patch_b, w->pos_embed, h + (size_t)b * T * Hd, T,
                        PATCH_K, Hd, 0, tile, st));
    INSTAG_TRY(tap(h, (size_t)M * Hd));
    INSTAG_TRY(run_layers(w, B, T, LayerBuffers{h, ws + p.x, ws + p.qkv, ws + p.ctx, ws + p.ff}, VIT_LN_EPS, tile, tap, st,
                          flash_attention));
    INSTAG_TRY(layernorm(h, feat, w->enc_ln_g, w->enc_ln_b, M, Hd, 0, VIT_LN_EPS, st));
    INSTAG_TRY(tap(feat, (size_t)M * Hd));
    if (mode == 1) return INSTAG_OK;
  }

  float* buf[2] = {ws + p.buf[0], ws + p.buf[1]};
  double *partial = reinterpret_cast<double*>(ws + p.partial), *stats = reinterpret_cast<double*>(ws + p.stats);
  INSTAG_TRY(copy_map(feat, buf[0], B, p.gh, p.gw, Hd, 0, 1, st));
  for (int s = 1; s <= nd + nc; ++s) {
    float *in = buf[(s - 1) & 1], *o = buf[s & 1];
    const int hs = p.sh[s], wd = p.sw[s], C = p.sc[s], pad = p.sp[s];
    const float *gamma, *beta;
    if (s <= nd) {
      if (pad)
        INSTAG_CHECK_HIP(hipMemsetAsync(o, 0, (size_t)B * (hs + 2) * (wd + 2) * C * sizeof(float), st));
      INSTAG_TRY(deconv(in, w->deconv_w[s - 1], w->zeros, o, pad, B, p.sh[s - 1], p.sw[s - 1], p.sc[s - 1], C, tile, st));
      gamma = w->deconv_g[s - 1];
      beta = w->deconv_b[s - 1];
    } else {
      const int j = s - nd - 1;
      INSTAG_TRY(linear(in, w->conv_w[j], w->conv_bias[j], nullptr, o, B * hs * wd, p.sc[s - 1], C, 0, tile, st));
      gamma = w->conv_g[j];
      beta = w->conv_beta[j];
    }
    INSTAG_TRY(instance_norm_silu(o, pad, B, hs, wd, C, gamma, beta, partial, stats, st));
    if (taps) {
      if (pad) {
        INSTAG_TRY(copy_map(o, taps + tap_off, B, hs, wd, C, 1, 0, st));
        tap_off += (size_t)B * hs * wd * C;
      } else {
        INSTAG_TRY(tap(o, (size_t)B * hs * wd * C));
      }
    }
  }
  float* rawp = raw ? raw : ws + p.raw;
  INSTAG_TRY(linear(buf[(nd + nc) & 1], w->seg_w, w->seg_b, nullptr, rawp, B * p.h * p.w, p.sc[nd + nc], RAW_C, 0, tile, st));
  INSTAG_TRY(tap(rawp, (size_t)B * p.h * p.w * RAW_C));
  return finish(rawp, B, p.h, p.w, w->out_channels, H, W, out, st);
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

inline size_t deconv_ws_floats(int B, int h, int w, int cin, int cout) {
  Arena a;
  a.take((size_t)B * (h + 2) * (w + 2) * cin);
  a.take((size_t)cout);
  return a.off;
}

inline bool deconv_shape_ok(int B, int h, int w, int cin, int cout) {
  return B >= 1 && B <= MAX_BATCH && h >= 1 && w >= 1 && cin >= 32 && cin % 32 == 0 && cin <= MAX_WIDTH && cout >= 32 && cout % 32 == 0 &&
         cout <= MAX_WIDTH && (int64_t)B * 4 * h * w <= INT32_MAX && (size_t)B * (h + 2) * (w + 2) * cin <= MAX_MAP &&
         (size_t)B * 4 * h * w * cout <= MAX_MAP;
}

inline bool norm_shape_ok(int B, int h, int w, int C) {
  return B >= 1 && B <= MAX_BATCH && h >= 1 && w >= 1 && C >= 1 && C <= MAX_WIDTH && (int64_t)B * h * w <= INT32_MAX &&
         (size_t)B * h * w * C <= MAX_MAP;
}

inline size_t norm_ws_floats(int B, int h, int w, int C) {
  Arena a;
  a.take((size_t)B * div_up((int64_t)h * w, (int64_t)IN_CHUNK) * C * 4);
  a.take((size_t)B * C * 4);
  return a.off;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_sapiens_workspace_bytes(const instag_sapiens_weights* w, int32_t batch) {
  Plan p;
  return entry_plan("workspace_bytes", w, batch, &p) ? p.total * sizeof(float) : 0;
}

size_t instag_sapiens_taps_floats(const instag_sapiens_weights* w, int32_t batch) {
  Plan p;
  return entry_plan("taps_floats", w, batch, &p) ? taps_floats(w, batch, p) : 0;
}

int instag_sapiens_forward(const instag_sapiens_weights* w, const uint8_t* frames, int32_t batch, int32_t H, int32_t W,
                           int32_t mode, float* out, float* raw, float* features, void* workspace,
                           size_t workspace_bytes, int32_t tile, float* taps, instag_stream_t stream) {
  Plan p;
  if (!entry_plan("forward", w, batch, &p)) return INSTAG_E_ARG;
  INSTAG_REQUIRE(mode >= 0 && mode <= 2, "sapiens_forward: mode must be 0, 1 or 2");
  INSTAG_REQUIRE(workspace && (mode == 2 || frames) && (mode == 1 || out) && (mode == 0 || features),
                 "sapiens_forward: NULL tensor");
  INSTAG_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE && (int64_t)batch * H * W <= INT32_MAX,
                 "sapiens_forward: H and W in [1, 16384], batch x H x W below 2^31");
  INSTAG_REQUIRE(tile >= 0 && tile <= 3, "sapiens_forward: tile must be 0..3");
  INSTAG_REQUIRE(!taps || mode == 0, "sapiens_forward: taps go with mode 0");
  INSTAG_REQUIRE(aligned16(workspace) && aligned16(raw) && aligned16(features),
                 "sapiens_forward: workspace, raw and features are 16-byte aligned");
  INSTAG_TRY(require_weights(w, mode));
  if (workspace_bytes < p.total * sizeof(float)) {
    set_error("sapiens_forward: workspace smaller than instag_sapiens_workspace_bytes(w, batch)");
    return INSTAG_E_SPACE;
  }
  return run(w, p, frames, batch, H, W, mode, out, raw, features, (float*)workspace, tile, taps, (hipStream_t)stream);
}

int instag_sapiens_patch_rows(const uint8_t* frames, int32_t batch, int32_t H, int32_t W, int32_t in_h, int32_t in_w,
                              const float* mean, const float* std, float* rows, instag_stream_t stream) {
  INSTAG_REQUIRE(frames && mean && std && rows, "sapiens_patch_rows: NULL tensor");
  INSTAG_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "sapiens_patch_rows: H and W in [1, 16384]");
  INSTAG_REQUIRE(in_h >= 12 && in_w >= 12 && in_h <= MAX_SIDE && in_w <= MAX_SIDE, "sapiens_patch_rows: in_h and in_w in [12, 16384]");
  INSTAG_REQUIRE(batch >= 1 && (int64_t)batch * H * W <= INT32_MAX && (int64_t)batch * grid_of(in_h) * grid_of(in_w) <= INT32_MAX / PATCH_K,
                 "sapiens_patch_rows: batch >= 1, batch x H x W and the rows' floats below 2^31");
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    INSTAG_REQUIRE(std[c] > 0.f, "sapiens_patch_rows: std must be positive");
    nm.mean[c] = mean[c];
    nm.std[c] = std[c];
  }
  return patch_rows(frames, batch, H, W, in_h, in_w, nm, rows, (hipStream_t)stream);
}

int instag_sapiens_attention(const float* qkv, float* ctx, int32_t batch, int32_t frames, int32_t heads,
                             instag_stream_t stream) {
  INSTAG_REQUIRE(qkv && ctx, "sapiens_attention: NULL tensor");
  INSTAG_REQUIRE(((uintptr_t)qkv | (uintptr_t)ctx) % 16 == 0, "sapiens_attention: qkv and ctx are 16-byte aligned");
  INSTAG_REQUIRE(batch >= 1 && batch <= 4096 && heads >= 1 && heads <= 65535,
                 "sapiens_attention: batch in [1, 4096], heads in [1, 65535]");
  INSTAG_REQUIRE(frames >= 1 && frames <= MAX_T, "sapiens_attention: frames in [1, INSTAG_SAPIENS_MAX_TOKENS]");
  return flash_attention(qkv, ctx, batch, frames, heads * HEAD_DIM, (hipStream_t)stream);
}

size_t instag_sapiens_deconv_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout) {
  if (!deconv_shape_ok(batch, h, w, cin, cout)) {
    set_error("sapiens_deconv_workspace_bytes: batch in [1, 4096], h, w >= 1, cin and cout multiples of 32 up to INSTAG_SAPIENS_MAX_WIDTH");
    return 0;
  }
  return deconv_ws_floats(batch, h, w, cin, cout) * sizeof(float);
}

int instag_sapiens_deconv(const float* x, const float* weight, float* y, int32_t batch, int32_t h, int32_t w,
                          int32_t cin, int32_t cout, void* workspace, size_t workspace_bytes, int32_t tile,
                          instag_stream_t stream) {
  INSTAG_REQUIRE(x && weight && y && workspace, "sapiens_deconv: NULL tensor");
  INSTAG_REQUIRE(deconv_shape_ok(batch, h, w, cin, cout),
                 "sapiens_deconv: batch in [1, 4096], h, w >= 1, cin and cout multiples of 32 up to INSTAG_SAPIENS_MAX_WIDTH");
  INSTAG_REQUIRE(tile >= 0 && tile <= 3, "sapiens_deconv: tile must be 0..3");
  INSTAG_REQUIRE(aligned16(x) && aligned16(weight) && aligned16(y) && aligned16(workspace),
                 "sapiens_deconv: the tensors are 16-byte aligned");
  if (workspace_bytes < deconv_ws_floats(batch, h, w, cin, cout) * sizeof(float)) {
    set_error("sapiens_deconv: workspace smaller than instag_sapiens_deconv_workspace_bytes");
    return INSTAG_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* P = (float*)workspace;
  float* zeros = P + align_up((size_t)batch * (h + 2) * (w + 2) * cin, 64);
  INSTAG_CHECK_HIP(hipMemsetAsync(zeros, 0, (size_t)cout * sizeof(float), st));
  INSTAG_TRY(copy_map(x, P, batch, h, w, cin, 0, 1, st));
  return deconv(P, weight, zeros, y, 0, batch, h, w, cin, cout, tile, st);
}

size_t instag_sapiens_norm_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t channels) {
  if (!norm_shape_ok(batch, h, w, channels)) {
    set_error("sapiens_norm_workspace_bytes: batch in [1, 4096], h, w >= 1, channels in [1, INSTAG_SAPIENS_MAX_WIDTH]");
    return 0;
  }
  return norm_ws_floats(batch, h, w, channels) * sizeof(float);
}

int instag_sapiens_instance_norm_silu(float* x, int32_t batch, int32_t h, int32_t w, int32_t channels,
                                      const float* gamma, const float* beta, void* workspace, size_t workspace_bytes,
                                      instag_stream_t stream) {
  INSTAG_REQUIRE(x && workspace, "sapiens_instance_norm_silu: NULL tensor");
  INSTAG_REQUIRE(!gamma == !beta, "sapiens_instance_norm_silu: gamma and beta both or neither");
  INSTAG_REQUIRE(norm_shape_ok(batch, h, w, channels),
                 "sapiens_instance_norm_silu: batch in [1, 4096], h, w >= 1, channels in [1, INSTAG_SAPIENS_MAX_WIDTH]");
  INSTAG_REQUIRE((uintptr_t)workspace % 16 == 0, "sapiens_instance_norm_silu: the workspace is 16-byte aligned");
  if (workspace_bytes < norm_ws_floats(batch, h, w, channels) * sizeof(float)) {
    set_error("sapiens_instance_norm_silu: workspace smaller than instag_sapiens_norm_workspace_bytes");
    return INSTAG_E_SPACE;
  }
  double* partial = (double*)workspace;
  double* stats = (double*)((float*)workspace +
                            align_up((size_t)batch * div_up((int64_t)h * w, (int64_t)IN_CHUNK) * channels * 4, 64));
  return instance_norm_silu(x, 0, batch, h, w, channels, gamma, beta, partial, stats, (hipStream_t)stream);
}

int instag_sapiens_finish(const float* raw, int32_t batch, int32_t h, int32_t w, int32_t channels, int32_t H, int32_t W,
                          float* out, instag_stream_t stream) {
  INSTAG_REQUIRE(raw && out, "sapiens_finish: NULL tensor");
  INSTAG_REQUIRE(channels == 1 || channels == 3, "sapiens_finish: channels must be 1 or 3");
  INSTAG_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE &&
                     (int64_t)batch * h * w <= INT32_MAX && (int64_t)batch * H * W <= INT32_MAX,
                 "sapiens_finish: batch, h, w >= 1, H and W in [1, 16384], the maps below 2^31 pixels");
  INSTAG_REQUIRE(aligned16(raw), "sapiens_finish: raw is 16-byte aligned");
  return finish(raw, batch, h, w, channels, H, W, out, (hipStream_t)stream);
}

}  // extern "C"
