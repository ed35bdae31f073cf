// Face detection (the face_alignment package's detection/sfd: net_s3fd.py, detect.py, bbox.py, sfd_detector.py): S3FD in
// eval mode, fp32, forward only, from uint8 frames to the face boxes the landmark network crops by
// (include/instag_face_detect.h; instag_amd/face_detect.py states the network, the tail and this project's rules).
//
//   convolutions  conv_mfma.hpp through ConvNet, the kernel parsing.hip, teeth.hip and landmarks.hip run: 19 trunk
//                 convolutions with (1, bias) and the ReLU in the epilogue and one head convolution per level (conf and
//                 loc packed along cout), 25 launches.
//   the stem      conv1_1 is the 3 x 3 uint8 stem at stride 1: the gather reads the RGB frame through a table of
//                 u - mean (stdev 1, the mean in RGB order); the BGR flip is a permutation of the weight's rows on the
//                 host.  The padding is zero after the subtraction.
//   fc6           3 x 3 with padding 3: the pool behind conv5_3 writes into the interior of a map with a zero border of
//                 2, and the pad-1 convolution over that map is the pad-3 result.
//   conv6_2, conv7_2   3 x 3, stride 2, odd input sides: the plain source's tap mask serves them as it stands.
//   pool          2 x 2 / stride 2 maximum, one thread per output element, the optional border written as zeros.
//   L2Norm        32 positions per workgroup, their channels split over 8 groups of threads; partial sums of squares
//                 through LDS, added in a fixed order, then x / (sqrt(sum) + 1e-10) * weight[c].
//   the tail      one workgroup of 1024 threads per frame, one launch per chunk: the scores straight from the logits;
//                 the candidates compacted into LDS in candidate order by ballots and a prefix over the 16 waves; a
//                 bitonic sort of 64-bit keys (score bits high, inverted index low: descending score, then ascending
//                 index); the boxes decoded into registers, four sorted positions per thread; the greedy NMS in rounds
//                 -- every wave finds the first position still alive in a 4096-bit mask in LDS, its owner broadcasts
//                 the box through LDS, every thread tests its later positions against it in fp64 and each wave writes
//                 its own mask words from a ballot.  A round ends the loop when the kept score is not above 0.5: the
//                 scores descend, so no later round could add a detection.
// No atomics anywhere, every sum in a fixed order, a frame reads nothing but its own data: its bits depend neither on
// the batch, the chunk nor the tile.  The file is compiled with -ffp-contract=off: the decode and the overlap are the
// statement's operations one by one (the convolution's FMAs are written out and stay).
#include "common.hpp"
#include "conv_net.hpp"
#include "instag_face_detect.h"

namespace instag {
namespace {

constexpr int NLAYER = INSTAG_FACE_DETECT_LAYERS, NLEVEL = INSTAG_FACE_DETECT_LEVELS;
constexpr int MAX_CAND = INSTAG_FACE_DETECT_MAX_CANDIDATES, MAX_FACES = INSTAG_FACE_DETECT_MAX_FACES;
constexpr int TAIL_TB = 1024, TAIL_WAVES = TAIL_TB / 64, SLOTS = MAX_CAND / TAIL_TB;
constexpr float MEAN_RGB[3] = {123.f, 117.f, 104.f};
// order of instag_face_detect_weights (instag_amd/face_detect.py: TRUNK, then the heads)
enum Layer { L_CONV1 = 0, L_CONV2 = 2, L_CONV3 = 4, L_CONV4 = 7, L_CONV5 = 10, L_FC6 = 13, L_FC7 = 14, L_CONV6 = 15,
             L_CONV7 = 17, L_HEAD = 19 };

inline int head_channels(int level) { return level == 0 ? 8 : 6; }

// the sides of the six levels along one axis of length n (a multiple of 32)
inline void level_sides(int n, int* s) {
  s[0] = n / 4; s[1] = n / 8; s[2] = n / 16; s[3] = n / 32 + 4; s[4] = (s[3] - 1) / 2 + 1; s[5] = (s[4] - 1) / 2 + 1;
}

inline bool detect_frames_ok(int B, int H, int W) {
  return frames_ok(B, H, W) && B <= INSTAG_FACE_DETECT_MAX_BATCH && (size_t)B * 64 * H * W < ((size_t)1 << 31);
}
constexpr const char* DETECT_FRAMES_OK = ": 1 <= B <= 64, H and W multiples of 32 in [64, 4096], B * 64 * H * W < 2^31";

// ---- 2 x 2 max-pool, stride 2, into a map with a zero border ------------------------------------------------------------
// in [planes, hi, wi] -> out [planes, hi / 2 + 2 border, wi / 2 + 2 border]
__global__ void __launch_bounds__(TB) pool2_kernel(const float* in, float* out, size_t planes, int hi, int wi, int border) {
  const int ho = hi / 2 + 2 * border, wo = wi / 2 + 2 * border;
  const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
  if (i >= planes * ho * wo) return;
  const int x = (int)(i % wo) - border, y = (int)((i / wo) % ho) - border;
  const size_t p = i / ((size_t)wo * ho);
  float m = 0.f;
  if (x >= 0 && x < wi / 2 && y >= 0 && y < hi / 2) {
    const float* src = in + p * hi * wi + (size_t)(2 * y) * wi + 2 * x;
    m = fmaxf(fmaxf(src[0], src[1]), fmaxf(src[wi], src[wi + 1]));
  }
  out[i] = m;
}

int launch_pool(const float* in, float* out, size_t planes, int hi, int wi, int border, hipStream_t st) {
  const size_t n = planes * (hi / 2 + 2 * border) * (wi / 2 + 2 * border);
  pool2_kernel<<<(unsigned)div_up(n, (size_t)TB), TB, 0, st>>>(in, out, planes, hi, wi, border);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

// ---- L2Norm over the channels of a position ---------------------------------------------------------------------------
// in [B, C, hw] -> out = in / (sqrt(sum_c in^2) + 1e-10) * weight[c].  A workgroup takes 32 positions and splits their
// channels over 8 groups of threads, group g the channels g, g + 8, ..: the maps at stride 16 have few positions, and a
// thread per position alone left most of the chip idle there.  A group adds its squares into four running sums (four loads
// in flight), (s0 + s1) + (s2 + s3) goes through LDS, and the eight partial sums are added in group order: a fixed order.
constexpr int L2_PX = 32, L2_CG = TB / L2_PX;

__global__ void __launch_bounds__(TB) l2norm_kernel(const float* in, const float* weight, float* out, int B, int C, int hw) {
  __shared__ float part[L2_CG][L2_PX];
  const int px = threadIdx.x % L2_PX, cg = threadIdx.x / L2_PX;
  const size_t i = (size_t)blockIdx.x * L2_PX + px;
  const bool ok = i < (size_t)B * hw;
  const size_t base = ok ? (i / hw) * C * hw + i % hw : 0;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (ok) {
    int c = cg;
    for (; c + 3 * L2_CG < C; c += 4 * L2_CG)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = in[base + (size_t)(c + j * L2_CG) * hw];
        s[j] += v * v;
      }
    for (int j = 0; c < C; c += L2_CG, ++j) {
      const float v = in[base + (size_t)c * hw];
      s[j] += v * v;
    }
  }
  part[cg][px] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (!ok) return;
  float sum = 0.f;
#pragma unroll
  for (int g = 0; g < L2_CG; ++g) sum += part[g][px];
  const float d = sqrtf(sum) + 1e-10f;
#pragma unroll 4
  for (int c = cg; c < C; c += L2_CG) out[base + (size_t)c * hw] = in[base + (size_t)c * hw] / d * weight[c];
}

int launch_l2norm(const float* in, const float* weight, float* out, int B, int C, int hw, hipStream_t st) {
  l2norm_kernel<<<(unsigned)div_up((size_t)B * hw, (size_t)L2_PX), TB, 0, st>>>(in, weight, out, B, C, hw);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

// ---- the tail ---------------------------------------------------------------------------------------------------------
struct TailArgs {
  const float* map[NLEVEL];    // [B, C, h, w], C = 8 at level 0 and 6 elsewhere
  int h[NLEVEL], w[NLEVEL];
  int start[NLEVEL + 1];       // the first candidate index of a level; start[6]: the positions of a frame
  float* boxes;                // [B, 16, 5]
  int32_t* count;              // [B]
  uint8_t* overflow;           // [B]
};

// candidate index -> its level, position and the address of its first channel
struct Position {
  const float* p;
  size_t plane;
  int level, y, x;
};

__device__ inline Position position_of(const TailArgs& a, int frame, int idx) {
  Position q;
  q.level = 0;
#pragma unroll
  for (int l = 1; l < NLEVEL; ++l)
    if (idx >= a.start[l]) q.level = l;
  const int l = q.level, pos = idx - a.start[l];
  q.y = pos / a.w[l];
  q.x = pos - q.y * a.w[l];
  q.plane = (size_t)a.h[l] * a.w[l];
  q.p = a.map[l] + (size_t)frame * (l == 0 ? 8 : 6) * q.plane + pos;
  return q;
}

__device__ inline float score_of(const Position& q) {
  float bg, face;
  if (q.level == 0) {
    bg = fmaxf(fmaxf(q.p[0], q.p[q.plane]), q.p[2 * q.plane]);
    face = q.p[3 * q.plane];
  } else {
    bg = q.p[0];
    face = q.p[q.plane];
  }
  return (float)(1.0 / (1.0 + exp((double)bg - (double)face)));
}

__global__ void __launch_bounds__(TAIL_TB) tail_kernel(TailArgs a) {
  __shared__ uint64_t keys[MAX_CAND];
  __shared__ uint64_t alive[MAX_CAND / 64];
  __shared__ int wave_sum[TAIL_WAVES];
  __shared__ double kbox[5];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, frame = blockIdx.x;
  const int total = a.start[NLEVEL];

  // the candidates in index order: a ballot inside the wave, a prefix over the waves
  int n = 0;                                                                   // candidates so far, capped nowhere
  for (int base = 0; base < total; base += TAIL_TB) {
    const int idx = base + t;
    float s = 0.f;
    bool c = false;
    if (idx < total) {
      s = score_of(position_of(a, frame, idx));
      c = s > 0.05f;
    }
    const uint64_t b = __ballot(c);
    if (lane == 0) wave_sum[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & (((uint64_t)1 << lane) - 1)), all = 0;
#pragma unroll
    for (int v = 0; v < TAIL_WAVES; ++v) {
      const int ws = wave_sum[v];
      if (v < wave) before += ws;
      all += ws;
    }
    const int slot = n + before;
    if (c && slot < MAX_CAND) keys[slot] = ((uint64_t)__float_as_uint(s) << 32) | (uint32_t)~(uint32_t)idx;
    n += all;
    __syncthreads();
  }
  const int m = min(n, MAX_CAND);
  int n2 = 1;
  while (n2 < m) n2 <<= 1;
  for (int i = m + t; i < n2; i += TAIL_TB) keys[i] = 0;                       // below every candidate: score bits > 0
  __syncthreads();

  // bitonic sort, descending
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < n2; i += TAIL_TB) {
        const int p = i ^ j;
        if (p > i) {
          const uint64_t u = keys[i], v = keys[p];
          if ((i & k) == 0 ? u < v : u > v) {
            keys[i] = v;
            keys[p] = u;
          }
        }
      }
      __syncthreads();
    }

  // sorted position k TAIL_TB + t is this thread's: its box in fp64, as the statement decodes it
  double x1[SLOTS], y1[SLOTS], x2[SLOTS], y2[SLOTS], area[SLOTS];
  bool live[SLOTS];
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) {
    const int p = k * TAIL_TB + t;
    live[k] = p < m;
    x1[k] = y1[k] = x2[k] = y2[k] = area[k] = 0.0;
    if (live[k]) {
      const Position q = position_of(a, frame, (int)~(uint32_t)keys[p]);
      const float* loc = q.p + (q.level == 0 ? 4 : 2) * q.plane;
      const double s = (double)(4 << q.level);
      const double px = s / 2.0 + (double)q.x * s, py = s / 2.0 + (double)q.y * s, pw = 4.0 * s;
      const double cx = px + (double)loc[0] * 0.1 * pw, cy = py + (double)loc[q.plane] * 0.1 * pw;
      const double bw = pw * exp(0.2 * (double)loc[2 * q.plane]), bh = pw * exp(0.2 * (double)loc[3 * q.plane]);
      x1[k] = cx - bw / 2.0;
      y1[k] = cy - bh / 2.0;
      x2[k] = cx + bw / 2.0;
      y2[k] = cy + bh / 2.0;
      area[k] = (x2[k] - x1[k] + 1.0) * (y2[k] - y1[k] + 1.0);
    }
    const uint64_t word = __ballot(live[k]);                                  // positions k TAIL_TB + 64 wave ..
    if (lane == 0) alive[k * TAIL_WAVES + wave] = word;
  }
  __syncthreads();

  // greedy NMS: the first position still alive is kept, the later ones are tested against it
  int cur = 0, kept = 0;
  while (true) {
    const int w0 = cur >> 6;
    uint64_t wd = alive[lane];
    if (lane < w0) wd = 0;
    if (lane == w0) wd &= ~(uint64_t)0 << (cur & 63);
    const uint64_t has = __ballot(wd != 0);
    if (!has) break;
    const int wi = __ffsll((long long)has) - 1;
    uint64_t word = alive[wi];
    if (wi == w0) word &= ~(uint64_t)0 << (cur & 63);
    const int next = wi * 64 + __ffsll((long long)word) - 1;
    const float sc = __uint_as_float((uint32_t)(keys[next] >> 32));
    if (!(sc > 0.5f)) break;
    if (t == (next & (TAIL_TB - 1))) {
#pragma unroll
      for (int k = 0; k < SLOTS; ++k)
        if (k == next / TAIL_TB) {
          kbox[0] = x1[k]; kbox[1] = y1[k]; kbox[2] = x2[k]; kbox[3] = y2[k]; kbox[4] = area[k];
          if (kept < MAX_FACES) {
            float* row = a.boxes + ((size_t)frame * MAX_FACES + kept) * 5;
            row[0] = (float)x1[k]; row[1] = (float)y1[k]; row[2] = (float)x2[k]; row[3] = (float)y2[k]; row[4] = sc;
          }
        }
    }
    __syncthreads();
    const double kx1 = kbox[0], ky1 = kbox[1], kx2 = kbox[2], ky2 = kbox[3], karea = kbox[4];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      if (live[k] && k * TAIL_TB + t > next) {
        const double xx1 = fmax(kx1, x1[k]), yy1 = fmax(ky1, y1[k]), xx2 = fmin(kx2, x2[k]), yy2 = fmin(ky2, y2[k]);
        const double iw = fmax(0.0, xx2 - xx1 + 1.0), ih = fmax(0.0, yy2 - yy1 + 1.0);
        const double inter = iw * ih;
        const double ovr = inter / (karea + area[k] - inter);
        if (!(ovr <= 0.3)) live[k] = false;
      }
      const uint64_t word2 = __ballot(live[k]);
      if (lane == 0) alive[k * TAIL_WAVES + wave] = word2;
    }
    __syncthreads();
    ++kept;
    cur = next + 1;
  }

  if (t == 0) {
    a.count[frame] = kept;
    a.overflow[frame] = n > MAX_CAND ? 1 : 0;
  }
  for (int i = t; i < MAX_FACES * 5; i += TAIL_TB)
    if (i / 5 >= kept) a.boxes[(size_t)frame * MAX_FACES * 5 + i] = __int_as_float(0x7fc00000);
}

int launch_tail(const float* const* maps, int B, int H, int W, float* boxes, int32_t* count, uint8_t* overflow,
                hipStream_t st) {
  TailArgs a;
  int hs[NLEVEL], ws[NLEVEL];
  level_sides(H, hs);
  level_sides(W, ws);
  a.start[0] = 0;
  for (int l = 0; l < NLEVEL; ++l) {
    a.map[l] = maps[l];
    a.h[l] = hs[l];
    a.w[l] = ws[l];
    a.start[l + 1] = a.start[l] + hs[l] * ws[l];
  }
  a.boxes = boxes;
  a.count = count;
  a.overflow = overflow;
  tail_kernel<<<B, TAIL_TB, 0, st>>>(a);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------
// Floats per frame: 144 H W and the maps (144 MiB at 512 x 512).
struct Layout {
  size_t a, b;                 // the trunk's two maps in flight: 64 channels at full resolution each
  size_t norm;                 // an L2Norm's output, then conv6_2's: at most 256 channels at stride 4
  size_t map[NLEVEL];          // the packed head outputs, where the caller gives none
  size_t total;                // floats
};

Layout layout(int B, int H, int W) {
  Layout l;
  const size_t hw = (size_t)B * H * W;
  int hs[NLEVEL], ws[NLEVEL];
  level_sides(H, hs);
  level_sides(W, ws);
  Arena a;
  l.a = a.take(64 * hw);
  l.b = a.take(64 * hw);
  l.norm = a.take(16 * hw);
  for (int i = 0; i < NLEVEL; ++i) l.map[i] = a.take((size_t)B * head_channels(i) * hs[i] * ws[i]);
  l.total = a.off;
  return l;
}

// frames -> the six packed maps
int forward(const instag_face_detect_weights* w, const uint8_t* frames, int B, int H, int W, float* const* maps,
            float* base, const Layout& L, hipStream_t st) {
  const ConvNet conv{w->w, w->scale, w->shift, B, st};
  float *A = base + L.a, *Bf = base + L.b, *N = base + L.norm;
  int hs[NLEVEL], ws[NLEVEL];
  level_sides(H, hs);
  level_sides(W, ws);
  auto head = [&](int level, const float* in, int cin) -> int {
    return conv(L_HEAD + level, 3, in, cin, hs[level], ws[level], 1, head_channels(level), maps[level], nullptr, 0);
  };

  {
    ConvArgs e{};
    e.frames = frames;
    for (int c = 0; c < 3; ++c) { e.mean[c] = MEAN_RGB[c]; e.stdev[c] = 1.f; }
    INSTAG_TRY(conv(L_CONV1, 3, nullptr, 3, H, W, 1, 64, A, nullptr, 1, e));
  }
  INSTAG_TRY(conv(L_CONV1 + 1, 3, A, 64, H, W, 1, 64, Bf, nullptr, 1));
  INSTAG_TRY(launch_pool(Bf, A, (size_t)B * 64, H, W, 0, st));
  INSTAG_TRY(conv(L_CONV2, 3, A, 64, H / 2, W / 2, 1, 128, Bf, nullptr, 1));
  INSTAG_TRY(conv(L_CONV2 + 1, 3, Bf, 128, H / 2, W / 2, 1, 128, A, nullptr, 1));
  INSTAG_TRY(launch_pool(A, Bf, (size_t)B * 128, H / 2, W / 2, 0, st));
  // conv3, conv4, conv5: three convolutions (the map ends in A), the L2Norm and its head, the pool (into Bf)
  int cin = 128, layer = L_CONV3;
  for (int s = 0; s < 3; ++s) {
    const int ch = s == 0 ? 256 : 512, h = hs[s], wd = ws[s];
    INSTAG_TRY(conv(layer, 3, Bf, cin, h, wd, 1, ch, A, nullptr, 1));
    INSTAG_TRY(conv(layer + 1, 3, A, ch, h, wd, 1, ch, Bf, nullptr, 1));
    INSTAG_TRY(conv(layer + 2, 3, Bf, ch, h, wd, 1, ch, A, nullptr, 1));
    INSTAG_TRY(launch_l2norm(A, w->norm[s], N, B, ch, h * wd, st));
    INSTAG_TRY(head(s, N, ch));
    INSTAG_TRY(launch_pool(A, Bf, (size_t)B * ch, h, wd, s == 2 ? 2 : 0, st));      // behind conv5_3: fc6's border
    cin = ch;
    layer += 3;
  }
  INSTAG_TRY(conv(L_FC6, 3, Bf, 512, hs[3], ws[3], 1, 1024, A, nullptr, 1));
  INSTAG_TRY(conv(L_FC7, 1, A, 1024, hs[3], ws[3], 1, 1024, Bf, nullptr, 1));
  INSTAG_TRY(head(3, Bf, 1024));
  INSTAG_TRY(conv(L_CONV6, 1, Bf, 1024, hs[3], ws[3], 1, 256, A, nullptr, 1));
  INSTAG_TRY(conv(L_CONV6 + 1, 3, A, 256, hs[3], ws[3], 2, 512, N, nullptr, 1));
  INSTAG_TRY(head(4, N, 512));
  INSTAG_TRY(conv(L_CONV7, 1, N, 512, hs[4], ws[4], 1, 128, A, nullptr, 1));
  INSTAG_TRY(conv(L_CONV7 + 1, 3, A, 128, hs[4], ws[4], 2, 256, Bf, nullptr, 1));
  return head(5, Bf, 256);
}

int check_weights(const instag_face_detect_weights* w, const char* who) {
  const ConvNet conv{w->w, w->scale, w->shift, 1, nullptr};
  const int null_layer = conv.null_layer(NLAYER);
  INSTAG_REQUIRE(null_layer < 0, std::string(who) + ": NULL weight of layer " + std::to_string(null_layer));
  INSTAG_REQUIRE(w->norm[0] && w->norm[1] && w->norm[2], std::string(who) + ": NULL L2Norm weight");
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_face_detect_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (!detect_frames_ok(B, H, W)) {
    set_error(std::string("face_detect_workspace_bytes") + DETECT_FRAMES_OK);
    return 0;
  }
  return layout(B, H, W).total * sizeof(float);
}

int instag_face_detect_forward(const instag_face_detect_weights* w, const uint8_t* frames, int32_t B, int32_t H,
                               int32_t W, float* const* maps, void* workspace, size_t workspace_bytes,
                               instag_stream_t stream) {
  INSTAG_REQUIRE(w && frames && maps && workspace, "face_detect_forward: NULL tensor");
  for (int l = 0; l < NLEVEL; ++l) INSTAG_REQUIRE(maps[l], "face_detect_forward: NULL map of level " + std::to_string(l));
  INSTAG_TRY(check_weights(w, "face_detect_forward"));
  INSTAG_REQUIRE(detect_frames_ok(B, H, W), std::string("face_detect_forward") + DETECT_FRAMES_OK);
  const Layout L = layout(B, H, W);
  if (workspace_bytes < L.total * sizeof(float)) {
    set_error("face_detect_forward: workspace too small");
    return INSTAG_E_SPACE;
  }
  return forward(w, frames, B, H, W, maps, (float*)workspace, L, (hipStream_t)stream);
}

int instag_face_detect_post(const float* const* maps, int32_t B, int32_t H, int32_t W, float* boxes, int32_t* count,
                            uint8_t* overflow, instag_stream_t stream) {
  INSTAG_REQUIRE(maps && boxes && count && overflow, "face_detect_post: NULL tensor");
  for (int l = 0; l < NLEVEL; ++l) INSTAG_REQUIRE(maps[l], "face_detect_post: NULL map of level " + std::to_string(l));
  INSTAG_REQUIRE(detect_frames_ok(B, H, W), std::string("face_detect_post") + DETECT_FRAMES_OK);
  return launch_tail(maps, B, H, W, boxes, count, overflow, (hipStream_t)stream);
}

int instag_face_detect(const instag_face_detect_weights* w, const uint8_t* frames, int32_t B, int32_t H, int32_t W,
                       float* boxes, int32_t* count, uint8_t* overflow, void* workspace, size_t workspace_bytes,
                       instag_stream_t stream) {
  INSTAG_REQUIRE(w && frames && boxes && count && overflow && workspace, "face_detect: NULL tensor");
  INSTAG_TRY(check_weights(w, "face_detect"));
  INSTAG_REQUIRE(detect_frames_ok(B, H, W), std::string("face_detect") + DETECT_FRAMES_OK);
  const Layout L = layout(B, H, W);
  if (workspace_bytes < L.total * sizeof(float)) {
    set_error("face_detect: workspace too small");
    return INSTAG_E_SPACE;
  }
  float* base = (float*)workspace;
  float* maps[NLEVEL];
  for (int l = 0; l < NLEVEL; ++l) maps[l] = base + L.map[l];
  INSTAG_TRY(forward(w, frames, B, H, W, maps, base, L, (hipStream_t)stream));
  return launch_tail(maps, B, H, W, boxes, count, overflow, (hipStream_t)stream);
}

int instag_face_detect_pool(const float* in, float* out, int32_t planes, int32_t hi, int32_t wi, int32_t border,
                            instag_stream_t stream) {
  INSTAG_REQUIRE(in && out, "face_detect_pool: NULL tensor");
  INSTAG_REQUIRE(planes >= 1 && hi >= 2 && wi >= 2 && hi % 2 == 0 && wi % 2 == 0 && hi <= 4096 && wi <= 4096 &&
                     (size_t)planes * hi * wi < ((size_t)1 << 31),
                 "face_detect_pool: planes >= 1, hi and wi even in [2, 4096], planes * hi * wi < 2^31");
  INSTAG_REQUIRE(border >= 0 && border <= 8, "face_detect_pool: border in [0, 8]");
  return launch_pool(in, out, (size_t)planes, hi, wi, border, (hipStream_t)stream);
}

int instag_face_detect_l2norm(const float* in, const float* weight, float* out, int32_t B, int32_t C, int32_t hw,
                              instag_stream_t stream) {
  INSTAG_REQUIRE(in && weight && out, "face_detect_l2norm: NULL tensor");
  INSTAG_REQUIRE(B >= 1 && C >= 1 && C <= 1024 && hw >= 1 && (size_t)B * C * hw < ((size_t)1 << 31),
                 "face_detect_l2norm: B >= 1, C in [1, 1024], hw >= 1, B * C * hw < 2^31");
  return launch_l2norm(in, weight, out, B, C, hw, (hipStream_t)stream);
}

}  // extern "C"
