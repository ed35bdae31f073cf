// Preparing an identity (gfx950): the shared background, the ground-truth frames and the torso frames from the decoded
// frames and their parsing maps -- data_utils/process.py:89-176 (extract_background) and :199-374
// (extract_torso_and_gt), as integer kernels on the 8-bit data.  Colours are RGB: head (0,0,255), neck (0,255,0),
// torso (255,0,0), background (255,255,255).
//
// instag_prep_background.  The reference asks a kd-tree for the distance from every pixel to the nearest
// non-background pixel of every sample, stacks the answers [S, H*W] in fp64 and takes max / argmax over S.  Here the
// exact SQUARED distance is computed in integers, separably:
//   nearest_in_row_kernel   one wave per image row: the column of the nearest set pixel of that row (u16, NONE if the
//                           row has none; of two at the same distance the left one), by a wave scan from each side.
//   column_max_kernel       a block owns a 16-column x 64-row band, a thread four of its pixels.  Per sample the
//                           strip's in-row distances g of ALL rows are staged in LDS as u16 (H * 16 * 2 bytes) and each
//                           pixel minimises g(y')^2 + (y - y')^2 outward from its own row, stopping once dy^2 reaches
//                           the minimum found.  The running maximum over the samples and the first sample attaining
//                           it (strictly-greater update = np.argmax) stay in registers across the sample loop; the
//                           [S, H*W] stack never exists.  (The row pass is kept for a chunk of samples at a time, so
//                           its workspace is bounded; between chunks the maximum rests in max_d2 / arg.)
//   known pixels (max_d2 > 25, the reference's max_dist > 5) take ori[arg]; the others are filled by
//   fill_kernel                the same separable search over the known mask, carrying coordinates: smallest squared
//                           distance, then smallest row, then smallest column.
//
// instag_prep_frames.  Work is per image column, because every decision of the reference is: the topmost torso /
// dilated-neck pixel of a column, what lies above it, how many neck pixels the column has.
//   column_kernel           four threads per (frame, column), a quarter of the rows each: a first walk down the quarter
//                           finds its share of the two paint anchors (combined through LDS), a second writes gt and
//                           the torso RGBA of its rows (mask and alpha included).
//   blur_kernel             one thread per (frame, column, painted neck row): the 5x5 fixed-point Gaussian of the image
//                           as it stands after the neck paint.  That image is a pure function of the inputs and the
//                           per-column anchors, so it is re-evaluated per tap rather than kept as a copy; nothing is
//                           read from the buffer being written.
#include "common.hpp"

namespace instag {
namespace {

constexpr uint32_t NONE16 = 0xffffu;
constexpr int STRIP = 16;             // columns of a band
constexpr int BAND = 64;              // rows of a band: 16 thread rows x PIX
constexpr int PIX = 4;
constexpr int MAX_SIDE = 2048;        // H * STRIP * 2 bytes of LDS <= 64 KiB; columns fit u16 below NONE16
constexpr int KNOWN_D2 = 25;
constexpr int L_TORSO = 9, L_NECK = 53, PUSH_DOWN = 4;
constexpr int ROW_PARTS = 4;          // a column's rows are shared by this many threads
constexpr int BIG = 0x3fffffff;

__device__ __forceinline__ bool is_rgb(const uint8_t* p, uint32_t r, uint32_t g, uint32_t b) {
  return p[0] == r && p[1] == g && p[2] == b;
}

// ---- the nearest set pixel of every row ---------------------------------------------------------------------------
// mode 0: rows of `n_img` parsing images (set = not background); mode 1: rows of max_d2 (set = known).
// nearest [rows, W] u16; any[image] = 1 if the image has a set pixel (cleared by the caller).
__global__ void __launch_bounds__(256) nearest_in_row_kernel(const uint8_t* __restrict__ parsing,
                                                             const int32_t* __restrict__ max_d2, int mode, int rows, int H,
                                                             int W, uint16_t* __restrict__ nearest, int32_t* __restrict__ any) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;                         // (whole waves leave: a wave is one row)
  const size_t base = (size_t)row * W;
  auto set_at = [&](int x) -> bool {
    if (mode == 0) return !is_rgb(parsing + (base + x) * 3, 255u, 255u, 255u);
    return max_d2[base + x] > KNOWN_D2;
  };
  int carry = -1;                                  // nearest set column at or left of the chunk's start
  for (int x0 = 0; x0 < W; x0 += 64) {
    const int x = x0 + lane;
    int v = (x < W && set_at(x)) ? x : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v = max(v, t);
    }
    v = max(v, carry);
    if (x < W) nearest[base + x] = (uint16_t)(v < 0 ? NONE16 : (uint32_t)v);
    carry = __shfl(v, 63);
  }
  if (carry >= 0 && lane == 0) any[row / H] = 1;   // (every writer writes the same value)
  carry = BIG;
  for (int x0 = (W - 1) / 64 * 64; x0 >= 0; x0 -= 64) {
    const int x = x0 + lane;
    int v = (x < W && set_at(x)) ? x : BIG;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(v, o);
      if (lane + o < 64) v = min(v, t);
    }
    v = min(v, carry);
    if (x < W && v != BIG) {
      const uint32_t l = nearest[base + x];
      if (l == NONE16 || v - x < x - (int)l) nearest[base + x] = (uint16_t)v;     // a tie keeps the left one
    }
    carry = __shfl(v, 0);
  }
}

// ---- the column pass of the distance, and the running maximum over the samples ---------------------------------------
// grid (strips, bands).  nearest: the row pass of samples [s0, s0 + n).  max_d2 / arg: read when s0 > 0, written.
__global__ void __launch_bounds__(256) column_max_kernel(const uint16_t* __restrict__ nearest, int s0, int n, int H, int W,
                                                         int32_t* __restrict__ max_d2, int32_t* __restrict__ arg) {
  extern __shared__ uint16_t g_lds[];              // [H][STRIP]
  const int cx = threadIdx.x % STRIP, ty = threadIdx.x / STRIP;
  const int x = blockIdx.x * STRIP + cx;
  const int y0 = blockIdx.y * BAND + ty;
  int best[PIX], who[PIX];
#pragma unroll
  for (int j = 0; j < PIX; ++j) {
    const int y = y0 + 16 * j;
    const bool in = x < W && y < H;
    best[j] = (in && s0 > 0) ? max_d2[(size_t)y * W + x] : -1;
    who[j] = (in && s0 > 0) ? arg[(size_t)y * W + x] : 0;
  }
  for (int s = 0; s < n; ++s) {
    __syncthreads();                               // the previous sample's strip has been read
    for (int i = threadIdx.x; i < H * STRIP; i += 256) {
      const int yy = i / STRIP, xx = blockIdx.x * STRIP + i % STRIP;
      uint32_t g = NONE16;
      if (xx < W) {
        const uint32_t c = nearest[((size_t)s * H + yy) * W + xx];
        if (c != NONE16) g = (uint32_t)abs(xx - (int)c);
      }
      g_lds[i] = (uint16_t)g;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
      const int y = y0 + 16 * j;
      if (x >= W || y >= H) continue;
      int m = BIG;
      const uint32_t g0 = g_lds[y * STRIP + cx];
      if (g0 != NONE16) m = (int)(g0 * g0);
      for (int dy = 1; dy * dy < m; ++dy) {
        const int up = y - dy, dn = y + dy;
        if (up < 0 && dn >= H) break;
        if (up >= 0) {
          const uint32_t g = g_lds[up * STRIP + cx];
          if (g != NONE16) m = min(m, (int)(g * g) + dy * dy);
        }
        if (dn < H) {
          const uint32_t g = g_lds[dn * STRIP + cx];
          if (g != NONE16) m = min(m, (int)(g * g) + dy * dy);
        }
      }
      if (m > best[j]) { best[j] = m; who[j] = s0 + s; }
    }
  }
#pragma unroll
  for (int j = 0; j < PIX; ++j) {
    const int y = y0 + 16 * j;
    if (x < W && y < H) { max_d2[(size_t)y * W + x] = best[j]; arg[(size_t)y * W + x] = who[j]; }
  }
}

// ---- the background image: known pixels from their sample, the others from the nearest known pixel -------------------
// grid (strips, bands).  nearest: the row pass over the known mask.
__global__ void __launch_bounds__(256) fill_kernel(const uint8_t* __restrict__ ori, const uint16_t* __restrict__ nearest,
                                                   const int32_t* __restrict__ max_d2, const int32_t* __restrict__ arg, int H,
                                                   int W, uint8_t* __restrict__ bc) {
  extern __shared__ uint16_t c_lds[];              // [H][STRIP]: column of the row's nearest known pixel
  for (int i = threadIdx.x; i < H * STRIP; i += 256) {
    const int yy = i / STRIP, xx = blockIdx.x * STRIP + i % STRIP;
    c_lds[i] = xx < W ? nearest[(size_t)yy * W + xx] : (uint16_t)NONE16;
  }
  __syncthreads();
  const int cx = threadIdx.x % STRIP, ty = threadIdx.x / STRIP;
  const int x = blockIdx.x * STRIP + cx;
  if (x >= W) return;
#pragma unroll
  for (int j = 0; j < PIX; ++j) {
    const int y = blockIdx.y * BAND + ty + 16 * j;
    if (y >= H) continue;
    int sy = y, sx = x;
    if (max_d2[(size_t)y * W + x] <= KNOWN_D2) {
      int m = BIG;
      sy = -1;
      const uint32_t c0 = c_lds[y * STRIP + cx];
      if (c0 != NONE16) { const int d = x - (int)c0; m = d * d; sy = y; sx = (int)c0; }
      // (dy^2 == m can still bring an equal distance in a smaller row; rows are visited smaller first within a dy, and
      // a later dy brings a smaller row only through `up`)
      for (int dy = 1; dy * dy <= m; ++dy) {
        const int up = y - dy, dn = y + dy;
        if (up < 0 && dn >= H) break;
        if (up >= 0) {
          const uint32_t c = c_lds[up * STRIP + cx];
          if (c != NONE16) {
            const int d = x - (int)c, v = d * d + dy * dy;
            if (v <= m) { m = v; sy = up; sx = (int)c; }       // equal: `up` is the smallest row seen so far
          }
        }
        if (dn < H) {
          const uint32_t c = c_lds[dn * STRIP + cx];
          if (c != NONE16) {
            const int d = x - (int)c, v = d * d + dy * dy;
            if (v < m) { m = v; sy = dn; sx = (int)c; }        // equal: every row seen before is smaller
          }
        }
      }
    }
    uint8_t* o = bc + ((size_t)y * W + x) * 3;
    if (sy < 0) { o[0] = o[1] = o[2] = 0; continue; }          // (no known pixel at all: the call reports it)
    const size_t p = (size_t)sy * W + sx;
    const uint8_t* src = ori + ((size_t)arg[p] * H * W + p) * 3;
    o[0] = src[0]; o[1] = src[1]; o[2] = src[2];
  }
}

// ---- frames -----------------------------------------------------------------------------------------------------------
struct FramesArgs {
  const uint8_t* ori; const uint8_t* parsing; const uint8_t* bc; const uint8_t* table;   // table [L_NECK][256]
  uint8_t* gt; uint8_t* torso; int32_t* cols;                                             // cols [F][W][2]
  int F, H, W;
};

__device__ __forceinline__ int wrap(int y, int H) { return y < 0 ? y + H : y; }           // y in (-H, H)

// the ground-truth colour of pixel p (index into the frame) of frame f
__device__ __forceinline__ void gt_rgb(const FramesArgs& A, size_t fp, size_t p, uint32_t (&c)[3]) {
  const uint8_t* par = A.parsing + (fp + p) * 3;
  const uint8_t* s = is_rgb(par, 255u, 255u, 255u) ? A.bc + p * 3 : A.ori + (fp + p) * 3;
  c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
}

// the torso image as it stands after the neck paint (before the blur, before the mask), pixel (y, x) of frame f;
// a3 / a4: the column's anchors (-1: none)
__device__ __forceinline__ void painted_rgb(const FramesArgs& A, size_t fp, int y, int x, int a3, int a4, uint32_t (&c)[3]) {
  const int H = A.H, W = A.W;
  const int k4 = a4 >= 0 ? wrap(a4 - y, H) : L_NECK, k3 = a3 >= 0 ? wrap(a3 - y, H) : L_TORSO;
  if (k4 < L_NECK || k3 < L_TORSO) {
    const int k = k4 < L_NECK ? k4 : k3, a = k4 < L_NECK ? a4 : a3;
    gt_rgb(A, fp, (size_t)a * W + x, c);
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = A.table[k * 256 + c[i]];
    return;
  }
  const size_t p = (size_t)y * W + x;
  const uint8_t* par = A.parsing + (fp + p) * 3;
  const bool from_bc = is_rgb(par, 255u, 255u, 255u) || is_rgb(par, 0u, 0u, 255u);
  const uint8_t* s = from_bc ? A.bc + p * 3 : A.ori + (fp + p) * 3;
  c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
}

// grid (W / 64, F), block (64, ROW_PARTS): a wave owns 64 columns of one part of the rows, a thread one column of it
__global__ void __launch_bounds__(64 * ROW_PARTS) column_kernel(FramesArgs A) {
  __shared__ int s_torso[ROW_PARTS][64], s_neck[ROW_PARTS][64], s_count[ROW_PARTS][64];
  const int lane = threadIdx.x, part = threadIdx.y;
  const int x = blockIdx.x * 64 + lane, f = blockIdx.y;
  const int H = A.H, W = A.W;
  const bool live = x < W;
  const int per = (H + ROW_PARTS - 1) / ROW_PARTS;
  const int r0 = min(H, part * per), r1 = min(H, r0 + per);
  const size_t fp = (size_t)f * H * W;
  const uint8_t* par = A.parsing + (fp + (live ? x : 0)) * 3;
  const size_t row = (size_t)W * 3;
  auto neck_at = [&](int r) -> uint32_t { return r >= 0 && r < H ? (uint32_t)is_rgb(par + (size_t)r * row, 0u, 255u, 0u) : 0u; };
  // first walk, over the part and three rows either side of it: the part's topmost torso row, its topmost dilated-neck
  // row and its dilated-neck count (H = none).  Bit i of `win` = neck at row r - i, so the dilated neck of row r - 3
  // is win != 0.
  int top_torso = H, top_neck = H, count = 0;
  if (live) {
    uint32_t win = 0;
    for (int r = r0 - 3; r < r1 + 3; ++r) {
      win = (win << 1 | neck_at(r)) & 0x7fu;
      if (r >= r0 && r < r1 && top_torso == H && is_rgb(par + (size_t)r * row, 255u, 0u, 0u)) top_torso = r;
      if (r - 3 >= r0 && win) { ++count; if (top_neck == H) top_neck = r - 3; }
    }
  }
  s_torso[part][lane] = top_torso; s_neck[part][lane] = top_neck; s_count[part][lane] = count;
  __syncthreads();
  if (!live) return;
  top_torso = top_neck = H; count = 0;
#pragma unroll
  for (int p = 0; p < ROW_PARTS; ++p) {
    top_torso = min(top_torso, s_torso[p][lane]);
    top_neck = min(top_neck, s_neck[p][lane]);
    count += s_count[p][lane];
  }
  int a3 = -1, a4 = -1;
  if (top_torso < H && is_rgb(par + (size_t)wrap(top_torso - 1, H) * row, 0u, 0u, 255u)) a3 = top_torso;
  if (top_neck < H && is_rgb(par + (size_t)wrap(top_neck - 1, H) * row, 0u, 0u, 255u))
    a4 = top_neck + min(count - 1, PUSH_DOWN);     // (count - 1 further set rows lie below top_neck: inside the image)
  if (part == 0) {
    A.cols[((size_t)f * W + x) * 2] = a3;
    A.cols[((size_t)f * W + x) * 2 + 1] = a4;
  }
  uint32_t c3[3] = {0u, 0u, 0u}, c4[3] = {0u, 0u, 0u};
  if (a3 >= 0) gt_rgb(A, fp, (size_t)a3 * W + x, c3);
  if (a4 >= 0) gt_rgb(A, fp, (size_t)a4 * W + x, c4);
  // second walk: the gt and torso pixel of every row of the part.  The neck paint's rows get their colour here as well;
  // blur_kernel replaces it.
  uint32_t win = 0;
  for (int r = r0 - 3; r < r0 + 3; ++r) win = win << 1 | neck_at(r);
  for (int y = r0; y < r1; ++y) {
    const size_t p = (size_t)y * W + x;
    const uint8_t* q = par + (size_t)y * row;
    const uint32_t ahead = y + 3 < H ? (uint32_t)is_rgb(par + (size_t)(y + 3) * row, 0u, 255u, 0u) : 0u;
    win = (win << 1 | ahead) & 0x7fu;              // neck at rows y + 3 .. y - 3
    const bool bg = is_rgb(q, 255u, 255u, 255u), head = is_rgb(q, 0u, 0u, 255u), tor = is_rgb(q, 255u, 0u, 0u);
    const uint8_t* o = A.ori + (fp + p) * 3;
    const uint8_t* b = A.bc + p * 3;
    uint32_t g[3], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      g[i] = bg ? b[i] : o[i];
      t[i] = head ? b[i] : g[i];
    }
    uint8_t* go = A.gt + (fp + p) * 3;
    go[0] = (uint8_t)g[0]; go[1] = (uint8_t)g[1]; go[2] = (uint8_t)g[2];
    const int k4 = a4 >= 0 ? wrap(a4 - y, H) : L_NECK, k3 = a3 >= 0 ? wrap(a3 - y, H) : L_TORSO;
    if (k4 < L_NECK) {
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = A.table[k4 * 256 + c4[i]];
    } else if (k3 < L_TORSO) {
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = A.table[k3 * 256 + c3[i]];
    }
    const bool inside = win != 0u || tor || k4 < L_NECK || k3 < L_TORSO;
    reinterpret_cast<uint32_t*>(A.torso)[fp + p] = inside ? (t[0] | t[1] << 8 | t[2] << 16 | 0xff000000u) : 0u;
  }
}

__device__ __forceinline__ int reflect101(int i, int n) { i = i < 0 ? -i : i; return i >= n ? 2 * n - 2 - i : i; }

// grid (W / 64, L_NECK, F): one thread per (column, painted row)
__global__ void __launch_bounds__(64) blur_kernel(FramesArgs A) {
  const int x = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y, f = blockIdx.z;
  const int H = A.H, W = A.W;
  if (x >= W) return;
  const int32_t* cols = A.cols + (size_t)f * W * 2;
  const int a4 = cols[x * 2 + 1];
  if (a4 < 0) return;
  const int y = wrap(a4 - k, H);
  const size_t fp = (size_t)f * H * W;
  constexpr uint32_t Q[5] = {48u, 53u, 54u, 53u, 48u};     // round(256 w), w ~ exp(-i^2 / 32), the centre takes the rest
  uint32_t sum[3] = {0u, 0u, 0u};
#pragma unroll
  for (int dx = -2; dx <= 2; ++dx) {
    const int xx = reflect101(x + dx, W);
    const int n3 = cols[xx * 2], n4 = cols[xx * 2 + 1];
    uint32_t h[3] = {0u, 0u, 0u};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
      uint32_t c[3];
      painted_rgb(A, fp, reflect101(y + dy, H), xx, n3, n4, c);
#pragma unroll
      for (int i = 0; i < 3; ++i) h[i] += Q[dy + 2] * c[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) sum[i] += Q[dx + 2] * h[i];
  }
  uint8_t* o = A.torso + (fp + (size_t)y * W + x) * 4;
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (uint8_t)((sum[i] + 32768u) >> 16);
}

inline int chunk_samples(int S, int H, int W) {
  const size_t per = (size_t)H * W * 2;
  const size_t n = ((size_t)64 << 20) / per;       // at most 64 MiB of row-pass results at a time
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)S, n));
}
inline size_t flags_offset(int S, int H, int W) { return align_up((size_t)chunk_samples(S, H, W) * H * W * 2, 256); }

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_prep_background_workspace_bytes(int32_t S, int32_t H, int32_t W) {
  if (S < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return 0;
  return flags_offset(S, H, W) + align_up(((size_t)S + 1) * sizeof(int32_t), 256);
}

int instag_prep_background(const uint8_t* ori, const uint8_t* parsing, int32_t S, int32_t H, int32_t W, uint8_t* bc,
                           int32_t* max_d2, int32_t* arg, void* workspace, size_t workspace_bytes,
                           instag_stream_t stream) {
  INSTAG_REQUIRE(ori && parsing && bc && max_d2 && arg && workspace, "prep_background: NULL tensor");
  INSTAG_REQUIRE(S >= 1 && S <= (1 << 20), "prep_background: 1 .. 2^20 samples");
  INSTAG_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "prep_background: image sides in 1 .. 2048");
  INSTAG_REQUIRE((((uintptr_t)max_d2 | (uintptr_t)arg | (uintptr_t)workspace) & 3) == 0, "prep_background: misaligned tensor");
  if (workspace_bytes < instag_prep_background_workspace_bytes(S, H, W)) {
    set_error("prep_background: workspace too small");
    return INSTAG_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  uint16_t* nearest = reinterpret_cast<uint16_t*>(workspace);
  int32_t* any = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(workspace) + flags_offset(S, H, W));
  INSTAG_CHECK_HIP(hipMemsetAsync(any, 0, ((size_t)S + 1) * sizeof(int32_t), st));
  const int chunk = chunk_samples(S, H, W);
  const dim3 bands(div_up(W, STRIP), div_up(H, BAND));
  const size_t lds = (size_t)H * STRIP * sizeof(uint16_t);
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int n = std::min(chunk, S - s0);
    const int rows = n * H;
    nearest_in_row_kernel<<<div_up(rows, 4), 256, 0, st>>>(parsing + (size_t)s0 * H * W * 3, nullptr, 0, rows, H, W,
                                                           nearest, any + s0);
    INSTAG_CHECK_LAUNCH();
    column_max_kernel<<<bands, 256, lds, st>>>(nearest, s0, n, H, W, max_d2, arg);
    INSTAG_CHECK_LAUNCH();
  }
  nearest_in_row_kernel<<<div_up(H, 4), 256, 0, st>>>(nullptr, max_d2, 1, H, H, W, nearest, any + S);
  INSTAG_CHECK_LAUNCH();
  fill_kernel<<<bands, 256, lds, st>>>(ori, nearest, max_d2, arg, H, W, bc);
  INSTAG_CHECK_LAUNCH();
  // the two conditions the reference would raise on (inside sklearn) are data: read them back
  std::string flags((size_t)(S + 1) * sizeof(int32_t), '\0');
  INSTAG_CHECK_HIP(hipMemcpyAsync(&flags[0], any, flags.size(), hipMemcpyDeviceToHost, st));
  INSTAG_CHECK_HIP(hipStreamSynchronize(st));
  const int32_t* fl = reinterpret_cast<const int32_t*>(flags.data());
  for (int s = 0; s < S; ++s)
    if (!fl[s]) {
      set_error("prep_background: sample " + std::to_string(s) + " has no non-background pixel");
      return INSTAG_E_ARG;
    }
  INSTAG_REQUIRE(fl[S] != 0, "prep_background: no pixel is ever farther than 5 from the foreground");
  return INSTAG_OK;
}

int instag_prep_frames(const uint8_t* ori, const uint8_t* parsing, const uint8_t* bc, const uint8_t* table, int32_t F,
                       int32_t H, int32_t W, uint8_t* gt, uint8_t* torso, int32_t* cols, instag_stream_t stream) {
  INSTAG_REQUIRE(ori && parsing && bc && table && gt && torso && cols, "prep_frames: NULL tensor");
  INSTAG_REQUIRE(F >= 1 && F <= 65535, "prep_frames: 1 .. 65535 frames per call");
  INSTAG_REQUIRE(H >= 64 && W >= 3 && H <= 16384 && W <= 16384, "prep_frames: H in 64 .. 16384, W in 3 .. 16384");
  INSTAG_REQUIRE((((uintptr_t)torso | (uintptr_t)cols) & 3) == 0, "prep_frames: torso and cols must be 4-byte aligned");
  const FramesArgs a{ori, parsing, bc, table, gt, torso, cols, F, H, W};
  hipStream_t st = (hipStream_t)stream;
  column_kernel<<<dim3(div_up(W, 64), F), dim3(64, ROW_PARTS), 0, st>>>(a);
  INSTAG_CHECK_LAUNCH();
  blur_kernel<<<dim3(div_up(W, 64), L_NECK, F), 64, 0, st>>>(a);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
