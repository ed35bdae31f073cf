// Evaluation of a trained head on the device (gfx950): frame metrics and the inference epilogue.
//
// instag_frame_metrics: L1, MSE, PSNR (both forms) and SSIM of B frame pairs in one tile launch plus one small
// finalize launch.  The reference scores its result twice: train_face.py:821-878 (L1 and utils/image_utils.py psnr on
// held-out cameras) and metrics.py:105-217 (PSNR of the 8-bit frames of the two videos); SSIM is utils/loss_utils.py:42-72
// (11 taps, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2).  One workgroup takes one 16x16 tile of one channel of
// one frame: the 26x26 halo of both images is staged in LDS once (clamped / quantised on the way in), the five windowed
// moments run separably (horizontal pass into LDS, vertical pass in registers), and the tile's three sums go to a
// workspace.  Nothing else is written: no derivative maps (the training kernel of ssim.hip stores 3*C*H*W floats for its
// backward).
//
// Precision.  The pixels are fp32; every sum over them -- the window moments, the tile sums, the sums over tiles -- is
// carried in fp64.  An evaluation figure is read to six digits and compared between runs, and sigma^2 = E[x^2] - mu^2
// loses most of an fp32 mantissa on flat regions; the kernel is bound by its LDS traffic, not by the adds.  Every
// reduction has a fixed order (no float atomics): repeated runs and graph replays give the same bits.
//
// instag_infer_compose: synthesize_fuse.py:65-76 in one forward-only launch -- the optional dilation of the mouth alpha
// (a running maximum from an LDS tile), both compositions, the clamp and the 8-bit frame.
#include "common.hpp"
#include "device_math.hpp"

#include <cmath>

namespace instag {
namespace {

constexpr int TS = 16;            // tile side
constexpr int RAD = 5;            // 11 taps
constexpr int HS = TS + 2 * RAD;  // 26
constexpr int MAX_DILATE = 31;
constexpr int DHS = TS + MAX_DILATE - 1;   // 46
constexpr int F_CLAMP = 1, F_QUANT = 2;

// The fp32 window losses._window builds (exp(-(x-5)^2 / 4.5) in fp32, divided by its fp32 sum), bit for bit.
__device__ constexpr float GW[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f,
                                     0x1.10656p-2f,   0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f,
                                     0x1.0d956cp-10f};

// What a video frame keeps of a value: float(int(clamp(x, 0, 1) * 255)) / 255, truncating.  __fmul_rn / __fdiv_rn are
// single correctly rounded fp32 operations that the compiler neither contracts nor turns into a reciprocal multiply, so
// the operands are the floats metrics.py:205-206 feeds its meters.
__device__ __forceinline__ float quantise(float x) {
  const float c = fminf(fmaxf(x, 0.f), 1.f);
  return __fdiv_rn((float)(int)__fmul_rn(c, 255.f), 255.f);
}

__device__ __forceinline__ float prepare(float v, bool clamp, bool quant) {
  if (quant) return quantise(v);
  return clamp ? fminf(fmaxf(v, 0.f), 1.f) : v;
}

// partials [B][3][tiles][3] doubles: (SSIM map sum, sum |d|, sum d^2) of one tile of one channel of one frame
__global__ void __launch_bounds__(256)
frame_metrics_tile_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W, int flags,
                          double* __restrict__ partials) {
  __shared__ float s_x[HS][HS + 1], s_y[HS][HS + 1];
  __shared__ double s_h[5][HS][TS + 1];
  __shared__ double s_red[3][4];
  const int bc = blockIdx.z;                       // frame * 3 + channel
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
  const size_t plane = (size_t)H * W;
  const float* p1 = pred + (size_t)bc * plane;
  const float* p2 = gt + (size_t)bc * plane;
  const bool quant = (flags & F_QUANT) != 0, clamp = (flags & F_CLAMP) != 0;
  for (int i = threadIdx.x; i < HS * HS; i += 256) {
    const int ly = i / HS, lx = i - ly * HS;
    const int gy = y0 + ly - RAD, gx = x0 + lx - RAD;
    float xv = 0.f, yv = 0.f;                      // zero padding (of the prepared images)
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      xv = prepare(p1[(size_t)gy * W + gx], clamp, quant);
      yv = prepare(p2[(size_t)gy * W + gx], false, quant);
    }
    s_x[ly][lx] = xv;
    s_y[ly][lx] = yv;
  }
  __syncthreads();
  // horizontal pass: HS rows x TS columns x 5 moments
  for (int i = threadIdx.x; i < HS * TS; i += 256) {
    const int ly = i / TS, lx = i - ly * TS;
    double a = 0., b = 0., aa = 0., bb = 0., ab = 0.;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const double xv = s_x[ly][lx + k], yv = s_y[ly][lx + k], w = GW[k];
      const double wx = w * xv, wy = w * yv;
      a += wx; b += wy; aa += wx * xv; bb += wy * yv; ab += wx * yv;
    }
    s_h[0][ly][lx] = a; s_h[1][ly][lx] = b; s_h[2][ly][lx] = aa; s_h[3][ly][lx] = bb; s_h[4][ly][lx] = ab;
  }
  __syncthreads();
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int gx = x0 + tx, gy = y0 + ty;
  double v[3] = {0., 0., 0.};
  if (gx < W && gy < H) {                          // (uniform control flow is not needed below: no barrier inside)
    double mu1 = 0., mu2 = 0., e11 = 0., e22 = 0., e12 = 0.;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const double w = GW[k];
      mu1 += w * s_h[0][ty + k][tx]; mu2 += w * s_h[1][ty + k][tx];
      e11 += w * s_h[2][ty + k][tx]; e22 += w * s_h[3][ty + k][tx]; e12 += w * s_h[4][ty + k][tx];
    }
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
    const double s11 = e11 - mu1s, s22 = e22 - mu2s, s12 = e12 - mu12;
    v[0] = ((2. * mu12 + C1) * (2. * s12 + C2)) / ((mu1s + mu2s + C1) * (s11 + s22 + C2));
    const double d = (double)s_x[ty + RAD][tx + RAD] - (double)s_y[ty + RAD][tx + RAD];
    v[1] = fabs(d);
    v[2] = d * d;
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double w = wave_sum(v[q]);
    if ((threadIdx.x & 63) == 0) s_red[q][wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    const size_t tiles = (size_t)gridDim.x * gridDim.y;
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partials[((size_t)bc * tiles + tile) * 3 + q] = ((s_red[q][0] + s_red[q][1]) + s_red[q][2]) + s_red[q][3];
  }
}

// One workgroup of 16 waves; wave w folds frames w, w + 16, ... (lane-strided over the tiles, then a butterfly: a fixed
// order), lane 0 turns the nine sums into the five figures.  Thread 0 adds the valid frames into the meter in frame order.
constexpr int FIN_WAVES = 16;

__global__ void __launch_bounds__(FIN_WAVES * 64)
frame_metrics_finalize_kernel(const double* __restrict__ partials, int B, int tiles, double npix, int n_valid,
                              float* __restrict__ per_frame, double* __restrict__ meter) {
  __shared__ float s_val[FIN_WAVES][5];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc[5] = {0., 0., 0., 0., 0.};
  int count = 0;
  for (int base = 0; base < B; base += FIN_WAVES) {
    const int b = base + wave;
    if (b < B) {
      double s[3][3];                              // [channel][ssim, |d|, d^2]
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double* p = partials + ((size_t)(b * 3 + c) * tiles) * 3;
        double a0 = 0., a1 = 0., a2 = 0.;
        for (int t = lane; t < tiles; t += 64) {
          a0 += p[(size_t)t * 3]; a1 += p[(size_t)t * 3 + 1]; a2 += p[(size_t)t * 3 + 2];
        }
        s[c][0] = wave_sum(a0); s[c][1] = wave_sum(a1); s[c][2] = wave_sum(a2);
      }
      if (lane == 0) {
        const double n3 = 3. * npix;
        const double mse = ((s[0][2] + s[1][2]) + s[2][2]) / n3;
        double rgb = 0.;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb += 20. * log10(1. / sqrt(s[c][2] / npix));   // image_utils.psnr, per channel
        const float out[5] = {(float)(((s[0][1] + s[1][1]) + s[2][1]) / n3), (float)mse,
                              (float)(-10. * log10(mse)),                           // mse == 0 -> +inf, as numpy
                              (float)(rgb / 3.), (float)(((s[0][0] + s[1][0]) + s[2][0]) / n3)};
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          per_frame[(size_t)b * 5 + j] = out[j];
          s_val[wave][j] = out[j];
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0 && meter != nullptr) {
      for (int k = 0; k < FIN_WAVES && base + k < n_valid; ++k) {
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[j] += (double)s_val[k][j];
        ++count;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && meter != nullptr) {
#pragma unroll
    for (int j = 0; j < 5; ++j) meter[j] += acc[j];
    meter[5] += (double)count;
  }
}

// slot[0] += values[0] + ... + values[n - 1] (in order), slot[1] += n: a further figure (LPIPS) in the meter's state
__global__ void meter_add_kernel(const float* __restrict__ values, int n, double* __restrict__ slot) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.;
  for (int i = 0; i < n; ++i) a += (double)values[i];
  slot[0] += a;
  slot[1] += (double)n;
}

struct ComposeArgs {
  const float* face; const float* a_face; const float* mouth; const float* a_mouth; const float* bg;
  const float* scene; float* image; uint8_t* frame_u8; int H, W, dilate, packed;
};

// One 16x16 tile per workgroup.  a_d = the dilate x dilate running maximum of the mouth alpha (stride 1; positions
// outside the image do not take part: F.max_pool2d(a_m, dilate, 1, dilate // 2)), separably from an LDS tile with a
// dilate / 2 halo.  The rasterizer's flat background leaves with the RENDERED alphas; only the scene background sees a_d.
__global__ void __launch_bounds__(256)
infer_compose_kernel(ComposeArgs A) {
  __shared__ float s_a[DHS][DHS + 1];
  __shared__ float s_m[DHS][TS + 1];
  __shared__ __attribute__((aligned(16))) uint8_t s_u8[TS][TS * 3];
  const int H = A.H, W = A.W, r = A.dilate >> 1, hs = TS + 2 * r;
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int gx = x0 + tx, gy = y0 + ty;
  const bool inside = gx < W && gy < H;
  const size_t plane = (size_t)H * W;
  const size_t pix = (size_t)gy * W + gx;
  float a_d = 0.f;
  if (r > 0) {                                     // (uniform: the barriers below are reached by every thread)
    for (int i = threadIdx.x; i < hs * hs; i += 256) {
      const int ly = i / hs, lx = i - ly * hs;
      const int sy = y0 + ly - r, sx = x0 + lx - r;
      s_a[ly][lx] = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? A.a_mouth[(size_t)sy * W + sx] : -INFINITY;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < hs * TS; i += 256) {
      const int ly = i / TS, lx = i - ly * TS;
      float m = s_a[ly][lx];
      for (int k = 1; k <= 2 * r; ++k) m = fmaxf(m, s_a[ly][lx + k]);
      s_m[ly][lx] = m;
    }
    __syncthreads();
    a_d = s_m[ty][tx];
    for (int k = 1; k <= 2 * r; ++k) a_d = fmaxf(a_d, s_m[ty + k][tx]);
  } else if (inside) {
    a_d = A.a_mouth[pix];
  }
  if (inside) {
    const float tf = 1.0f - A.a_face[pix], tm = 1.0f - A.a_mouth[pix], td = 1.0f - a_d;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float sc = A.scene ? A.scene[c * plane + pix] : 0.f;
      const float mi = (A.mouth[c * plane + pix] - A.bg[c] * tm) + sc * td;
      const float v = fminf(fmaxf((A.face[c * plane + pix] - A.bg[c] * tf) + mi * tf, 0.f), 1.f);
      A.image[c * plane + pix] = v;
      if (A.frame_u8) {
        const uint8_t q = (uint8_t)(int)__fmul_rn(v, 255.f);
        if (A.packed) s_u8[ty][tx * 3 + c] = q;
        else A.frame_u8[pix * 3 + c] = q;
      }
    }
  }
  if (A.frame_u8 && A.packed) {                    // (uniform) W % 16 == 0: full tile rows, 48 bytes = 3 x 16 each
    __syncthreads();
    if (threadIdx.x < TS * 3) {
      const int row = threadIdx.x / 3, part = threadIdx.x - row * 3;
      if (y0 + row < H) {
        const uint4 val = *reinterpret_cast<const uint4*>(&s_u8[row][part * 16]);
        *reinterpret_cast<uint4*>(A.frame_u8 + ((size_t)(y0 + row) * W + x0) * 3 + part * 16) = val;
      }
    }
  }
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

int64_t instag_frame_metrics_num_partials(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return (int64_t)B * 9 * div_up(H, TS) * div_up(W, TS);
}

int instag_frame_metrics(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W, int32_t flags,
                         double* partials, float* per_frame, double* meter, int32_t n_valid, instag_stream_t stream) {
  INSTAG_REQUIRE(pred && gt && partials && per_frame, "frame_metrics: NULL tensor");
  INSTAG_REQUIRE(B >= 1 && H >= 1 && W >= 1, "frame_metrics: bad shape");
  INSTAG_REQUIRE((int64_t)B * 3 <= 65535, "frame_metrics: at most 21845 frames per call");
  INSTAG_REQUIRE(div_up(H, TS) <= 65535 && (int64_t)div_up(H, TS) * div_up(W, TS) <= 0x7fffffffll,
                 "frame_metrics: image too large");
  INSTAG_REQUIRE((flags & ~(F_CLAMP | F_QUANT)) == 0, "frame_metrics: unknown flag");
  INSTAG_REQUIRE(n_valid >= 0 && n_valid <= B, "frame_metrics: n_valid must be in [0, B]");
  const dim3 grid(div_up(W, TS), div_up(H, TS), B * 3);
  frame_metrics_tile_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pred, gt, H, W, flags, partials);
  INSTAG_CHECK_LAUNCH();
  frame_metrics_finalize_kernel<<<1, FIN_WAVES * 64, 0, (hipStream_t)stream>>>(
      partials, B, (int)(grid.x * grid.y), (double)H * (double)W, n_valid, per_frame, meter);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_meter_add(const float* values, int32_t n, double* slot, instag_stream_t stream) {
  INSTAG_REQUIRE(values && slot, "meter_add: NULL tensor");
  INSTAG_REQUIRE(n >= 0, "meter_add: negative count");
  if (n == 0) return INSTAG_OK;
  meter_add_kernel<<<1, 64, 0, (hipStream_t)stream>>>(values, n, slot);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_infer_compose(const float* face, const float* a_face, const float* mouth, const float* a_mouth,
                         const float* bg, const float* scene, int32_t dilate, float* image, uint8_t* frame_u8,
                         int32_t H, int32_t W, instag_stream_t stream) {
  INSTAG_REQUIRE(face && a_face && mouth && a_mouth && bg && image, "infer_compose: NULL tensor");
  INSTAG_REQUIRE(H >= 1 && W >= 1 && div_up(H, TS) <= 65535, "infer_compose: bad image size");
  INSTAG_REQUIRE(dilate >= 1 && dilate <= MAX_DILATE && (dilate & 1), "infer_compose: dilate must be odd, 1 .. 31");
  // 16-byte stores of the byte frame need every tile row to start on a 16-byte boundary and to be whole
  const int packed = frame_u8 != nullptr && W % TS == 0 && ((uintptr_t)frame_u8 & 15) == 0;
  const ComposeArgs a{face, a_face, mouth, a_mouth, bg, scene, image, frame_u8, H, W, dilate, packed};
  infer_compose_kernel<<<dim3(div_up(W, TS), div_up(H, TS)), 256, 0, (hipStream_t)stream>>>(a);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
