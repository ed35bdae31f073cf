// What the JPEG encoder and decoder (mjpeg.hip, jpeg_decode.hip) share: the zig-zag order, the MCU grid of a frame, the
// shape both take and the rule that tells a block's component.  instag_amd/jpeg_common.py is the same on the Python side.
#pragma once
#include "common.hpp"
#include "instag_jpeg_decode.h"
#include "instag_mjpeg.h"

namespace instag {

static_assert(INSTAG_MJPEG_MAX_BATCH == INSTAG_JPEG_DECODE_MAX_BATCH && INSTAG_MJPEG_MAX_SIDE == INSTAG_JPEG_DECODE_MAX_SIDE,
              "one shape check serves both directions");

// zig-zag position k -> index in the 8 x 8 block, row by row (internal linkage: a copy per translation unit)
static __device__ const uint8_t d_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40,
                                                48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29,
                                                22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                                                47, 55, 62, 63};

// a frame as MCUs of 8 sub x 8 sub pixels: mx x my of them, `per` blocks each (sub^2 of Y, Cb, Cr), nblk blocks in all
struct JpegGrid {
  int H, W, sub, mx, my, per, nblk;
};
static inline JpegGrid jpeg_grid(int H, int W, int sub) {
  const int mx = div_up(W, 8 * sub), my = div_up(H, 8 * sub), per = sub * sub + 2;
  return {H, W, sub, mx, my, per, mx * my * per};
}

static inline bool jpeg_shape_ok(int B, int H, int W, int sub) {
  return B >= 1 && B <= INSTAG_MJPEG_MAX_BATCH && H >= 1 && H <= INSTAG_MJPEG_MAX_SIDE && W >= 1 &&
         W <= INSTAG_MJPEG_MAX_SIDE && (sub == 1 || sub == 2);
}
static const char* const JPEG_SHAPE_OK = ": 1 <= B <= 64, 1 <= H, W <= 4096, sub 1 (4:4:4) or 2 (4:2:0)";

// the component (0 Y, 1 Cb, 2 Cr) of block j of an MCU
__host__ __device__ inline int mcu_component(int j, int sub) { return j < sub * sub ? 0 : j - sub * sub + 1; }

}  // namespace instag
