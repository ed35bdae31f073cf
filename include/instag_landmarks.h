/* C ABI of the face landmark network (csrc/landmarks.hip): FAN-2D-4, the crop in front of it and the decode behind it,
 * what writes ori_imgs/<i>.lms.  Part of libinstag_hip.so; written in the C subset of instag_hip.h and read by the same
 * reader (instag_amd/_cabi.py), so the ctypes side is derived from this text.  The error codes, instag_stream_t and
 * instag_last_error are instag_hip.h's.
 */
#ifndef INSTAG_LANDMARKS_H
#define INSTAG_LANDMARKS_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSTAG_LANDMARKS_LAYERS 194
#define INSTAG_LANDMARKS_POINTS 68
#define INSTAG_LANDMARKS_STACKS 4
#define INSTAG_LANDMARKS_MIN_SIDE 64
#define INSTAG_LANDMARKS_MAX_SIDE 512
#define INSTAG_LANDMARKS_SIDE_MULTIPLE 64
#define INSTAG_LANDMARKS_MAX_BATCH 64
#define INSTAG_LANDMARKS_MAX_FRAME 8192
#define INSTAG_LANDMARKS_MAX_COORD 1048576

/* ------------------------------------------------------------------------------------------
 * FAN(num_modules = 4), eval mode, fp32, forward only (instag_amd/landmarks.py states the network and the layer order).
 *
 * Weights, device pointers to fp32, one entry per layer of landmarks.LAYERS:
 *   w          the convolution as [K = (cin, ky, kx)][cout]; the 7 x 7 stem's K = 147 padded with zero rows to 160 and
 *              al{i}'s K = 68 to 96;
 *   scale, shift   [cout], applied behind the convolution: BatchNorm folded for conv1 and conv_last{i}, (1, bias) for
 *              l{i}, bl{i}, al{i}, (1, 0) for the bias-free block convolutions;
 *   pre_scale, pre_shift   [cin]: the BatchNorm in FRONT of a block convolution or a downsample, folded; the
 *              convolution reads max(v pre_scale + pre_shift, 0) inside the image and zero outside.  NULL (both) where
 *              a layer has no pre-activation.
 *
 * instag_landmarks_forward: crops uint8 [B, S, S, 3] (RGB; they enter as u / 255) -> heatmaps fp32.  all_stacks == 0:
 * [B, 68, S / 4, S / 4], the last stack's; otherwise [B, 4, 68, S / 4, S / 4].  S a multiple of
 * INSTAG_LANDMARKS_SIDE_MULTIPLE in [MIN_SIDE, MAX_SIDE], 1 <= B <= INSTAG_LANDMARKS_MAX_BATCH.
 *
 * instag_landmarks_crop: frames uint8 [N, H, W, 3], boxes fp32 [B, 4] = (x1, y1, x2, y2), frame_index int32 [B] (the
 * frame of each box; NULL: box b belongs to frame b and N == B) -> crops uint8 [B, S, S, 3].  In fp64:
 *   center = (x2 - (x2 - x1) / 2, y2 - (y2 - y1) / 2 - 0.12 (y2 - y1)), h = 200 (x2 - x1 + y2 - y1) / 195,
 *   inv(p, res) = trunc(p h / res + center - h / 2), ul = inv(1, 256), br = inv(256, 256) per axis (256 whatever S is:
 *   the package's crop is defined at its own resolution),
 *   crop pixel (y, x) of the (br - ul) image = frame[y + ul_y][x + ul_x] inside the frame, 0 outside,
 * then a half-pixel-centre bilinear resize to S x S in integers: source position ((2 o + 1) n - S) / (2 S) of n source
 * pixels, its floor and the next index clamped to [0, n - 1], the fraction rounded half up to an integer weight of 512,
 * the weighted sum rounded half up to uint8 ((sum + 2^17) >> 18).  A box with a coordinate that is not finite or beyond
 * INSTAG_LANDMARKS_MAX_COORD in magnitude, or whose br - ul is below 1 on an axis, gives a zero crop.
 * H, W in [1, INSTAG_LANDMARKS_MAX_FRAME].
 *
 * instag_landmarks_decode: heatmaps fp32 [B, 68, R, R], boxes fp32 [B, 4] -> landmarks fp32 [B, 68, 2] = (x, y), whole
 * numbers: the first maximum (py, px) of a map; where 0 < px < R - 1 and 0 < py < R - 1, x += 0.25 sign(hm[py][px + 1] -
 * hm[py][px - 1]) and y likewise (sign(0) = 0); p = (px + 1, py + 1) + shift - 0.5; the landmark is inv(p, R).  A box as
 * refused above gives NaN.  R a multiple of 16 in [16, 128].
 *
 * instag_landmarks_conv is one convolution of the network's body alone (the tests drive the options of the shared
 * kernel through it): in fp32 [B, cin, H, W], w [K][cout] with K = cin ks ks rounded up to 32 and the rows past cin ks ks
 * zero, ks 1 or 3 (pad ks / 2, stride 1) -> channels out_off .. out_off + cout - 1 of out [B, out_ch, H, W] =
 * act(scale conv(pre(in)) + shift + res + nearest_x2(res2)): pre_scale / pre_shift [cin] or both NULL; res [B, out_ch, H,
 * W] and res2 [B, out_ch, H / 2, W / 2] (H and W even) are read at the same channels, or NULL; raw [B, cout, H, W] or
 * NULL receives scale conv + shift.  tile: 0, or 1 / 2 to pin the narrow / wide tile -- the bits do not depend on it.
 * 1 <= B <= INSTAG_LANDMARKS_MAX_BATCH, cin and out_ch in [1, 1024], H and W in [1, 256].
 *
 * Bad arguments: INSTAG_E_ARG before any device work (workspace_bytes: 0); INSTAG_E_SPACE for a short workspace.  No
 * atomics, a fixed K order: a face's bits depend neither on its batch nor on the tile chosen.
 * ------------------------------------------------------------------------------------------ */
typedef struct instag_landmarks_weights {
  const float* w[194];
  const float* scale[194];
  const float* shift[194];
  const float* pre_scale[194];
  const float* pre_shift[194];
} instag_landmarks_weights;

size_t instag_landmarks_workspace_bytes(int32_t B, int32_t S);
int instag_landmarks_forward(const instag_landmarks_weights* w, const uint8_t* crops, int32_t B, int32_t S,
                             int32_t all_stacks, float* heatmaps, void* workspace, size_t workspace_bytes,
                             instag_stream_t stream);
int instag_landmarks_crop(const uint8_t* frames, int32_t N, int32_t H, int32_t W, const float* boxes,
                          const int32_t* frame_index, int32_t B, int32_t S, uint8_t* crops, instag_stream_t stream);
int instag_landmarks_conv(const float* in, const float* w, const float* scale, const float* shift, const float* pre_scale,
                          const float* pre_shift, const float* res, const float* res2, float* raw, float* out, int32_t B,
                          int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t ks, int32_t out_ch, int32_t out_off,
                          int32_t relu, int32_t tile, instag_stream_t stream);
int instag_landmarks_decode(const float* heatmaps, const float* boxes, int32_t B, int32_t R, float* landmarks,
                            instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
