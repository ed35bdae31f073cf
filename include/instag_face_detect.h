/* C ABI of the face detector (csrc/face_detect.hip): S3FD, from uint8 frames to face boxes, what stands in front of the
 * landmark network (include/instag_landmarks.h).  Part of libinstag_hip.so; written in the C subset of instag_hip.h and
 * read by the same reader (instag_amd/_cabi.py), so the ctypes side is derived from this text.  The error codes,
 * instag_stream_t and instag_last_error are instag_hip.h's.
 */
#ifndef INSTAG_FACE_DETECT_H
#define INSTAG_FACE_DETECT_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSTAG_FACE_DETECT_LAYERS 25
#define INSTAG_FACE_DETECT_LEVELS 6
#define INSTAG_FACE_DETECT_MAX_CANDIDATES 4096
#define INSTAG_FACE_DETECT_MAX_FACES 16
#define INSTAG_FACE_DETECT_MAX_BATCH 64

/* ------------------------------------------------------------------------------------------
 * S3FD, fp32, forward only (instag_amd/face_detect.py states the network, the tail and this project's rules).
 *
 * Weights, device pointers to fp32.  w, scale, shift: one entry per convolution launch, the 19 trunk convolutions in
 * the order conv1_1 .. conv5_3, fc6, fc7, conv6_1, conv6_2, conv7_1, conv7_2, then the six heads in level order:
 *   w          [K = (cin, ky, kx)][cout].  conv1_1 reads the RGB frame: its input channels are the checkpoint's BGR ones
 *              reversed and its K = 27 is padded with zero rows to 32.  A head is the level's conf and loc
 *              convolutions as one of cout 6 (level 0: 8): the conf channels, then the four loc channels;
 *   scale, shift   [cout]: (1, bias).
 * norm: the three L2Norm weights, [256], [512], [512].
 *
 * The maps of a batch are six tensors fp32 [B, C, h, w] in level order, C = 8 at level 0 and 6 elsewhere (conf, then
 * loc), with h x w = H/4, H/8, H/16, then g = H/32 + 4 (fc6's padding of 3), (g - 1) / 2 + 1 and once more (the two
 * stride-2 convolutions); likewise for W.  `maps` is a host array of the six device pointers.
 *
 * instag_face_detect_forward: frames uint8 [B, H, W, 3] (RGB; they enter as BGR minus (104, 117, 123)) -> the maps.
 * instag_face_detect_post: the maps -> boxes fp32 [B, 16, 5] = (x1, y1, x2, y2, score) in descending score, the rows
 *   past the count NaN; count int32 [B], the true number of detections; overflow uint8 [B], 1 where the frame had more
 *   than INSTAG_FACE_DETECT_MAX_CANDIDATES candidates, of which the first that many in candidate order (level, y, x)
 *   entered.  Score = fp32(1 / (1 + exp(bg - face))) in fp64 on the fp32 logits, bg at level 0 the maximum of the first
 *   three conf channels; candidates have score > fp32(0.05); the decode and the greedy NMS (overlap with the + 1 of
 *   pixel boxes, a candidate survives a kept one where ovr <= 0.3, ties in score to the lower candidate index) are
 *   fp64; the detections are the kept candidates with score > 0.5.  One workgroup per frame, no atomics.
 * instag_face_detect: both; the maps live in the workspace.
 * instag_face_detect_pool: the 2 x 2 / stride 2 max-pool alone, in [planes, hi, wi] (hi, wi even) -> out [planes,
 *   hi / 2 + 2 border, wi / 2 + 2 border] with a zero border.  instag_face_detect_l2norm: in [B, C, hw] -> out =
 *   in / (sqrt(sum_c in^2) + 1e-10) * weight[c], the channels summed in a fixed order.  Both for the tests.
 *
 * H and W multiples of 32 in [64, 4096], 1 <= B <= INSTAG_FACE_DETECT_MAX_BATCH, B * 64 * H * W < 2^31.  Bad
 * arguments: INSTAG_E_ARG before any device work (workspace_bytes: 0); INSTAG_E_SPACE for a short workspace.  A frame's
 * bits depend neither on its batch nor on the tile a convolution chose.
 * ------------------------------------------------------------------------------------------ */
typedef struct instag_face_detect_weights {
  const float* w[25];
  const float* scale[25];
  const float* shift[25];
  const float* norm[3];
} instag_face_detect_weights;

size_t instag_face_detect_workspace_bytes(int32_t B, int32_t H, int32_t W);
int instag_face_detect_forward(const instag_face_detect_weights* w, const uint8_t* frames, int32_t B, int32_t H,
                               int32_t W, float* const* maps, void* workspace, size_t workspace_bytes,
                               instag_stream_t stream);
int instag_face_detect_post(const float* const* maps, int32_t B, int32_t H, int32_t W, float* boxes, int32_t* count,
                            uint8_t* overflow, instag_stream_t stream);
int instag_face_detect(const instag_face_detect_weights* w, const uint8_t* frames, int32_t B, int32_t H, int32_t W,
                       float* boxes, int32_t* count, uint8_t* overflow, void* workspace, size_t workspace_bytes,
                       instag_stream_t stream);
int instag_face_detect_pool(const float* in, float* out, int32_t planes, int32_t hi, int32_t wi, int32_t border,
                            instag_stream_t stream);
int instag_face_detect_l2norm(const float* in, const float* weight, float* out, int32_t B, int32_t C, int32_t hw,
                              instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
