/* C ABI of the per-frame codes of a 'hubert' head (csrc/audio.hip), the third instag_frame_code family.  Part of
 * libinstag_hip.so; written in the C subset of instag_hip.h and read by the same reader (instag_amd/_cabi.py), so the
 * ctypes side is derived from this text.  The error codes, instag_stream_t and instag_last_error are instag_hip.h's.
 */
#ifndef INSTAG_FRAME_CODE_WIDE_H
#define INSTAG_FRAME_CODE_WIDE_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The codes of instag_frame_code_* for a network whose AudioNet reads windows of TWO samples of dim_in
 * features (audio_extractor == 'hubert': a [8, 1024, 2]):
 *   enc_a [1, dim_aud] = AudioAttNet(AudioNet(a)), enc_e [6] = cat(exp_encode_net(e[:5]), e[5:]).
 * AudioNet's slice x[:, :, 0:16] keeps both samples, so the lengths of its four k3 s2 p1 convolutions go
 * 2 -> 1 -> 1 -> 1 -> 1: in encoder_conv.0 taps 1 and 2 meet the two samples and tap 0 only padding, in
 * encoder_conv.{2,4,6} only the centre tap is live.
 * a [8, dim_in, 2], e [6] or NULL (then enc_e NULL).  `params` / `grads` are HOST arrays of 26 DEVICE pointers
 * in the order of instag_frame_code_* (instag_hip.h); the last two may be NULL when e is NULL.
 * Supported: mid == 128, dim_in in {256, 512, 768, 1024}, any dim_aud >= 1 whose two passes fit 160 KB of LDS.
 * Anything else: instag_frame_code_wide_saved_floats returns -1 and the entry points return INSTAG_E_ARG before
 * any device work.
 * Semantics of instag_frame_code_ave_*: forward keeps the activations backward reads in `saved`
 * (instag_frame_code_wide_saved_floats floats); backward OVERWRITES every grads[i], the dead taps with 0.0
 * (grads may be uninitialised memory); no gradient flows to a or e; no atomics on floats, two runs give the
 * same bits.  A weight or gradient of encoder_conv.0 that is not 16-byte aligned is read / written 4 bytes at a time.
 * arrivals (device uint32, ZERO before the first call, one word per set of calls that may overlap): the 128
 * neurons of encoder_conv.0 are split over 16 workgroups, each reads its rows of the weight once for all eight
 * windows, the last one to arrive runs the rest and leaves the word zero again.  NULL selects the
 * single-workgroup form.  backward runs on 16 workgroups that write disjoint rows of encoder_conv.0's weight
 * gradient: it needs no workspace (workspace may be NULL, workspace_bytes is not read).
 * ------------------------------------------------------------------------------------------ */
int64_t instag_frame_code_wide_saved_floats(int32_t dim_in, int32_t mid, int32_t dim_aud);
int instag_frame_code_wide_forward(const float* a, const float* e, const float* const* params, float* enc_a,
                                   float* enc_e, float* saved, int32_t dim_in, int32_t mid, int32_t dim_aud,
                                   uint32_t* arrivals, instag_stream_t stream);
int instag_frame_code_wide_backward(const float* a, const float* e, const float* const* params, const float* saved,
                                    const float* d_enc_a, const float* d_enc_e, float* const* grads, int32_t dim_in,
                                    int32_t mid, int32_t dim_aud, void* workspace, size_t workspace_bytes,
                                    instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
