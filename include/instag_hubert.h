/* C ABI of the HuBERT encoder (csrc/hubert.hip), the audio features of a 'hubert' head.  Part of libinstag_hip.so;
 * written in the C subset of instag_hip.h and read by the same reader (instag_amd/_cabi.py), which is told of the
 * structs of instag_wav2vec.h, so the ctypes side is derived from this text.  The error codes, instag_stream_t and
 * instag_last_error are instag_hip.h's; the weights are instag_wav2vec.h's struct.
 */
#ifndef INSTAG_HUBERT_H
#define INSTAG_HUBERT_H

#include "instag_wav2vec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSTAG_HUBERT_MAX_FRAMES 1024

/* ------------------------------------------------------------------------------------------
 * HuBERT "large" (facebook/hubert-large-ls960-ft): the network of instag_wav2vec.h without its head, fp32,
 * forward only: input_values [B,n] -> hidden [B,T,hidden] = LayerNorm(h; enc_ln), T = (n - 400) / 320 + 1,
 * transformers' HubertModel(input_values).last_hidden_state.
 *
 *  input_values are taken as given: the processor normalises the whole utterance, not a clip, so that is
 *  the caller's.  head_w, head_b and vocab are neither read nor required.  The weights' layouts, the shape
 *  rules but vocab's, tile and taps (instag_hubert_taps_floats floats, the wav2vec order and sizes) are as
 *  in instag_wav2vec.h; 400 <= n <= 2^20 and T <= INSTAG_HUBERT_MAX_FRAMES.  Anything else: INSTAG_E_ARG
 *  before any device work (workspace_bytes: 0); INSTAG_E_SPACE for a short workspace.
 *
 *  Every layer's attention, at every T, is instag_hubert_attention:
 *    ctx[b, t, head * 64 + d] = sum_c softmax_c(q[b, t, head] . k[b, c, head] / 8) v[b, c, head * 64 + d]
 *  for qkv [B, frames, 3 * 64 heads] (q | k | v) and ctx [B, frames, 64 heads], 1 <= frames <=
 *  INSTAG_HUBERT_MAX_FRAMES, 1 <= heads <= 65535, 1 <= batch <= 4096.  A workgroup owns 64 query rows of one
 *  (segment, head) and walks the keys in tiles of 64 with a running maximum and sum per row; both products
 *  run on the f32-input MFMA, the scores stay in registers, the LDS need does not depend on frames.
 *
 *  No atomics, a fixed summation order: a segment's bits do not depend on the batch it sat in or on the
 *  tile, and repeated runs give the same bits.
 * ------------------------------------------------------------------------------------------ */
size_t instag_hubert_workspace_bytes(const instag_wav2vec_weights* w, int32_t batch, int32_t n_samples);
size_t instag_hubert_taps_floats(const instag_wav2vec_weights* w, int32_t batch, int32_t n_samples);
int instag_hubert_forward(const instag_wav2vec_weights* w, const float* input_values, int32_t batch, int32_t n_samples,
                          float* hidden, void* workspace, size_t workspace_bytes, int32_t tile, float* taps,
                          instag_stream_t stream);
int instag_hubert_attention(const float* qkv, float* ctx, int32_t batch, int32_t frames, int32_t heads,
                            instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
