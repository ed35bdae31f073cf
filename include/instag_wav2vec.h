/* C ABI of the wav2vec 2.0 CTC network (csrc/wav2vec.hip), the audio features of an 'esperanto' head.  Part of
 * libinstag_hip.so; written in the C subset of instag_hip.h and read by the same reader (instag_amd/_cabi.py), so the
 * ctypes side is derived from this text.  The error codes, instag_stream_t and instag_last_error are instag_hip.h's.
 */
#ifndef INSTAG_WAV2VEC_H
#define INSTAG_WAV2VEC_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSTAG_WAV2VEC_MAX_LAYERS 48
#define INSTAG_WAV2VEC_MAX_FRAMES 128

/* ------------------------------------------------------------------------------------------
 * wav2vec 2.0 "stable layer norm" CTC model (feat_extract_norm "layer", conv_bias, gelu), fp32,
 * forward only: segments [B,n] of 16 kHz samples -> logits [B,T,vocab], T = (n - 400) / 320 + 1.
 *
 *  Per segment (x - mean) / sqrt(var + 1e-7); seven blocks GELU(LayerNorm_channels(conv1d(x) + b)) with
 *  kernels 10,3,3,3,3,2,2 and strides 5,2,2,2,2,2,2; LayerNorm, Linear to hidden;
 *  h += GELU(grouped conv1d(h, pos_kernel, padding pos_kernel / 2)[..., :-1]); per layer
 *  h += out(softmax(q k^T / 8) v) on LayerNorm(h) and h += W2 GELU(W1 LayerNorm(h)); LayerNorm; the head.
 *  LayerNorm eps 1e-5, no mask.
 *
 *  Activations are time-major [B,T,C]; every matrix is stored [K][N], N contiguous:
 *    conv_w[0] [10][conv_dim]; conv_w[l >= 1] [(tap, cin)][cout]; proj_w [conv_dim][hidden];
 *    pos_w [groups][(tap, cin in group)][cout in group], the weight norm folded by the caller;
 *    qkv_w[l] [hidden][3 hidden] (q | k | v), out_w[l] [hidden][hidden], ff1_w[l] [hidden][intermediate],
 *    ff2_w[l] [intermediate][hidden], head_w [hidden][vocab]; biases and LayerNorm gains as stored.
 *  Shapes: head dimension hidden / heads == 64; conv_dim, hidden, intermediate multiples of 32 and
 *  conv_dim, hidden <= 1024; pos_kernel even; hidden / pos_groups a multiple of 32; vocab a multiple of 4;
 *  1 <= layers <= INSTAG_WAV2VEC_MAX_LAYERS; 400 <= n and T <= INSTAG_WAV2VEC_MAX_FRAMES (the attention keeps
 *  a segment's scores in LDS).  Anything else: INSTAG_E_ARG before any device work (workspace_bytes: 0);
 *  INSTAG_E_SPACE for a short workspace.
 *  tile: 0, or 1 / 2 / 3 to run every GEMM on the 64 x 64 / 64 x 128 / 128 x 128 tile (tests).
 *  taps: NULL, or room for instag_wav2vec_taps_floats(w, batch, n_samples) floats (0 = bad argument) that
 *    receive a copy of every stage's output, one behind the other: the seven convolution blocks
 *    [B,T_l,conv_dim], the projection, h behind the positional convolution, and per layer h behind the
 *    attention and behind the feed-forward, each [B,T,hidden] (tests).
 *  No atomics, a fixed K order: a segment's logits do not depend on the batch it sat in or on the
 *  tile, and repeated runs give the same bits.
 * ------------------------------------------------------------------------------------------ */
typedef struct instag_wav2vec_weights {
  int32_t conv_dim, hidden, heads, intermediate, layers, pos_kernel, pos_groups, vocab;
  const float* conv_w[7];
  const float* conv_b[7];
  const float* conv_ln_g[7];
  const float* conv_ln_b[7];
  const float *proj_ln_g, *proj_ln_b, *proj_w, *proj_b;
  const float *pos_w, *pos_b;
  const float *enc_ln_g, *enc_ln_b, *head_w, *head_b;
  const float* ln1_g[48];
  const float* ln1_b[48];
  const float* qkv_w[48];
  const float* qkv_b[48];
  const float* out_w[48];
  const float* out_b[48];
  const float* ln2_g[48];
  const float* ln2_b[48];
  const float* ff1_w[48];
  const float* ff1_b[48];
  const float* ff2_w[48];
  const float* ff2_b[48];
} instag_wav2vec_weights;
size_t instag_wav2vec_workspace_bytes(const instag_wav2vec_weights* w, int32_t batch, int32_t n_samples);
size_t instag_wav2vec_taps_floats(const instag_wav2vec_weights* w, int32_t batch, int32_t n_samples);
int instag_wav2vec_forward(const instag_wav2vec_weights* w, const float* segments, int32_t batch, int32_t n_samples,
                           float* logits, void* workspace, size_t workspace_bytes, int32_t tile, float* taps,
                           instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
