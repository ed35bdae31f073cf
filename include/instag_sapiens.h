/* C ABI of the Sapiens normal / depth network (csrc/sapiens.hip), the geometry priors of an identity.  Part of
 * libinstag_hip.so; written in the C subset of instag_hip.h and read by the same reader (instag_amd/_cabi.py), so the
 * ctypes side is derived from this text.  The error codes, instag_stream_t and instag_last_error are instag_hip.h's.
 */
#ifndef INSTAG_SAPIENS_H
#define INSTAG_SAPIENS_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSTAG_SAPIENS_MAX_TOKENS 4096
#define INSTAG_SAPIENS_MAX_LAYERS 48
#define INSTAG_SAPIENS_MAX_HEAD 8
#define INSTAG_SAPIENS_MAX_WIDTH 4096

/* ------------------------------------------------------------------------------------------
 * A plain ViT backbone with a dense decode head, fp32, forward only: uint8 frames [B,H,W,3] (RGB) ->
 * out [B,C,H,W], C = 3 (normal) or 1 (depth).
 *
 *  Front end: each frame is resized to in_h x in_w on the 8-bit image (half-pixel centres, clamped indices,
 *  per-axis weights rounded to 1/2048, the exact integer sum rounded half up), normalised per channel as
 *  (x - mean) / std, padded with two zeros in front (Conv2d's padding of 2) and cut into 16 x 16 patches:
 *  grid_h = (in_h - 12) / 16 + 1 rows of grid_w = (in_w - 12) / 16 + 1 patches, T = grid_h grid_w tokens.
 *  instag_sapiens_patch_rows writes these as rows [B T][768], k = channel * 256 + ky * 16 + kx.
 *  Backbone: h = rows W_patch + b + pos_embed; `layers` pre-LayerNorm blocks (eps 1e-6, q|k|v as one
 *  product, heads of 64, erf-GELU); LayerNorm -> features [B,T,hidden], which is the map [B,grid_h,grid_w,hidden].
 *  Head, NHWC: n_deconv x [ConvTranspose2d(kernel 4, stride 2, padding 1, no bias), InstanceNorm (biased
 *  variance, eps 1e-5, per frame and channel), SiLU]; n_conv x [1 x 1 convolution with bias, InstanceNorm, SiLU];
 *  a 1 x 1 convolution to C channels -> raw [B,h,w,4], h = grid_h 2^n_deconv (channels C..3 are padding).
 *  Finish: bilinear to H x W (align_corners = false, no antialiasing); C = 3: n / (|n| + 1e-5) per pixel.
 *
 *  Every matrix is stored [K][N], N contiguous: patch_w [768][hidden]; qkv_w[l] [hidden][3 hidden] (q | k | v),
 *  out_w[l] [hidden][hidden], ff1_w[l] [hidden][intermediate], ff2_w[l] [intermediate][hidden];
 *  deconv_w[j] [py][px][v][(u, cin)][cout] = W[cin][cout][3 - py - 2 v][3 - px - 2 u], the four output phases
 *  (py, px) each as two vertical taps v of one horizontal tap pair u; conv_w[j] [cin][cout]; seg_w [cin][4] and
 *  seg_b [4] with zero columns behind C.  deconv_g/deconv_b and conv_g/conv_beta are the InstanceNorm's gain and
 *  shift, NULL for a norm without them.  zeros: at least INSTAG_SAPIENS_MAX_WIDTH zero floats.
 *  Shapes: hidden / heads == 64, hidden <= 1024, intermediate a multiple of 32, 1 <= layers <=
 *  INSTAG_SAPIENS_MAX_LAYERS, T <= INSTAG_SAPIENS_MAX_TOKENS, 1 <= n_deconv and 0 <= n_conv <=
 *  INSTAG_SAPIENS_MAX_HEAD, widths multiples of 32 up to INSTAG_SAPIENS_MAX_WIDTH, out_channels 1 or 3,
 *  1 <= H, W <= 16384, batch >= 1 and batch h w < 2^31.  Anything else: INSTAG_E_ARG before any device work
 *  (workspace_bytes, taps_floats: 0); INSTAG_E_SPACE for a short workspace.
 *
 *  forward: mode 0 runs the whole chain; 1 the front end and the backbone alone (features is written, out and
 *    raw are not touched); 2 the head and the finish alone (features is read).  In mode 0 features and raw may be
 *    NULL; raw, where given, receives [B,h,w,4].
 *  tile: 0, or 1 / 2 / 3 to run every GEMM on the 64 x 64 / 64 x 128 / 128 x 128 tile (tests).
 *  taps: NULL, or room for instag_sapiens_taps_floats floats (mode 0) that receive a copy of every stage, one
 *    behind the other: the embedded tokens, per layer h behind the attention and behind the feed-forward and
 *    the features, each [B,T,hidden]; every deconv and conv stage behind its SiLU [B,h_j,w_j,C_j]; raw [B,h,w,4].
 *  The transposed convolution runs as its four output phases over a zero-bordered copy of its input; the products
 *  are the fp32 MFMA GEMM of the other networks.  The InstanceNorm sums in fp64 over chunks of 1024 pixels and
 *  then over the chunks in order.  No atomics, every sum in a fixed order: a frame's bits depend on neither its
 *  batch, its chunk nor the tile, and repeated runs give the same bits.
 * ------------------------------------------------------------------------------------------ */
typedef struct instag_sapiens_weights {
  int32_t hidden, heads, intermediate, layers, in_h, in_w, n_deconv, n_conv, out_channels;
  int32_t deconv_c[8];
  int32_t conv_c[8];
  float mean[3];
  float std[3];
  const float *patch_w, *patch_b, *pos_embed, *enc_ln_g, *enc_ln_b, *seg_w, *seg_b, *zeros;
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
  const float* deconv_w[8];
  const float* deconv_g[8];
  const float* deconv_b[8];
  const float* conv_w[8];
  const float* conv_bias[8];
  const float* conv_g[8];
  const float* conv_beta[8];
} instag_sapiens_weights;
size_t instag_sapiens_workspace_bytes(const instag_sapiens_weights* w, int32_t batch);
size_t instag_sapiens_taps_floats(const instag_sapiens_weights* w, int32_t batch);
int instag_sapiens_forward(const instag_sapiens_weights* w, const uint8_t* frames, int32_t batch, int32_t H, int32_t W,
                           int32_t mode, float* out, float* raw, float* features, void* workspace,
                           size_t workspace_bytes, int32_t tile, float* taps, instag_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The stages, each alone (tests).
 *  patch_rows: frames uint8 [B,H,W,3] -> rows [B T][768] as above; mean and std: 3 floats each on the host.
 *  attention: instag_hubert_attention's kernel with 1 <= frames <= INSTAG_SAPIENS_MAX_TOKENS.
 *  deconv: x [B,h,w,cin] -> y [B,2h,2w,cout] with packed weights as deconv_w above; the workspace holds the
 *    zero-bordered copy of x and cout zeros (instag_sapiens_deconv_workspace_bytes).
 *  instance_norm_silu: x [B,h,w,C] in place, gamma and beta both NULL or both given; the workspace holds the
 *    fp64 partial sums (instag_sapiens_norm_workspace_bytes).
 *  finish: raw [B,h,w,4] -> out [B,channels,H,W], channels 1 or 3.
 * ------------------------------------------------------------------------------------------ */
int instag_sapiens_patch_rows(const uint8_t* frames, int32_t batch, int32_t H, int32_t W, int32_t in_h, int32_t in_w,
                              const float* mean, const float* std, float* rows, instag_stream_t stream);
int instag_sapiens_attention(const float* qkv, float* ctx, int32_t batch, int32_t frames, int32_t heads,
                             instag_stream_t stream);
size_t instag_sapiens_deconv_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout);
int instag_sapiens_deconv(const float* x, const float* weight, float* y, int32_t batch, int32_t h, int32_t w,
                          int32_t cin, int32_t cout, void* workspace, size_t workspace_bytes, int32_t tile,
                          instag_stream_t stream);
size_t instag_sapiens_norm_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t channels);
int instag_sapiens_instance_norm_silu(float* x, int32_t batch, int32_t h, int32_t w, int32_t channels,
                                      const float* gamma, const float* beta, void* workspace, size_t workspace_bytes,
                                      instag_stream_t stream);
int instag_sapiens_finish(const float* raw, int32_t batch, int32_t h, int32_t w, int32_t channels, int32_t H, int32_t W,
                          float* out, instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
