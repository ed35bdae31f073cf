/* C ABI of the DeepSpeech 0.1.0 network (csrc/deepspeech.hip), the audio features of a 'deepspeech' head.  Part of
 * libinstag_hip.so; written in the C subset of instag_hip.h and read by the same reader (instag_amd/_cabi.py), so the
 * ctypes side is derived from this text.  The error codes, instag_stream_t and instag_last_error are instag_hip.h's.
 */
#ifndef INSTAG_DEEPSPEECH_H
#define INSTAG_DEEPSPEECH_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSTAG_DEEPSPEECH_MAX_CELL 4096
#define INSTAG_DEEPSPEECH_MAX_STEPS 1048576

/* ------------------------------------------------------------------------------------------
 * DeepSpeech 0.1.0, fp32, forward only: x [S, n_in] -> logits [S, n_out] (no softmax), batch 1.
 *
 *   h1 = min(relu(x W1 + b1), clip), h2, h3 likewise; a bidirectional BasicLSTMCell of `cell` units over the whole
 *   sequence from a zero state, z = [x_t, h_{t-1}] kernel + bias split into i, j, f, o:
 *   c_t = c_{t-1} sigmoid(f + forget_bias) + sigmoid(i) tanh(j), h_t = tanh(c_t) sigmoid(o), the backward direction
 *   the same cell over the reversed sequence; h5 = min(relu([fw_t, bw_t] W5 + b5), clip); logits = h5 W6 + b6.
 *
 * Weights, device pointers to fp32, every matrix [K][N] with n contiguous; k1 = n_in rounded up to 32 and
 * n6 = n_out rounded up to 4, the padding zeros:
 *   w1 [k1, hidden], w2, w3 [hidden, hidden], w5 [2 cell, hidden], w6 [hidden, n6], b1 b2 b3 b5 [hidden], b6 [n6];
 *   wx [2, hidden, 4 cell] and bx [2, 4 cell]: per direction the input half of the LSTM kernel and its bias, the
 *   columns gate-major (i | j | f | o, `cell` each);
 *   wh [2, cell, 4, cell]: the recurrent half transposed, wh[dir][unit][gate][k] = kernel[hidden + k][gate cell + unit],
 *   so the four rows a unit needs are 4 cell contiguous floats.  wh is 16-byte aligned.
 * Shape rules: 1 <= n_in <= 4096, hidden a multiple of 32 in [32, 4096], cell a multiple of 256 in
 * [256, INSTAG_DEEPSPEECH_MAX_CELL] (a lane of the step kernel takes 16 bytes of each 256 floats), 1 <= n_out <= 1024,
 * clip > 0, 1 <= steps <= INSTAG_DEEPSPEECH_MAX_STEPS, max_rows >= 1.  Anything else: INSTAG_E_ARG before any device
 * work (workspace_bytes, taps_floats: 0); INSTAG_E_SPACE for a short workspace.
 *
 * The dense layers and both directions' input projections xp[t][dir] = h3[t] wx[dir] + bx[dir] run on the f32 MFMA
 * GEMM in time blocks of at most max_rows steps (forward rows and their mirror image for the backward direction);
 * the recurrence is one launch per step that serves both directions (step s: t = s forward, t = S - 1 - s backward),
 * a wave per unit.  No atomics, a fixed summation order: the bits depend on neither max_rows nor tile, and repeated
 * runs give the same bits.  tile: 0, or 1..3 to pin the GEMM tile.  taps: NULL, or instag_deepspeech_taps_floats
 * floats that receive h1, h2, h3 [S, hidden], the LSTM's output [S, 2 cell] and h5 [S, hidden], in that order.
 *
 * instag_deepspeech_lstm is the recurrence alone: xp [steps, 2, 4 cell] as above (row t serves both directions at
 * time t) -> hseq [steps, 2 cell] (forward | backward); c [2, cell] is set to zero first and holds the last cell
 * states afterwards.  Of the weights it reads cell, forget_bias and wh.
 * ------------------------------------------------------------------------------------------ */
typedef struct instag_deepspeech_weights {
  int32_t n_in, hidden, cell, n_out;
  float clip, forget_bias;
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  const float *wx, *bx, *wh;
  const float *w5, *b5, *w6, *b6;
} instag_deepspeech_weights;

size_t instag_deepspeech_workspace_bytes(const instag_deepspeech_weights* w, int32_t steps, int32_t max_rows);
size_t instag_deepspeech_taps_floats(const instag_deepspeech_weights* w, int32_t steps);
int instag_deepspeech_forward(const instag_deepspeech_weights* w, const float* x, int32_t steps, int32_t max_rows,
                              float* logits, void* workspace, size_t workspace_bytes, int32_t tile, float* taps,
                              instag_stream_t stream);
int instag_deepspeech_lstm(const instag_deepspeech_weights* w, const float* xp, float* hseq, float* c, int32_t steps,
                           instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
