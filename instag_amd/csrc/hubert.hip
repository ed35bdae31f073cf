// HuBERT encoder of the 'hubert' audio features (include/instag_hubert.h), fp32, forward only: the network of
// wav2vec_net.hpp on input values taken as given, ending in the encoder's LayerNorm, with clips of up to 1024 rows.
// Its attention is the streaming softmax of flash_attention.hpp, which the Sapiens backbone shares, under this file's
// bound on the rows.
#include "wav2vec_net.hpp"
#include "flash_attention.hpp"
#include "instag_hubert.h"

namespace instag {
namespace {

constexpr int MAX_T = INSTAG_HUBERT_MAX_FRAMES;

constexpr Net NET = {"hubert", ": batch in [1, 4096], 400 <= n_samples <= 2^20 and at most INSTAG_HUBERT_MAX_FRAMES frames",
                     MAX_T, false};

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_hubert_workspace_bytes(const instag_wav2vec_weights* w, int32_t batch, int32_t n_samples) {
  Plan p;
  return entry_plan(NET, "workspace_bytes", true, w, batch, n_samples, &p) ? p.total * sizeof(float) : 0;
}

size_t instag_hubert_taps_floats(const instag_wav2vec_weights* w, int32_t batch, int32_t n_samples) {
  Plan p;
  return entry_plan(NET, "taps_floats", false, w, batch, n_samples, &p) ? taps_floats(w, batch, p) : 0;
}

int instag_hubert_forward(const instag_wav2vec_weights* w, const float* input_values, int32_t batch, int32_t n_samples,
                          float* hidden, void* workspace, size_t workspace_bytes, int32_t tile, float* taps,
                          instag_stream_t stream) {
  Plan p;
  INSTAG_TRY(forward_prologue(NET, w, input_values, hidden, batch, n_samples, workspace, workspace_bytes, tile, &p));
  return run_network(w, p, input_values, nullptr, batch, (float*)workspace, tile, taps, hidden, (hipStream_t)stream, flash_attention);
}

int instag_hubert_attention(const float* qkv, float* ctx, int32_t batch, int32_t frames, int32_t heads,
                            instag_stream_t stream) {
  INSTAG_REQUIRE(qkv && ctx, "hubert_attention: NULL tensor");
  INSTAG_REQUIRE(((uintptr_t)qkv | (uintptr_t)ctx) % 16 == 0, "hubert_attention: qkv and ctx are 16-byte aligned");
  INSTAG_REQUIRE(batch >= 1 && batch <= 4096 && heads >= 1 && heads <= 65535,
                 "hubert_attention: batch in [1, 4096], heads in [1, 65535]");
  INSTAG_REQUIRE(frames >= 1 && frames <= MAX_T, "hubert_attention: frames in [1, INSTAG_HUBERT_MAX_FRAMES]");
  return flash_attention(qkv, ctx, batch, frames, heads * HEAD_DIM, (hipStream_t)stream);
}

}  // extern "C"
