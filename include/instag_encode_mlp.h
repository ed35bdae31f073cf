/* C ABI of the tri-plane encode fused into the motion fields' forward MLP kernels (csrc/mlp.hip).  Part of
 * libinstag_hip.so; written in the C subset of instag_hip.h and read by the same reader (instag_amd/_cabi.py), so the
 * ctypes side is derived from this text.  The error codes, instag_stream_t and instag_last_error are instag_hip.h's;
 * additions only, INSTAG_ABI_VERSION is unchanged.
 */
#ifndef INSTAG_ENCODE_MLP_H
#define INSTAG_ENCODE_MLP_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The tri-plane encode of a motion field and the MLPs that read its rows, in ONE launch per field: one workgroup per CU
 * keeps the three tables and the weights in LDS and evaluates a tile's features straight into the first layer's operand
 * registers.  Arguments up to total_params as instag_triplane_forward (enc_x [N,36] is its `out`, written as before: the
 * glue and the first-layer weight gradients read it); the rest as instag_mlp_forward with NL = 2 / instag_mlp2_forward.
 * Results are bit-identical to the two launches they replace.
 * instag_triplane_mlp_supported: heads = 1 -- a 2-layer MLP 36 -> HA -> OA with 25 <= HA <= 32, OA <= 8 (align_net; HB,
 * OB ignored); heads = 2 -- the pair instag_mlp2_supported accepts; L must be 12 and 3 * total_params floats must fit
 * 150 KB of LDS next to the weights (the face fields' 9,464 entries do, the mouth field's 46,600 do not).
 * max_blocks: 0 = one workgroup per CU as needed; otherwise an upper bound on the workgroups (a wave then walks more
 * tiles; the results do not depend on it).
 * ------------------------------------------------------------------------------------------ */
int instag_triplane_mlp_supported(uint32_t L, uint32_t total_params, int32_t heads, int32_t HA, int32_t OA, int32_t HB,
                                  int32_t OB);
int instag_triplane_mlp_forward(const float* xyz, const float* table_xy, const float* table_yz, const float* table_xz,
                                const int32_t* offsets, const float* shift, uint32_t shift_stride, float shift_scale,
                                uint32_t N, uint32_t L, float S, uint32_t H, float bound, uint32_t total_params,
                                const float* w1, const float* w2, float* enc_x, float* y, float* a1, uint32_t* s1,
                                int32_t HA, int32_t OA, uint32_t max_blocks, instag_stream_t stream);
int instag_triplane_mlp2_forward(const float* xyz, const float* table_xy, const float* table_yz, const float* table_xz,
                                 const int32_t* offsets, const float* shift, uint32_t shift_stride, float shift_scale,
                                 uint32_t N, uint32_t L, float S, uint32_t H, float bound, uint32_t total_params,
                                 const float* wa1, const float* wa2, const float* wb1, const float* wb2, float* enc_x,
                                 float* ya, float* yb, float* a1a, float* a1b, uint32_t* s1, int32_t HA, int32_t OA,
                                 int32_t HB, int32_t OB, uint32_t max_blocks, instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
