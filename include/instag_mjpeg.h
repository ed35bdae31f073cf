/* C ABI of the baseline JPEG encoder (csrc/mjpeg.hip): uint8 frames to JFIF files on the device, what a Motion-JPEG
 * video is made of.  Part of libinstag_hip.so; written in the C subset of instag_hip.h and read by the same reader
 * (instag_amd/_cabi.py), so the ctypes side is derived from this text.  The error codes, instag_stream_t and
 * instag_last_error are instag_hip.h's.
 */
#ifndef INSTAG_MJPEG_H
#define INSTAG_MJPEG_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSTAG_MJPEG_MAX_SIDE 4096
#define INSTAG_MJPEG_MAX_BATCH 64
#define INSTAG_MJPEG_BLOCK_BITS 1660
#define INSTAG_MJPEG_SCAN_BLOCKS 1024
#define INSTAG_MJPEG_SCAN_BYTES 262144

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG (ITU T.81: 8 bit, Huffman, the Annex K tables scaled by the IJG quality rule), integers only;
 * instag_amd/mjpeg.py states every stage and this project's rules (colour transform, edge replication, chroma mean,
 * integer DCT), and the device agrees with it to the bit.
 *
 * frames uint8 [B, H, W, 3] RGB.  sub: 1 for 4:4:4 (MCU 8 x 8, blocks Y Cb Cr), 2 for 4:2:0 (MCU 16 x 16, blocks
 * Y00 Y01 Y10 Y11 Cb Cr); nblk = MCUs x (3 or 6).
 *
 * instag_mjpeg_coefficients: -> coef int16 [B, nblk, 64], the quantised coefficients in zig-zag order, the blocks in
 *   scan order.  Stage one alone, for the tests.
 * instag_mjpeg_encode: -> out uint8 [B, capacity]: frame b's file is out[b][0 .. length[b]): the caller's header
 *   (device pointer, header_bytes of it: SOI .. SOS), the entropy-coded scan, EOI.  length int32 [B]; overflow uint8 [B]
 *   is 1 where the file does not fit capacity: its length is then the size it needs, what was written of its row is
 *   not a file, nothing is written past the row, and the other frames are not affected.
 *   The scan is built without atomics on shared totals: one wave per block turns the 64-bit ballot of the nonzero
 *   coefficients into symbols and bit counts; one workgroup per frame scans the block lengths INSTAG_MJPEG_SCAN_BLOCKS
 *   at a time with a carried total; every lane ORs its bits into a zeroed word stream at its absolute offset (OR does
 *   not depend on the order); the 0xFF bytes are counted per 1024 bytes, scanned per frame INSTAG_MJPEG_SCAN_BYTES at a
 *   time, and the bytes scattered with their 0x00.
 *
 * 1 <= H, W <= INSTAG_MJPEG_MAX_SIDE, 1 <= B <= INSTAG_MJPEG_MAX_BATCH, quality in 1..100, sub 1 or 2, 1 <=
 * header_bytes <= 4096, 1 <= capacity.  Bad arguments: INSTAG_E_ARG before any device work (workspace_bytes: 0);
 * INSTAG_E_SPACE for a short workspace.  No host synchronisation, nothing but kernel launches on `stream`: capturable.
 * ------------------------------------------------------------------------------------------ */
size_t instag_mjpeg_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t sub);
int instag_mjpeg_coefficients(const uint8_t* frames, int32_t B, int32_t H, int32_t W, int32_t quality, int32_t sub,
                              int16_t* coef, instag_stream_t stream);
int instag_mjpeg_encode(const uint8_t* frames, int32_t B, int32_t H, int32_t W, int32_t quality, int32_t sub,
                        const uint8_t* header, int32_t header_bytes, uint8_t* out, int32_t capacity, int32_t* length,
                        uint8_t* overflow, void* workspace, size_t workspace_bytes, instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
