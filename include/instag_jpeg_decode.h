/* C ABI of the baseline JPEG decoder (csrc/jpeg_decode.hip): the entropy-coded scans of JFIF files to uint8 frames on
 * the device, the other direction of instag_mjpeg.h.  Part of libinstag_hip.so; written in the C subset of instag_hip.h
 * and read by the same reader (instag_amd/_cabi.py), so the ctypes side is derived from this text.  The error codes,
 * instag_stream_t and instag_last_error are instag_hip.h's.
 */
#ifndef INSTAG_JPEG_DECODE_H
#define INSTAG_JPEG_DECODE_H

#include "instag_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSTAG_JPEG_DECODE_MAX_SIDE 4096
#define INSTAG_JPEG_DECODE_MAX_BATCH 64
#define INSTAG_JPEG_DECODE_MAX_CAPACITY 268435456
#define INSTAG_JPEG_DECODE_MIN_SUB_BITS 64
#define INSTAG_JPEG_DECODE_MAX_SUB_BITS 4096
#define INSTAG_JPEG_DECODE_LANES 1024
#define INSTAG_JPEG_DECODE_SCAN_BYTES 262144
#define INSTAG_JPEG_DECODE_TABLE_BYTES 384
#define INSTAG_JPEG_DECODE_STATUS_CODE 1
#define INSTAG_JPEG_DECODE_STATUS_INDEX 2
#define INSTAG_JPEG_DECODE_STATUS_END 3

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG (ITU T.81: SOF0, 8 bit, Huffman, one interleaved scan of three components), integers only;
 * instag_amd/jpeg_decode.py parses the files, states every stage (the rules are libjpeg's defaults: the "islow" inverse
 * DCT, "fancy" h2v2 upsampling, the 16-bit YCbCr -> RGB table rule), and the device agrees with it to the bit.
 *
 * sub: 1 for 4:4:4 (MCU 8 x 8, blocks Y Cb Cr), 2 for 4:2:0 (MCU 16 x 16, blocks Y00 Y01 Y10 Y11 Cb Cr); nblk = MCUs x
 * (3 or 6).
 *
 * scans uint8 [B, capacity]: frame b's entropy-coded bytes (what lies between SOS and EOI, still stuffed) are
 *   scans[b][0 .. scan_bytes[b]); scan_bytes int32 [B] is read on the device and clamped to 0 .. capacity.
 * huffman uint8 [B, 6, INSTAG_JPEG_DECODE_TABLE_BYTES]: per frame the tables DC Y, DC Cb, DC Cr, AC Y, AC Cb, AC Cr, each
 *   int32 limit[16], int32 base[16], uint8 vals[256] derived from the DHT (bits, vals): with `first` the first code of
 *   length l (Annex C) and `k` the number of codes shorter than l, limit[l - 1] = (first + bits[l - 1]) << (16 - l) and
 *   base[l - 1] = k - first.  The code of the next 16 bits v has the smallest length l with v < limit[l - 1], and its
 *   symbol is vals[((v >> (16 - l)) + base[l - 1]) & 255].
 * quant uint16 [B, 3, 64]: per frame and component the quantisation table, row by row (de-zig-zagged).
 * sub_bits: bits per subsequence of the parallel Huffman decode, a multiple of 32 in MIN_SUB_BITS .. MAX_SUB_BITS.  The
 *   result does not depend on it.
 *
 * instag_jpeg_decode_coefficients: -> coef int16 [B, nblk, 64], the quantised coefficients in zig-zag order, the blocks
 *   in scan order, the DC summed per component; status int32 [B]: 0, or why frame b's scan could not be decoded:
 *   STATUS_CODE a code that is in no table, STATUS_INDEX a coefficient index past 63, STATUS_END the bits ended before
 *   the last block: the first one a sequential decoder meets.  Such a frame's coefficients are unspecified, nothing is
 *   written outside its own rows and the other frames are not affected.
 *   unstuff: the 0x00 behind a 0xFF is dropped: counted per 1024 bytes, scanned per frame INSTAG_JPEG_DECODE_SCAN_BYTES
 *   at a time with a carried total, scattered.  decode: one workgroup of INSTAG_JPEG_DECODE_LANES lanes per frame; every
 *   lane decodes a subsequence from a guessed state, the lanes then walk on until their exit states agree with the
 *   stored ones (at most as many rounds as there are subsequences), an exclusive scan of the blocks completed gives
 *   every subsequence its first block, every lane decodes once more and writes; a per-component running sum turns the
 *   DC differences into values.  No waits between workgroups, no atomics on shared totals (the first error of a
 *   damaged frame is a minimum in LDS).
 * instag_jpeg_decode_pixels: coef and quant -> frames uint8 [B, H, W, 3] RGB: dequantise, inverse DCT, upsample,
 *   colour, crop.
 * instag_jpeg_decode: both, the coefficients kept in the workspace.
 *
 * 1 <= H, W <= MAX_SIDE, 1 <= B <= MAX_BATCH, sub 1 or 2, 1 <= capacity <= MAX_CAPACITY.  Bad arguments: INSTAG_E_ARG
 * before any device work (workspace_bytes: 0); INSTAG_E_SPACE for a short workspace (one size serves the three entry
 * points; instag_jpeg_decode_pixels reads neither capacity nor sub_bits and takes the size of capacity 1, sub_bits 64).
 * No host synchronisation, nothing but kernel launches and one memset on `stream`: capturable.
 * ------------------------------------------------------------------------------------------ */
size_t instag_jpeg_decode_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t sub, int32_t capacity, int32_t sub_bits);
int instag_jpeg_decode_coefficients(const uint8_t* scans, int32_t capacity, const int32_t* scan_bytes,
                                    const uint8_t* huffman, int32_t B, int32_t H, int32_t W, int32_t sub,
                                    int32_t sub_bits, int16_t* coef, int32_t* status, void* workspace,
                                    size_t workspace_bytes, instag_stream_t stream);
int instag_jpeg_decode_pixels(const int16_t* coef, const uint16_t* quant, int32_t B, int32_t H, int32_t W, int32_t sub,
                              uint8_t* frames, void* workspace, size_t workspace_bytes, instag_stream_t stream);
int instag_jpeg_decode(const uint8_t* scans, int32_t capacity, const int32_t* scan_bytes, const uint8_t* huffman,
                       const uint16_t* quant, int32_t B, int32_t H, int32_t W, int32_t sub, int32_t sub_bits,
                       uint8_t* frames, int32_t* status, void* workspace, size_t workspace_bytes, instag_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
