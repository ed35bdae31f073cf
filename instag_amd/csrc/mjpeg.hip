// Baseline JPEG encoder (include/instag_mjpeg.h; instag_amd/mjpeg.py is the statement, stage by stage).  Integers only:
// every sum is exact, so the bytes do not depend on the order anything ran in.
//
//   blocks     a workgroup takes a strip of 64 pixels by one MCU row: reads the pixels (clamped to the frame: the edge
//              rule) and converts them once into LDS, takes the 2 x 2 chroma means there, then one wave per 8 x 8
//              block does the two integer 8 x 8 products, quantises and writes the block in zig-zag order
//   bits       one wave per block, lane = zig-zag index: the 64-bit ballot of "coefficient != 0" gives a nonzero lane
//              its zero run (distance to the previous set bit), the lane behind the last one the EOB, lane 0 the DC
//              difference against the predecessor block of its component (index arithmetic, no walk); a wave sum is
//              the block's bit length
//   scan       one workgroup per frame: exclusive scan of the block lengths, SCAN_BLOCKS at a time with a carried
//              total; then zeroes the words the frame's bits will occupy
//   pack       the symbols again (cheaper than storing them), a wave prefix sum for the lane's offset in the block;
//              the lane ORs its at most 59 bits into at most three words at its absolute offset
//   count      0xFF bytes of the packed stream (the last byte filled with ones) per STUFF_BYTES
//   finish     one workgroup per frame: exclusive scan of those counts; header, EOI, length and overflow
//   scatter    every byte to header + index + 0xFF bytes in front of it, a 0x00 behind each 0xFF; nothing at or past
//              `capacity`
#include "block_scan.hpp"
#include "jpeg_common.hpp"

namespace instag {
namespace {

constexpr int SCAN_THREADS = 1024;            // blocks per step of the per-frame scan of bit lengths
constexpr int STUFF_THREADS = 256;            // one 32-bit word of the stream per thread:
constexpr int STUFF_BYTES = 4 * STUFF_THREADS;   // bytes per 0xFF count
constexpr int FINISH_THREADS = 256;           // counts per step of the per-frame scan of 0xFF counts
static_assert(SCAN_THREADS == INSTAG_MJPEG_SCAN_BLOCKS && FINISH_THREADS * STUFF_BYTES == INSTAG_MJPEG_SCAN_BYTES, "");

// ---- ITU T.81 Annex K ------------------------------------------------------------------------------------------------
__device__ const uint8_t d_quant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// round(16384 C), C the orthonormal 8-point DCT-II matrix
__device__ const int16_t d_dct[64] = {
    5793, 5793,  5793,  5793,  5793,  5793,  5793,  5793,  8035, 6811,  4551,  1598,  -1598, -4551, -6811, -8035,
    7568, 3135,  -3135, -7568, -7568, -3135, 3135,  7568,  6811, -1598, -8035, -4551, 4551,  8035,  1598,  -6811,
    5793, -5793, -5793, 5793,  5793,  -5793, -5793, 5793,  4551, -8035, 1598,  6811,  -6811, -1598, 8035,  -4551,
    3135, -7568, 7568,  -3135, -3135, 7568,  -7568, 3135,  1598, -4551, 6811,  -8035, 8035,  -6811, 4551,  -1598};

struct HuffSpec {
  uint8_t dc_bits[2][16];
  uint8_t ac_bits[2][16];
  uint8_t ac_vals[2][162];
};
constexpr HuffSpec HUFF = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}},
    {{0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
      0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
      0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
      0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
      0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}}};

// code | length << 16 by symbol (Annex C), [0] luma, [1] chroma
struct HuffCodes {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};
constexpr HuffCodes make_codes() {
  HuffCodes t{};
  for (int c = 0; c < 2; ++c) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < HUFF.dc_bits[c][len - 1]; ++i) t.dc[c][k++] = code++ | (uint32_t)len << 16;
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < HUFF.ac_bits[c][len - 1]; ++i) t.ac[c][HUFF.ac_vals[c][k++]] = code++ | (uint32_t)len << 16;
      code <<= 1;
    }
  }
  return t;
}
__device__ const HuffCodes d_codes = make_codes();

// ---- geometry and the workspace --------------------------------------------------------------------------------------
struct Geom : JpegGrid {
  uint32_t max_bits;                     // of one frame's scan: nblk * BLOCK_BITS (< 2^30 at 4096 x 4096)
  uint32_t words;                        // of one frame's word stream, three spare for the last lane's span
  uint32_t counts;                       // 0xFF counts of one frame
  size_t coef, offset, total, stream, count, bytes;   // byte offsets of the pieces in the workspace of B frames
};

Geom geometry(int B, int H, int W, int sub) {
  Geom g{jpeg_grid(H, W, sub)};
  g.max_bits = (uint32_t)g.nblk * INSTAG_MJPEG_BLOCK_BITS;
  g.words = div_up(g.max_bits, 32u) + 3;
  g.counts = div_up(div_up(g.max_bits, 8u), (uint32_t)STUFF_BYTES);
  ByteArena a;
  g.coef = a.take((size_t)B * g.nblk * 64 * sizeof(int16_t));
  g.offset = a.take((size_t)B * g.nblk * sizeof(uint32_t));
  g.total = a.take((size_t)B * 4 * sizeof(uint32_t));
  g.stream = a.take((size_t)B * g.words * sizeof(uint32_t));
  g.count = a.take((size_t)B * g.counts * sizeof(uint32_t));
  g.bytes = a.off;
  return g;
}

// ---- blocks ------------------------------------------------------------------------------------------------------------
constexpr int STRIP = 64;                // pixels of a strip; 24 blocks at either subsampling

template <int SUB>
__global__ __launch_bounds__(256) void mjpeg_blocks(const uint8_t* __restrict__ frames, int H, int W, int mx, int nblk,
                                                    int quality, int16_t* __restrict__ coef) {
  constexpr int MCU = 8 * SUB, MPS = STRIP / MCU, PER = SUB * SUB + 2, NB = MPS * PER;
  static_assert(NB % 4 == 0, "every wave walks the same number of blocks");
  __shared__ int16_t s_y[MCU][STRIP], s_cb[MCU][STRIP], s_cr[MCU][STRIP];
  __shared__ int16_t s_c[2][8][STRIP / SUB];
  __shared__ int s_t[4][64];
  __shared__ int16_t s_o[4][64];
  __shared__ int s_q[64];
  const int tid = threadIdx.x, b = blockIdx.z, row0 = blockIdx.y * MCU, col0 = blockIdx.x * STRIP;
  const uint8_t* f = frames + (size_t)b * H * W * 3;
  if (tid < 64) s_q[tid] = d_dct[tid];
  for (int i = tid; i < MCU * STRIP; i += 256) {
    const int r = i / STRIP, c = i % STRIP;
    const int y = min(row0 + r, H - 1), x = min(col0 + c, W - 1);
    const uint8_t* p = f + ((size_t)y * W + x) * 3;
    const int R = p[0], G = p[1], B = p[2];
    s_y[r][c] = (int16_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
    s_cb[r][c] = (int16_t)(((-11059 * R - 21709 * G + 32768 * B + 32767) >> 16) + 128);
    s_cr[r][c] = (int16_t)(((32768 * R - 27439 * G - 5329 * B + 32767) >> 16) + 128);
  }
  __syncthreads();
  for (int i = tid; i < 2 * 8 * (STRIP / SUB); i += 256) {
    const int pl = i / (8 * (STRIP / SUB)), r = i / (STRIP / SUB) % 8, c = i % (STRIP / SUB);
    const int16_t(*src)[STRIP] = pl ? s_cr : s_cb;
    if constexpr (SUB == 1)
      s_c[pl][r][c] = src[r][c];
    else
      s_c[pl][r][c] = (int16_t)((src[2 * r][2 * c] + src[2 * r][2 * c + 1] + src[2 * r + 1][2 * c] +
                                 src[2 * r + 1][2 * c + 1] + 2) >> 2);
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63, i8 = lane >> 3, v8 = lane & 7;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int blk = wave; blk < NB; blk += 4) {
    const int m = blk / PER, j = blk % PER, gm = blockIdx.x * MPS + m;
    const bool live = gm < mx;
    const int comp = mcu_component(j, SUB);
    // rows: T[i][v] = (sum_j X[i][j] Q[v][j] + 512) >> 10
    int acc = 0;
    if (live) {
      const int16_t* x = comp == 0 ? &s_y[(j / SUB) * 8 + i8][m * MCU + (j % SUB) * 8] : &s_c[comp - 1][i8][m * 8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += ((int)x[k] - 128) * s_q[v8 * 8 + k];
    }
    s_t[wave][lane] = (acc + 512) >> 10;
    __syncthreads();
    // columns: U[u][v] = sum_i Q[u][i] T[i][v]   (u = i8)
    int u = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) u += s_q[i8 * 8 + k] * s_t[wave][k * 8 + v8];
    const int q = min(max((d_quant[comp > 0][lane] * scale + 50) / 100, 1), 255);
    const uint32_t mag = ((uint32_t)abs(u) + ((uint32_t)q << 17)) / ((uint32_t)q << 18);
    s_o[wave][lane] = (int16_t)(u < 0 ? -(int)mag : (int)mag);
    __syncthreads();
    if (live) {
      const size_t g = ((size_t)blockIdx.y * mx + gm) * PER + j;
      coef[((size_t)b * nblk + g) * 64 + lane] = s_o[wave][d_zigzag[lane]];
    }
    __syncthreads();
  }
}

// ---- symbols -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int predecessor(int blk, int sub) {
  if (sub == 1) return blk >= 3 ? blk - 3 : -1;
  const int j = blk % 6;
  if (j >= 1 && j <= 3) return blk - 1;
  if (blk < 6) return -1;
  return j == 0 ? blk - 3 : blk - 6;       // Y00 follows the previous MCU's Y11
}

__device__ __forceinline__ int bit_length(int mag) { return 32 - __clz(mag); }     // (__clz(0) is 32)

// what lane `lane` of the wave that owns block `blk` of a frame writes: `n` bits, the low ones of `val`, MSB first
__device__ __forceinline__ void lane_symbol(const int16_t* __restrict__ fc, int blk, int sub, int lane, uint64_t& val,
                                            int& n) {
  const int tab = (sub == 1 ? mcu_component(blk % 3, 1) : mcu_component(blk % 6, 2)) > 0;
  const int v = fc[(size_t)blk * 64 + lane];
  const uint64_t set = __ballot(v != 0) | 1ull;            // bit 0 stands for "in front of the first AC position"
  val = 0, n = 0;
  if (lane == 0) {
    const int p = predecessor(blk, sub);
    const int d = v - (p < 0 ? 0 : (int)fc[(size_t)p * 64]);
    const int size = bit_length(abs(d));
    const uint32_t e = d_codes.dc[tab][size];
    val = (uint64_t)(e & 0xffff) << size | (uint32_t)(d >= 0 ? d : d + (1 << size) - 1);
    n = (int)(e >> 16) + size;
  } else if (v != 0) {
    const int prev = 63 - __clzll((long long)(set & ((1ull << lane) - 1)));
    const int run = lane - 1 - prev, size = bit_length(abs(v));
    const uint32_t zrl = d_codes.ac[tab][0xF0], e = d_codes.ac[tab][(run & 15) << 4 | size];
    for (int i = 0; i < run >> 4; ++i) val = val << (zrl >> 16) | (zrl & 0xffff);
    val = val << (e >> 16) | (e & 0xffff);
    val = val << size | (uint32_t)(v >= 0 ? v : v + (1 << size) - 1);
    n = (run >> 4) * (int)(zrl >> 16) + (int)(e >> 16) + size;
  } else if (lane == 64 - __clzll((long long)set)) {       // right behind the last nonzero (never lane 64)
    const uint32_t e = d_codes.ac[tab][0];
    val = e & 0xffff, n = (int)(e >> 16);
  }
}

// bit length of every block: offset[b][blk]
__global__ __launch_bounds__(256) void mjpeg_bits(const int16_t* __restrict__ coef, int nblk, int sub,
                                                  uint32_t* __restrict__ offset) {
  const int lane = threadIdx.x & 63, blk = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (blk >= nblk) return;                                 // (a whole wave)
  uint64_t val;
  int n;
  lane_symbol(coef + (size_t)b * nblk * 64, blk, sub, lane, val, n);
  const int sum = wave_inclusive_sum(n, lane);
  if (lane == 63) offset[(size_t)b * nblk + blk] = (uint32_t)sum;
}

// lengths -> exclusive bit offsets, in place; total[b] = {bits, bytes before stuffing, -, -}; zero the words in use
__global__ __launch_bounds__(SCAN_THREADS) void mjpeg_scan(uint32_t* __restrict__ offset, int nblk,
                                                           uint32_t* __restrict__ total, uint32_t* __restrict__ stream,
                                                           uint32_t words) {
  __shared__ uint32_t s_wave[SCAN_THREADS / 64];
  const int b = blockIdx.x;
  const uint32_t carry = carried_exclusive<SCAN_THREADS>(offset + (size_t)b * nblk, (uint32_t)nblk, s_wave);
  if (threadIdx.x == 0) {
    total[b * 4 + 0] = carry;
    total[b * 4 + 1] = (carry + 7) >> 3;
  }
  const uint32_t used = min(words, (carry + 31) / 32 + 3);
  uint32_t* s = stream + (size_t)b * words;
  for (uint32_t i = threadIdx.x; i < used; i += SCAN_THREADS) s[i] = 0;
}

__global__ __launch_bounds__(256) void mjpeg_pack(const int16_t* __restrict__ coef, int nblk, int sub,
                                                  const uint32_t* __restrict__ offset, uint32_t* __restrict__ stream,
                                                  uint32_t words) {
  const int lane = threadIdx.x & 63, blk = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (blk >= nblk) return;
  uint64_t val;
  int n;
  lane_symbol(coef + (size_t)b * nblk * 64, blk, sub, lane, val, n);
  const uint32_t at = offset[(size_t)b * nblk + blk] + (uint32_t)(wave_inclusive_sum(n, lane) - n);
  if (n == 0) return;
  // the n bits start at bit `at & 31` (from the MSB) of word `at >> 5` and end inside the third word at the latest
  const uint32_t w = at >> 5;
  const int sh = 96 - (int)(at & 31) - n;                  // left shift inside the 96-bit window, >= 6
  uint32_t w0, w1, w2;
  if (sh >= 64) {
    w0 = (uint32_t)(val << (sh - 64)), w1 = 0, w2 = 0;
  } else {
    const uint64_t lo = val << sh;
    w0 = (uint32_t)(val >> (64 - sh)), w1 = (uint32_t)(lo >> 32), w2 = (uint32_t)lo;
  }
  uint32_t* s = stream + (size_t)b * words;
  if (w + 2 < words) {                                     // (always: `words` has three spare)
    if (w0) atomicOr(s + w, w0);
    if (w1) atomicOr(s + w + 1, w1);
    if (w2) atomicOr(s + w + 2, w2);
  }
}

// ---- stuffing ----------------------------------------------------------------------------------------------------------
// the four bytes of word `wi` of a frame's stream, first byte in the top bits, the last byte of the stream filled with
// ones; `live`: how many of them are bytes of the stream
__device__ __forceinline__ uint32_t stream_word(const uint32_t* __restrict__ s, uint32_t wi, uint32_t bits, uint32_t bytes,
                                                int& live) {
  live = bytes > 4 * wi ? (int)min(4u, bytes - 4 * wi) : 0;
  if (!live) return 0;
  uint32_t w = s[wi];
  if ((bits & 7) && 4 * wi + live == bytes) w |= ((1u << (8 - (bits & 7))) - 1) << (8 * (4 - live));
  return w;
}

__device__ __forceinline__ int count_ff(uint32_t w, int live) {
  int c = 0;
  for (int k = 0; k < live; ++k) c += ((w >> (24 - 8 * k)) & 0xff) == 0xff;
  return c;
}

__global__ __launch_bounds__(STUFF_THREADS) void mjpeg_count(const uint32_t* __restrict__ stream, uint32_t words,
                                                             const uint32_t* __restrict__ total,
                                                             uint32_t* __restrict__ count, uint32_t counts) {
  __shared__ uint32_t s_wave[STUFF_THREADS / 64];
  const int b = blockIdx.y;
  const uint32_t bits = total[b * 4], bytes = total[b * 4 + 1];
  if ((uint64_t)blockIdx.x * STUFF_BYTES >= bytes) return;       // (the whole workgroup)
  const uint32_t wi = blockIdx.x * STUFF_THREADS + threadIdx.x;
  int live;
  const uint32_t w = stream_word(stream + (size_t)b * words, wi, bits, bytes, live);
  uint32_t ex;
  const uint32_t all = block_exclusive<STUFF_THREADS>((uint32_t)count_ff(w, live), s_wave, ex);
  if (threadIdx.x == 0) count[(size_t)b * counts + blockIdx.x] = all;
}

__global__ __launch_bounds__(FINISH_THREADS) void mjpeg_finish(uint32_t* __restrict__ count, uint32_t counts,
                                                               uint32_t* __restrict__ total,
                                                               const uint8_t* __restrict__ header, int header_bytes,
                                                               uint8_t* __restrict__ out, int capacity,
                                                               int32_t* __restrict__ length, uint8_t* __restrict__ overflow) {
  __shared__ uint32_t s_wave[FINISH_THREADS / 64];
  const int b = blockIdx.x;
  const uint32_t bytes = total[b * 4 + 1];
  const uint32_t used = (bytes + STUFF_BYTES - 1) / STUFF_BYTES;         // <= counts
  const uint32_t carry = carried_exclusive<FINISH_THREADS>(count + (size_t)b * counts, used, s_wave);
  uint8_t* row = out + (size_t)b * capacity;
  for (int i = threadIdx.x; i < header_bytes && i < capacity; i += FINISH_THREADS) row[i] = header[i];
  const uint32_t end = (uint32_t)header_bytes + bytes + carry;           // < 2^31: two bytes per bit-stream byte at most
  if (threadIdx.x == 0) {
    if (end < (uint32_t)capacity) row[end] = 0xff;
    if (end + 1 < (uint32_t)capacity) row[end + 1] = 0xd9;
    length[b] = (int32_t)(end + 2);
    overflow[b] = end + 2 > (uint32_t)capacity;
  }
}

__global__ __launch_bounds__(STUFF_THREADS) void mjpeg_scatter(const uint32_t* __restrict__ stream, uint32_t words,
                                                               const uint32_t* __restrict__ total,
                                                               const uint32_t* __restrict__ count, uint32_t counts,
                                                               int header_bytes, uint8_t* __restrict__ out, int capacity) {
  __shared__ uint32_t s_wave[STUFF_THREADS / 64];
  const int b = blockIdx.y;
  const uint32_t bits = total[b * 4], bytes = total[b * 4 + 1];
  if ((uint64_t)blockIdx.x * STUFF_BYTES >= bytes) return;
  const uint32_t wi = blockIdx.x * STUFF_THREADS + threadIdx.x;
  int live;
  const uint32_t w = stream_word(stream + (size_t)b * words, wi, bits, bytes, live);
  uint32_t ex;
  block_exclusive<STUFF_THREADS>((uint32_t)count_ff(w, live), s_wave, ex);
  uint32_t at = (uint32_t)header_bytes + 4 * wi + count[(size_t)b * counts + blockIdx.x] + ex;
  uint8_t* row = out + (size_t)b * capacity;
  for (int k = 0; k < live; ++k) {
    const uint32_t byte = (w >> (24 - 8 * k)) & 0xff;
    if (at < (uint32_t)capacity) row[at] = (uint8_t)byte;
    ++at;
    if (byte == 0xff) {
      if (at < (uint32_t)capacity) row[at] = 0;
      ++at;
    }
  }
}

int launch_blocks(const uint8_t* frames, int B, const Geom& g, int quality, int16_t* coef, hipStream_t stream) {
  const dim3 grid(div_up(g.sub == 1 ? g.mx * 8 : g.mx * 16, STRIP), g.my, B);
  if (g.sub == 1)
    hipLaunchKernelGGL(mjpeg_blocks<1>, grid, dim3(256), 0, stream, frames, g.H, g.W, g.mx, g.nblk, quality, coef);
  else
    hipLaunchKernelGGL(mjpeg_blocks<2>, grid, dim3(256), 0, stream, frames, g.H, g.W, g.mx, g.nblk, quality, coef);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_mjpeg_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t sub) {
  if (!jpeg_shape_ok(B, H, W, sub)) {
    set_error(std::string("mjpeg_workspace_bytes") + JPEG_SHAPE_OK);
    return 0;
  }
  return geometry(B, H, W, sub).bytes;
}

int instag_mjpeg_coefficients(const uint8_t* frames, int32_t B, int32_t H, int32_t W, int32_t quality, int32_t sub,
                              int16_t* coef, instag_stream_t stream) {
  INSTAG_REQUIRE(frames && coef, "mjpeg_coefficients: NULL tensor");
  INSTAG_REQUIRE(jpeg_shape_ok(B, H, W, sub), std::string("mjpeg_coefficients") + JPEG_SHAPE_OK);
  INSTAG_REQUIRE(quality >= 1 && quality <= 100, "mjpeg_coefficients: quality in 1..100");
  return launch_blocks(frames, B, geometry(B, H, W, sub), quality, coef, (hipStream_t)stream);
}

int instag_mjpeg_encode(const uint8_t* frames, int32_t B, int32_t H, int32_t W, int32_t quality, int32_t sub,
                        const uint8_t* header, int32_t header_bytes, uint8_t* out, int32_t capacity, int32_t* length,
                        uint8_t* overflow, void* workspace, size_t workspace_bytes, instag_stream_t stream) {
  INSTAG_REQUIRE(frames && header && out && length && overflow && workspace, "mjpeg_encode: NULL tensor");
  INSTAG_REQUIRE(jpeg_shape_ok(B, H, W, sub), std::string("mjpeg_encode") + JPEG_SHAPE_OK);
  INSTAG_REQUIRE(quality >= 1 && quality <= 100, "mjpeg_encode: quality in 1..100");
  INSTAG_REQUIRE(header_bytes >= 1 && header_bytes <= 4096 && capacity >= 1,
                 "mjpeg_encode: 1 <= header_bytes <= 4096, capacity >= 1");
  const Geom g = geometry(B, H, W, sub);
  if (workspace_bytes < g.bytes) {
    set_error("mjpeg_encode: workspace too small");
    return INSTAG_E_SPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)workspace;
  int16_t* coef = (int16_t*)(base + g.coef);
  uint32_t* offset = (uint32_t*)(base + g.offset);
  uint32_t* total = (uint32_t*)(base + g.total);
  uint32_t* words = (uint32_t*)(base + g.stream);
  uint32_t* count = (uint32_t*)(base + g.count);
  INSTAG_TRY(launch_blocks(frames, B, g, quality, coef, s));
  const dim3 per_block(div_up(g.nblk, 4), B), per_count(g.counts, B);
  hipLaunchKernelGGL(mjpeg_bits, per_block, dim3(256), 0, s, coef, g.nblk, sub, offset);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(mjpeg_scan, dim3(B), dim3(SCAN_THREADS), 0, s, offset, g.nblk, total, words, g.words);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(mjpeg_pack, per_block, dim3(256), 0, s, coef, g.nblk, sub, offset, words, g.words);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(mjpeg_count, per_count, dim3(STUFF_THREADS), 0, s, words, g.words, total, count, g.counts);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(mjpeg_finish, dim3(B), dim3(FINISH_THREADS), 0, s, count, g.counts, total, header, header_bytes, out,
                     capacity, length, overflow);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(mjpeg_scatter, per_count, dim3(STUFF_THREADS), 0, s, words, g.words, total, count, g.counts,
                     header_bytes, out, capacity);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
