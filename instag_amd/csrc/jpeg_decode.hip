// Baseline JPEG decoder (include/instag_jpeg_decode.h; instag_amd/jpeg_decode.py is the statement, stage by stage).
// Integers only, so the bytes do not depend on the order anything ran in, nor on sub_bits.
//
//   count      the 0x00 bytes behind a 0xFF per STUFF_BYTES of a frame's scan (the byte in front of a chunk is looked at,
//              so a pair split across two chunks is found)
//   scan       one workgroup per frame: exclusive scan of those counts, SCAN_BYTES at a time with a carried total; the
//              frame's bit count
//   scatter    every kept byte to its index less the dropped bytes in front of it: a bit-addressable stream
//   huffman    one workgroup per frame, one lane per subsequence of sub_bits bits (lanes loop):
//              (a) decode from the start of the subsequence as if a Y block began there, store the exit state
//              (b) walk on through the following subsequences until the exit state equals the stored one; a stored
//                  state that changes is followed up in the next round by the lane that changed it, so when a round
//                  changes nothing every stored state follows from the one in front, and the first one is true
//              (c) exclusive scan of the blocks completed per subsequence
//              (d) decode once more from the true states and write the coefficients (DC as a difference)
//              (e) running sum of the DC differences per component
//   idct       eight lanes per block: dequantise, jidctint's "islow" columns then rows, into Y / Cb / Cr planes
//   colour     one lane per pixel: h2v2 "fancy" upsampling at 4:2:0, YCbCr -> RGB, cropped
#include "block_scan.hpp"
#include "jpeg_common.hpp"

namespace instag {
namespace {

constexpr int STUFF_THREADS = 256;               // four bytes of the scan per thread:
constexpr int STUFF_BYTES = 4 * STUFF_THREADS;   // bytes per count of dropped bytes
constexpr int SCAN_THREADS = 256;                // counts per step of the per-frame scan
constexpr int LANES = INSTAG_JPEG_DECODE_LANES;
constexpr int TABLE_BYTES = INSTAG_JPEG_DECODE_TABLE_BYTES;
constexpr uint32_t IDLE = 0xffffffffu;           // k | j << 8 of a lane that walks no further
static_assert(SCAN_THREADS * STUFF_BYTES == INSTAG_JPEG_DECODE_SCAN_BYTES && TABLE_BYTES == 16 * 4 + 16 * 4 + 256, "");

// ---- geometry and the workspace --------------------------------------------------------------------------------------
struct Geom : JpegGrid {
  int Hp, Wp, Hc, Wc;                    // the luma and chroma planes, whole blocks
  uint32_t sstride;                      // bytes of one frame's unstuffed stream: capacity, and room for two words more
  uint32_t counts;                       // counts of dropped bytes of one frame
  uint32_t nsub;                         // subsequences of one frame at the most (states: one more)
  size_t coef, y, c, stream, count, total, state, bytes;   // byte offsets of the pieces in the workspace of B frames
};

bool scan_ok(int capacity, int sub_bits) {
  return capacity >= 1 && capacity <= INSTAG_JPEG_DECODE_MAX_CAPACITY && sub_bits >= INSTAG_JPEG_DECODE_MIN_SUB_BITS &&
         sub_bits <= INSTAG_JPEG_DECODE_MAX_SUB_BITS && sub_bits % 32 == 0;
}
const char* const SCAN_OK = ": 1 <= capacity <= 2^28, sub_bits a multiple of 32 in 64..4096";

Geom geometry(int B, int H, int W, int sub, int capacity, int sub_bits) {
  Geom g{jpeg_grid(H, W, sub)};
  g.Hp = g.my * 8 * sub, g.Wp = g.mx * 8 * sub, g.Hc = g.my * 8, g.Wc = g.mx * 8;
  g.sstride = (uint32_t)align_up((size_t)capacity, 4) + 8;
  g.counts = div_up((uint32_t)capacity, (uint32_t)STUFF_BYTES);
  g.nsub = (uint32_t)div_up((uint64_t)capacity * 8, (uint64_t)sub_bits);
  ByteArena a;
  g.coef = a.take((size_t)B * g.nblk * 64 * sizeof(int16_t));
  g.y = a.take((size_t)B * g.Hp * g.Wp);
  g.c = a.take((size_t)B * 2 * g.Hc * g.Wc);
  g.stream = a.take((size_t)B * g.sstride);
  g.count = a.take((size_t)B * g.counts * sizeof(uint32_t));
  g.total = a.take((size_t)B * 4 * sizeof(uint32_t));
  g.state = a.take((size_t)B * 5 * (g.nsub + 1) * sizeof(uint32_t));
  g.bytes = a.off;
  return g;
}

// ---- unstuff -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t scan_length(const int32_t* __restrict__ scan_bytes, int b, int capacity) {
  return (uint32_t)min(max(scan_bytes[b], 0), capacity);
}

// the four bytes of a thread, and which of them are a 0x00 behind a 0xFF (bit k of the result: byte k is dropped)
__device__ __forceinline__ uint32_t dropped_of(const uint8_t* __restrict__ s, uint32_t i0, uint32_t n, uint8_t (&byte)[4]) {
  uint32_t prev = i0 > 0 && i0 - 1 < n ? s[i0 - 1] : 0, drop = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t v = i0 + k < n ? s[i0 + k] : 1;
    byte[k] = (uint8_t)v;
    if (i0 + k < n && v == 0 && prev == 0xff) drop |= 1u << k;
    prev = v;
  }
  return drop;
}

__global__ __launch_bounds__(STUFF_THREADS) void jpeg_unstuff_count(const uint8_t* __restrict__ scans, int capacity,
                                                                     const int32_t* __restrict__ scan_bytes,
                                                                     uint32_t* __restrict__ count, uint32_t counts) {
  __shared__ uint32_t s_wave[STUFF_THREADS / 64];
  const int b = blockIdx.y;
  const uint32_t n = scan_length(scan_bytes, b, capacity);
  if ((uint64_t)blockIdx.x * STUFF_BYTES >= n) return;            // (the whole workgroup)
  uint8_t byte[4];
  const uint32_t drop = dropped_of(scans + (size_t)b * capacity, 4u * (blockIdx.x * STUFF_THREADS + threadIdx.x), n, byte);
  uint32_t ex;
  const uint32_t all = block_exclusive<STUFF_THREADS>((uint32_t)__popc(drop), s_wave, ex);
  if (threadIdx.x == 0) count[(size_t)b * counts + blockIdx.x] = all;
}

// counts -> exclusive, in place; total[b] = {bits of the unstuffed stream, -, -, -}
__global__ __launch_bounds__(SCAN_THREADS) void jpeg_unstuff_scan(uint32_t* __restrict__ count, uint32_t counts, int capacity,
                                                                  const int32_t* __restrict__ scan_bytes,
                                                                  uint32_t* __restrict__ total) {
  __shared__ uint32_t s_wave[SCAN_THREADS / 64];
  const int b = blockIdx.x;
  const uint32_t n = scan_length(scan_bytes, b, capacity);
  const uint32_t used = min(counts, (n + STUFF_BYTES - 1) / STUFF_BYTES);
  const uint32_t carry = carried_exclusive<SCAN_THREADS>(count + (size_t)b * counts, used, s_wave);
  if (threadIdx.x == 0) total[b * 4] = 8u * (n - min(carry, n));
}

__global__ __launch_bounds__(STUFF_THREADS) void jpeg_unstuff_scatter(const uint8_t* __restrict__ scans, int capacity,
                                                                       const int32_t* __restrict__ scan_bytes,
                                                                       const uint32_t* __restrict__ count, uint32_t counts,
                                                                       uint8_t* __restrict__ stream, uint32_t sstride) {
  __shared__ uint32_t s_wave[STUFF_THREADS / 64];
  const int b = blockIdx.y;
  const uint32_t n = scan_length(scan_bytes, b, capacity);
  if ((uint64_t)blockIdx.x * STUFF_BYTES >= n) return;
  const uint32_t i0 = 4u * (blockIdx.x * STUFF_THREADS + threadIdx.x);
  uint8_t byte[4];
  const uint32_t drop = dropped_of(scans + (size_t)b * capacity, i0, n, byte);
  uint32_t ex;
  block_exclusive<STUFF_THREADS>((uint32_t)__popc(drop), s_wave, ex);
  const uint32_t before = count[(size_t)b * counts + blockIdx.x] + ex;        // <= i0: dropped bytes in front
  uint8_t* out = stream + (size_t)b * sstride;
  uint32_t at = i0 - min(before, i0);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k < n && !(drop >> k & 1)) {
      if (at < sstride) out[at] = byte[k];
      ++at;
    }
}

// ---- huffman -----------------------------------------------------------------------------------------------------------
struct Tables {                          // of one frame: DC Y, Cb, Cr, AC Y, Cb, Cr
  int32_t limit[6][16];
  int32_t base[6][16];
  uint8_t vals[6][256];
};

// where a decoder stands: the bit position, the coefficient index k in 0..63 and the block index j within the MCU
struct State {
  uint32_t p, kj;
};

// the 32 bits from bit p of the stream, MSB first; bits at and past nbits read as 1.  Reads the words p / 32 and
// p / 32 + 1 for p < nbits <= 8 capacity: inside the frame's sstride bytes.
__device__ __forceinline__ uint32_t peek32(const uint32_t* __restrict__ s, uint32_t p, uint32_t nbits) {
  if (p >= nbits) return 0xffffffffu;
  const uint32_t i = p >> 5, sh = p & 31;
  const uint64_t w = (uint64_t)__builtin_bswap32(s[i]) << 32 | __builtin_bswap32(s[i + 1]);
  uint32_t v = (uint32_t)((w << sh) >> 32);
  const uint32_t left = nbits - p;
  if (left < 32) v |= 0xffffffffu >> left;
  return v;
}

// Decodes from `st` while the position is in front of `end` (<= nbits); -> 0 or the status code of the error met.
// `done`: blocks completed.  WRITE: the coefficients go to fc, the block st stands in being block `first`, the walk ends
// at block nblk and at the first error; every store is at (block < nblk) * 64 + (k <= 63).  Without WRITE (the guessed
// states of (a) and (b)) an error is what a decoder that began in the wrong place meets all the time, and it must find
// its way back: a bit pattern that starts no code is skipped bit by bit, a run past coefficient 63 ends its block, a
// position past the end stays at the end.  A decoder in the true state of a valid file meets none of the three.
template <bool WRITE>
__device__ __forceinline__ int decode_span(const uint32_t* __restrict__ s, uint32_t nbits, uint32_t end, const Tables& T,
                                           int sub, State& st, uint32_t& done, int16_t* __restrict__ fc, uint32_t first,
                                           uint32_t nblk) {
  const int per = sub * sub + 2;
  uint32_t p = st.p;
  int k = (int)(st.kj & 255), j = (int)(st.kj >> 8), err = 0;
  done = 0;
  while (p < end) {
    if (WRITE && first + done >= nblk) break;
    const int t = (k == 0 ? 0 : 3) + mcu_component(j, sub);
    const uint32_t v = peek32(s, p, nbits), v16 = v >> 16;
    int l = 0;
#pragma unroll
    for (int i = 15; i >= 0; --i)
      if (v16 < (uint32_t)T.limit[t][i]) l = i + 1;
    if (l == 0) {
      if (!WRITE) {
        ++p;
        continue;
      }
      err = INSTAG_JPEG_DECODE_STATUS_CODE;
      break;
    }
    const int sym = T.vals[t][((int)(v16 >> (16 - l)) + T.base[t][l - 1]) & 255];
    if (WRITE && k == 0 && sym > 15) {
      err = INSTAG_JPEG_DECODE_STATUS_CODE;
      break;
    }
    const int run = k == 0 ? 0 : sym >> 4, size = sym & 15;
    if (k != 0 && size == 0) {
      if (run != 15) {
        k = 64;
      } else {
        k += 16;
        if (k > 64) {
          if (WRITE) {
            err = INSTAG_JPEG_DECODE_STATUS_INDEX;
            break;
          }
          k = 64;
        }
      }
      p += l;
    } else {
      k += run;
      if (k > 63) {
        if (WRITE) {
          err = INSTAG_JPEG_DECODE_STATUS_INDEX;
          break;
        }
        k = 63;
      }
      if (WRITE) {
        const uint32_t bits = size ? (v << l) >> (32 - size) : 0;
        const int val = size == 0 || (bits >> (size - 1)) ? (int)bits : (int)bits - (1 << size) + 1;
        fc[(size_t)(first + done) * 64 + k] = (int16_t)val;
      }
      p += l + size;
      ++k;
    }
    if (p > nbits) {
      if (WRITE) {
        err = INSTAG_JPEG_DECODE_STATUS_END;
        break;
      }
      p = nbits;
    }
    if (k == 64) {
      k = 0, ++done;
      j = j + 1 == per ? 0 : j + 1;
    }
  }
  st.p = p;
  st.kj = (uint32_t)k | (uint32_t)j << 8;
  return err;
}

__global__ __launch_bounds__(LANES) void jpeg_huffman(const uint8_t* __restrict__ stream, uint32_t sstride,
                                                      const uint32_t* __restrict__ total, const uint8_t* __restrict__ huffman,
                                                      int sub, uint32_t sub_bits, uint32_t nblk, uint32_t nsub_max,
                                                      uint32_t* __restrict__ state, int16_t* __restrict__ coef,
                                                      int32_t* __restrict__ status) {
  __shared__ Tables T;
  __shared__ uint32_t s_wave[LANES / 64];
  __shared__ int s_changed[3];
  __shared__ uint32_t s_error;             // the first error in stream order: subsequence << 2 | status code
  const int b = blockIdx.x, tid = threadIdx.x;
  {
    const uint8_t* h = huffman + (size_t)b * 6 * TABLE_BYTES;
    for (int i = tid; i < 6 * TABLE_BYTES; i += LANES) {
      const int t = i / TABLE_BYTES, o = i % TABLE_BYTES;
      if (o < 128) {
        if ((o & 3) == 0) {
          const int32_t w = (int32_t)((uint32_t)h[i] | (uint32_t)h[i + 1] << 8 | (uint32_t)h[i + 2] << 16 | (uint32_t)h[i + 3] << 24);
          if (o < 64) T.limit[t][o >> 2] = w; else T.base[t][(o - 64) >> 2] = w;
        }
      } else {
        T.vals[t][o - 128] = h[i];
      }
    }
  }
  const uint32_t* s = (const uint32_t*)(stream + (size_t)b * sstride);
  const uint32_t nbits = min(total[b * 4], 8u * (sstride - 8));
  const uint32_t nsub = min(nsub_max, max(1u, (nbits + sub_bits - 1) / sub_bits));
  // per subsequence m: the entry state E[m] (E[m + 1] its exit), the blocks it completes, the state of the lane that
  // started at m in (a)
  uint32_t* E_p = state + (size_t)b * 5 * (nsub_max + 1);
  uint32_t* E_kj = E_p + (nsub_max + 1);
  uint32_t* cnt = E_kj + (nsub_max + 1);
  uint32_t* cur_p = cnt + (nsub_max + 1);
  uint32_t* cur_kj = cur_p + (nsub_max + 1);
  int16_t* fc = coef + (size_t)b * nblk * 64;
  if (tid == 0) {
    status[b] = 0;
    E_p[0] = 0, E_kj[0] = 0;
    s_changed[0] = s_changed[1] = s_changed[2] = 0;
    s_error = 0xffffffffu;
  }
  __syncthreads();

  // (a)
  for (uint32_t m = tid; m < nsub; m += LANES) {
    State st{m * sub_bits, 0};
    uint32_t done;
    decode_span<false>(s, nbits, min((m + 1) * sub_bits, nbits), T, sub, st, done, nullptr, 0, 0);
    cur_p[m] = E_p[m + 1] = st.p;
    cur_kj[m] = E_kj[m + 1] = st.kj;
    cnt[m] = done;
  }
  __syncthreads();

  // (b): in round r the lane that started at i decodes subsequence i + r.  It alone reads and writes E[i + r + 1],
  // cnt[i + r] and cur[i] in this round.  At most nsub - 1 rounds: the lane of subsequence 0 has then seen every one.
  for (uint32_t r = 1; r < nsub; ++r) {
    int changed = 0;
    if (tid == 0) s_changed[(r + 1) % 3] = 0;
    for (uint32_t i = tid; i + r < nsub; i += LANES) {
      State st{cur_p[i], cur_kj[i]};
      if (st.kj == IDLE) continue;
      const uint32_t m = i + r;
      uint32_t done;
      decode_span<false>(s, nbits, min((m + 1) * sub_bits, nbits), T, sub, st, done, nullptr, 0, 0);
      cnt[m] = done;
      if (E_p[m + 1] == st.p && E_kj[m + 1] == st.kj) {
        cur_kj[i] = IDLE;
      } else {
        E_p[m + 1] = cur_p[i] = st.p;
        E_kj[m + 1] = cur_kj[i] = st.kj;
        changed = 1;
      }
    }
    if (changed) s_changed[r % 3] = 1;
    __syncthreads();
    if (!s_changed[r % 3]) break;
  }
  __syncthreads();

  // (c)
  carried_exclusive<LANES>(cnt, nsub, s_wave);
  __syncthreads();

  // (d): a lane stops at its first error; the states behind it are those of a decoder that went on, so their lanes
  // write what they find (inside the frame's rows) and may meet errors of their own: the status is that of the first
  // subsequence with one, as a sequential decoder would report it (a minimum in LDS, the same in whatever order)
  for (uint32_t m = tid; m < nsub; m += LANES) {
    State st{E_p[m], E_kj[m]};
    const uint32_t first = cnt[m];
    if (first >= nblk) continue;
    uint32_t done;
    int err = decode_span<true>(s, nbits, min((m + 1) * sub_bits, nbits), T, sub, st, done, fc, first, nblk);
    if (!err && m == nsub - 1 && first + done < nblk) err = INSTAG_JPEG_DECODE_STATUS_END;
    if (err) atomicMin(&s_error, m << 2 | (uint32_t)err);
  }
  __syncthreads();
  if (tid == 0 && s_error != 0xffffffffu) status[b] = (int32_t)(s_error & 3);

  // (e): per component, the sum of the differences of the MCUs in front, LANES MCUs at a time
  const uint32_t ny = (uint32_t)(sub * sub), per = ny + 2, nmcu = nblk / per;
  uint32_t run[3] = {0, 0, 0};
  for (uint32_t base = 0; base < nmcu; base += LANES) {
    const uint32_t u = base + tid;
    int16_t* mc = fc + (size_t)min(u, nmcu - 1) * per * 64;
    uint32_t sum[3] = {0, 0, 0};
    if (u < nmcu) {
      for (uint32_t j = 0; j < ny; ++j) sum[0] += (uint32_t)(int)mc[j * 64];
      sum[1] = (uint32_t)(int)mc[ny * 64], sum[2] = (uint32_t)(int)mc[(ny + 1) * 64];
    }
    uint32_t at[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t ex;
      const uint32_t all = block_exclusive<LANES>(sum[c], s_wave, ex);
      at[c] = run[c] + ex;
      run[c] += all;
    }
    if (u < nmcu) {
      for (uint32_t j = 0; j < ny; ++j) {
        at[0] += (uint32_t)(int)mc[j * 64];
        mc[j * 64] = (int16_t)at[0];
      }
      mc[ny * 64] = (int16_t)(at[1] + sum[1]);
      mc[(ny + 1) * 64] = (int16_t)(at[2] + sum[2]);
    }
  }
}

// ---- pixels ------------------------------------------------------------------------------------------------------------
// one pass of jidctint.c's jpeg_idct_islow over x[0..7], in place: 13 fraction bits, the result descaled by SHIFT
template <int SHIFT>
__device__ __forceinline__ void idct_pass(int (&x)[8]) {
  int z1 = (x[2] + x[6]) * 4433;
  const int tmp2 = z1 - x[6] * 15137, tmp3 = z1 + x[2] * 6270;
  const int tmp0 = (x[0] + x[4]) * 8192, tmp1 = (x[0] - x[4]) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  int t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z5 - z3 * 16069, z4 = z5 - z4 * 3196;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  constexpr int HALF = 1 << (SHIFT - 1);
  x[0] = (tmp10 + t3 + HALF) >> SHIFT, x[7] = (tmp10 - t3 + HALF) >> SHIFT;
  x[1] = (tmp11 + t2 + HALF) >> SHIFT, x[6] = (tmp11 - t2 + HALF) >> SHIFT;
  x[2] = (tmp12 + t1 + HALF) >> SHIFT, x[5] = (tmp12 - t1 + HALF) >> SHIFT;
  x[3] = (tmp13 + t0 + HALF) >> SHIFT, x[4] = (tmp13 - t0 + HALF) >> SHIFT;
}

constexpr int IDCT_BLOCKS = 32;          // blocks of a workgroup of 256: eight lanes each

__global__ __launch_bounds__(256) void jpeg_idct(const int16_t* __restrict__ coef, const uint16_t* __restrict__ quant,
                                                 int nblk, int sub, int mx, int Hp, int Wp, int Hc, int Wc,
                                                 uint8_t* __restrict__ yplane, uint8_t* __restrict__ cplane) {
  __shared__ int s[IDCT_BLOCKS][65];
  const int tid = threadIdx.x, b = blockIdx.y, g0 = blockIdx.x * IDCT_BLOCKS;
  const int per = sub * sub + 2;
  for (int i = tid; i < IDCT_BLOCKS * 64; i += 256) {
    const int blk = i >> 6, k = i & 63, g = g0 + blk, nat = d_zigzag[k];
    int v = 0;
    if (g < nblk) {
      const int comp = mcu_component(g % per, sub);
      v = (int)coef[((size_t)b * nblk + g) * 64 + k] * (int)quant[((size_t)b * 3 + comp) * 64 + nat];
    }
    s[blk][nat] = v;
  }
  __syncthreads();
  const int blk = tid >> 3, c = tid & 7, g = g0 + blk;
  int x[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) x[r] = s[blk][r * 8 + c];
  idct_pass<11>(x);
#pragma unroll
  for (int r = 0; r < 8; ++r) s[blk][r * 8 + c] = x[r];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = s[blk][c * 8 + k];                    // (c is the row now)
  idct_pass<18>(x);
  if (g >= nblk) return;
  const int m = g / per, j = g % per, mrow = m / mx, mcol = m % mx, comp = mcu_component(j, sub);
  uint8_t* out;
  if (comp == 0)
    out = yplane + ((size_t)b * Hp + (mrow * sub + j / sub) * 8 + c) * Wp + (mcol * sub + j % sub) * 8;
  else
    out = cplane + (((size_t)b * 2 + (comp - 1)) * Hc + mrow * 8 + c) * Wc + mcol * 8;
  uint64_t packed = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) packed |= (uint64_t)min(max(x[k] + 128, 0), 255) << (8 * k);
  *(uint64_t*)out = packed;              // (8-aligned: the planes start at multiples of 256, rows and blocks at multiples of 8)
}

__global__ __launch_bounds__(256) void jpeg_colour(const uint8_t* __restrict__ yplane, const uint8_t* __restrict__ cplane,
                                                   int H, int W, int sub, int Hp, int Wp, int Hc, int Wc,
                                                   uint8_t* __restrict__ frames) {
  const int b = blockIdx.y;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (uint32_t)H * W) return;
  const int y = idx / W, x = idx % W;
  const int Y = yplane[((size_t)b * Hp + y) * Wp + x];
  int C[2];
  const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint8_t* p = cplane + ((size_t)b * 2 + i) * Hc * Wc;
    if (sub == 1) {
      C[i] = p[(size_t)y * Wc + x];
    } else if (cw <= 2) {                                                   // libjpeg repeats so narrow a plane
      C[i] = p[(size_t)(y >> 1) * Wc + (x >> 1)];
    } else {
      const int cy = y >> 1, cx = x >> 1;
      const int nr = y & 1 ? min(cy + 1, ch - 1) : max(cy - 1, 0), nc = x & 1 ? min(cx + 1, cw - 1) : max(cx - 1, 0);
      const int t = 3 * p[(size_t)cy * Wc + cx] + p[(size_t)nr * Wc + cx];
      const int tn = 3 * p[(size_t)cy * Wc + nc] + p[(size_t)nr * Wc + nc];
      C[i] = (3 * t + tn + (x & 1 ? 7 : 8)) >> 4;
    }
  }
  const int cb = C[0] - 128, cr = C[1] - 128;
  uint8_t* o = frames + ((size_t)b * H * W + idx) * 3;
  o[0] = (uint8_t)min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
  o[1] = (uint8_t)min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
  o[2] = (uint8_t)min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
}

int launch_coefficients(const uint8_t* scans, int capacity, const int32_t* scan_bytes, const uint8_t* huffman, int B,
                        const Geom& g, int sub_bits, int16_t* coef, int32_t* status, char* base, hipStream_t s) {
  uint8_t* stream = (uint8_t*)(base + g.stream);
  uint32_t* count = (uint32_t*)(base + g.count);
  uint32_t* total = (uint32_t*)(base + g.total);
  uint32_t* state = (uint32_t*)(base + g.state);
  const dim3 per_count(g.counts, B);
  INSTAG_CHECK_HIP(hipMemsetAsync(coef, 0, (size_t)B * g.nblk * 64 * sizeof(int16_t), s));
  hipLaunchKernelGGL(jpeg_unstuff_count, per_count, dim3(STUFF_THREADS), 0, s, scans, capacity, scan_bytes, count, g.counts);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_unstuff_scan, dim3(B), dim3(SCAN_THREADS), 0, s, count, g.counts, capacity, scan_bytes, total);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_unstuff_scatter, per_count, dim3(STUFF_THREADS), 0, s, scans, capacity, scan_bytes, count, g.counts,
                     stream, g.sstride);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_huffman, dim3(B), dim3(LANES), 0, s, stream, g.sstride, total, huffman, g.sub, (uint32_t)sub_bits,
                     (uint32_t)g.nblk, g.nsub, state, coef, status);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int launch_pixels(const int16_t* coef, const uint16_t* quant, int B, const Geom& g, uint8_t* frames, char* base,
                  hipStream_t s) {
  uint8_t* yplane = (uint8_t*)(base + g.y);
  uint8_t* cplane = (uint8_t*)(base + g.c);
  hipLaunchKernelGGL(jpeg_idct, dim3(div_up(g.nblk, IDCT_BLOCKS), B), dim3(256), 0, s, coef, quant, g.nblk, g.sub, g.mx, g.Hp,
                     g.Wp, g.Hc, g.Wc, yplane, cplane);
  INSTAG_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_colour, dim3(div_up(g.H * g.W, 256), B), dim3(256), 0, s, yplane, cplane, g.H, g.W, g.sub, g.Hp,
                     g.Wp, g.Hc, g.Wc, frames);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

size_t instag_jpeg_decode_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t sub, int32_t capacity, int32_t sub_bits) {
  if (!jpeg_shape_ok(B, H, W, sub) || !scan_ok(capacity, sub_bits)) {
    set_error(std::string("jpeg_decode_workspace_bytes") + (jpeg_shape_ok(B, H, W, sub) ? SCAN_OK : JPEG_SHAPE_OK));
    return 0;
  }
  return geometry(B, H, W, sub, capacity, sub_bits).bytes;
}

int instag_jpeg_decode_coefficients(const uint8_t* scans, int32_t capacity, const int32_t* scan_bytes,
                                    const uint8_t* huffman, int32_t B, int32_t H, int32_t W, int32_t sub,
                                    int32_t sub_bits, int16_t* coef, int32_t* status, void* workspace,
                                    size_t workspace_bytes, instag_stream_t stream) {
  INSTAG_REQUIRE(scans && scan_bytes && huffman && coef && status && workspace, "jpeg_decode_coefficients: NULL tensor");
  INSTAG_REQUIRE(jpeg_shape_ok(B, H, W, sub), std::string("jpeg_decode_coefficients") + JPEG_SHAPE_OK);
  INSTAG_REQUIRE(scan_ok(capacity, sub_bits), std::string("jpeg_decode_coefficients") + SCAN_OK);
  const Geom g = geometry(B, H, W, sub, capacity, sub_bits);
  if (workspace_bytes < g.bytes) {
    set_error("jpeg_decode_coefficients: workspace too small");
    return INSTAG_E_SPACE;
  }
  return launch_coefficients(scans, capacity, scan_bytes, huffman, B, g, sub_bits, coef, status, (char*)workspace,
                             (hipStream_t)stream);
}

int instag_jpeg_decode_pixels(const int16_t* coef, const uint16_t* quant, int32_t B, int32_t H, int32_t W, int32_t sub,
                              uint8_t* frames, void* workspace, size_t workspace_bytes, instag_stream_t stream) {
  INSTAG_REQUIRE(coef && quant && frames && workspace, "jpeg_decode_pixels: NULL tensor");
  INSTAG_REQUIRE(jpeg_shape_ok(B, H, W, sub), std::string("jpeg_decode_pixels") + JPEG_SHAPE_OK);
  const Geom g = geometry(B, H, W, sub, 1, INSTAG_JPEG_DECODE_MIN_SUB_BITS);
  if (workspace_bytes < g.bytes) {
    set_error("jpeg_decode_pixels: workspace too small");
    return INSTAG_E_SPACE;
  }
  return launch_pixels(coef, quant, B, g, frames, (char*)workspace, (hipStream_t)stream);
}

int instag_jpeg_decode(const uint8_t* scans, int32_t capacity, const int32_t* scan_bytes, const uint8_t* huffman,
                       const uint16_t* quant, int32_t B, int32_t H, int32_t W, int32_t sub, int32_t sub_bits,
                       uint8_t* frames, int32_t* status, void* workspace, size_t workspace_bytes, instag_stream_t stream) {
  INSTAG_REQUIRE(scans && scan_bytes && huffman && quant && frames && status && workspace, "jpeg_decode: NULL tensor");
  INSTAG_REQUIRE(jpeg_shape_ok(B, H, W, sub), std::string("jpeg_decode") + JPEG_SHAPE_OK);
  INSTAG_REQUIRE(scan_ok(capacity, sub_bits), std::string("jpeg_decode") + SCAN_OK);
  const Geom g = geometry(B, H, W, sub, capacity, sub_bits);
  if (workspace_bytes < g.bytes) {
    set_error("jpeg_decode: workspace too small");
    return INSTAG_E_SPACE;
  }
  char* base = (char*)workspace;
  int16_t* coef = (int16_t*)(base + g.coef);
  INSTAG_TRY(launch_coefficients(scans, capacity, scan_bytes, huffman, B, g, sub_bits, coef, status, base, (hipStream_t)stream));
  return launch_pixels(coef, quant, B, g, frames, base, (hipStream_t)stream);
}

}  // extern "C"
