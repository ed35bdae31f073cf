// The 8-bit frame store (gfx950): a processed identity's frames kept compact in HBM, expanded once per step.
//
// instag_frame_ingest (load time): the decoded 8-bit files of F frames -> the store layout.  Per frame, each plane on a
// 256-byte boundary: rgb [H*W*3] as decoded, bg [H*W*3] = the reference's per-camera background
// (dataset_readers.py:232-235), mask [H*W] = face | hair << 1 | mouth << 2 (dataset_readers.py:247-249); plus the
// pixel counts of the three masks (train_mouth.py:145 reads the mouth one).
//
// The background is (torso_rgb * a / 255.0 + bc * (1 - a / 255.0)).astype(uint8) AS NUMPY EVALUATES IT: fp64, that
// operation order, every operation rounded once, truncating conversion.  The integer form (t a + b (255 - a)) / 255
// differs from it in 13,608 of the 256^3 (t, a, b) triples and an fp32 evaluation in 31,953, so the operations are
// spelled with the __d*_rn intrinsics (no contraction, no reciprocal) and the file is built with -ffp-contract=off.
//
// instag_frame_unpack (every step): frame idx of a store -> the byte buffer of a packed Frame (train.py Frame.packed),
// ONE launch: image and background u8 / 255.0 as one correctly rounded fp32 division (torch's ByteTensor / 255.0), the
// three masks as bool bytes, the per-frame record, the audio window gathered from the device-resident feature table
// (utils/audio_utils.py:38-73, mode 2) and the fp32 priors.  Nothing outside the listed tensors is written.
//
// Access widths.  A thread owns four pixels: 12 bytes of an interleaved plane = three dwords, four mask bytes = one.
// Every plane of the store starts 256-byte aligned, so the store side is always dword accesses.  The decoded inputs of
// frame f start at f * H*W*3, which is no multiple of 4 in general: they are read as aligned dwords and funnel-shifted
// (load_dwords), byte by byte only where the aligned window would leave the tensor.  The fp32 planes of the packed
// Frame are 16-byte aligned exactly when H*W % 4 == 0 (float4 stores); otherwise a plane is only 4-byte aligned and
// the four values go out one by one, the last group of a plane only as far as the plane reaches.
#include "common.hpp"
#include "device_math.hpp"

namespace instag {
namespace {

constexpr int REC_DWORDS = 48;    // per-frame record: 16 + 16 + 3 + 6 + 4 = 45 dwords, padded
constexpr int REC_USED = 45;

__host__ __device__ inline size_t plane_bytes(size_t n) { return (n + 255) / 256 * 256; }

// ND dwords of bytes from byte offset `off` of a tensor of `total` bytes whose base is 4-byte aligned.  Bytes past the
// end of the tensor read as zero.
template <int ND>
__device__ __forceinline__ void load_dwords(const uint8_t* __restrict__ base, size_t off, size_t total,
                                            uint32_t (&out)[ND]) {
  const size_t a = off & ~(size_t)3;
  const int sh = (int)(off & 3) * 8;
  if (a + 4 * (ND + 1) <= total) {                 // the aligned window lies inside the tensor
    const uint32_t* p = reinterpret_cast<const uint32_t*>(base + a);
    uint32_t w[ND + 1];
#pragma unroll
    for (int i = 0; i <= ND; ++i) w[i] = p[i];
#pragma unroll
    for (int i = 0; i < ND; ++i) out[i] = sh ? ((w[i] >> sh) | (w[i + 1] << (32 - sh))) : w[i];
  } else {
#pragma unroll
    for (int i = 0; i < ND; ++i) out[i] = 0u;
#pragma unroll
    for (int b = 0; b < 4 * ND; ++b)
      if (off + b < total) out[b >> 2] |= (uint32_t)base[off + b] << ((b & 3) * 8);
  }
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 0xffu; }

// numpy: t * a / 255.0 + b * (1 - a / 255.0), fp64, then .astype(uint8)
__device__ __forceinline__ uint32_t composite(uint32_t t, uint32_t a, uint32_t b) {
  const double da = (double)a;
  const double fg = __ddiv_rn(__dmul_rn((double)t, da), 255.0);
  const double bgw = __dsub_rn(1.0, __ddiv_rn(da, 255.0));
  return (uint32_t)(int)__dadd_rn(fg, __dmul_rn((double)b, bgw)) & 0xffu;
}

struct IngestArgs {
  const uint8_t* gt; const uint8_t* torso; const uint8_t* bc; const uint8_t* parsing; const uint8_t* teeth;
  uint8_t* store; int32_t* counts; int F, H, W;
};

// grid (groups of 4 pixels / 256, F).  counts must be zero on entry.
__global__ void __launch_bounds__(256) frame_ingest_kernel(IngestArgs A) {
  const size_t HW = (size_t)A.H * A.W;
  const size_t groups = (HW + 3) / 4;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  uint32_t packed = 0;                             // three 10-bit pixel counts of this thread
  if (g < groups) {
    const size_t p0 = g * 4;
    const int n = (int)(HW - p0 < 4 ? HW - p0 : 4);
    const size_t P3 = plane_bytes(HW * 3), stride = 2 * P3 + plane_bytes(HW);
    uint32_t rgb[3], tor[4], bcw[3], par[3], tee[1];
    load_dwords<3>(A.gt, ((size_t)f * HW + p0) * 3, (size_t)A.F * HW * 3, rgb);
    load_dwords<4>(A.torso, ((size_t)f * HW + p0) * 4, (size_t)A.F * HW * 4, tor);
    load_dwords<3>(A.bc, p0 * 3, HW * 3, bcw);
    load_dwords<3>(A.parsing, ((size_t)f * HW + p0) * 3, (size_t)A.F * HW * 3, par);
    load_dwords<1>(A.teeth, (size_t)f * HW + p0, (size_t)A.F * HW, tee);
    uint32_t bg[3] = {0u, 0u, 0u}, out_rgb[3] = {0u, 0u, 0u}, mask = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        const uint32_t a = byte_of(tor, 4 * k + 3);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int b = 3 * k + c;
          bg[b >> 2] |= composite(byte_of(tor, 4 * k + c), a, byte_of(bcw, b)) << ((b & 3) * 8);
          out_rgb[b >> 2] |= byte_of(rgb, b) << ((b & 3) * 8);
        }
        const uint32_t R = byte_of(par, 3 * k), G = byte_of(par, 3 * k + 1), B = byte_of(par, 3 * k + 2);
        const uint32_t teeth = byte_of(tee, k) != 0u;
        const uint32_t face = (uint32_t)(B > 254u && R == 0u && G == 0u) ^ teeth;
        const uint32_t hair = (uint32_t)(R < 1u && G < 1u && B < 1u);
        const uint32_t mouth = (uint32_t)(R == 100u && G == 100u && B == 100u) | teeth;
        mask |= (face | hair << 1 | mouth << 2) << (k * 8);
        packed += face | hair << 10 | mouth << 20;
      }
    }
    // the last group of a plane holds n < 4 pixels = 3 n bytes: only the dwords that carry some of them are written
    // (a plane is padded to 256 bytes, so these end inside it; a full 12 bytes could reach into the next plane)
    uint8_t* fr = A.store + (size_t)f * stride;
    uint32_t* d_rgb = reinterpret_cast<uint32_t*>(fr) + g * 3;
    uint32_t* d_bg = reinterpret_cast<uint32_t*>(fr + P3) + g * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (i * 4 < n * 3) { d_rgb[i] = out_rgb[i]; d_bg[i] = bg[i]; }
    reinterpret_cast<uint32_t*>(fr + 2 * P3)[g] = mask;
  }
  // (uniform from here: every lane of the wave takes part in the butterfly; at most 4 * 64 = 256 < 1024 per field)
  packed = wave_sum(packed);
  if ((threadIdx.x & 63) == 0 && packed != 0u) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int c = (int)((packed >> (10 * q)) & 0x3ffu);
      if (c) atomicAdd(A.counts + (size_t)f * 3 + q, c);
    }
  }
}

// ---- unpack -------------------------------------------------------------------------------------------------------------
struct UnpackK {
  const uint8_t* frame;            // the frame's planes in the store
  const uint32_t* record;          // REC_DWORDS of this frame
  const float* normal; const float* depth;   // this frame's priors, or nullptr when the destination has none
  const float* audio;              // [T, row]
  uint8_t* dst;
  long long off_image, off_background, off_face, off_hair, off_mouth, off_record[5], off_auds, off_normal, off_depth;
  int H, W, T, row, audio_index, vec, pixel_blocks;
};

__device__ __forceinline__ float level(uint32_t v) { return __fdiv_rn((float)v, 255.0f); }

// four consecutive values of a plane starting at element p0 (n of them inside the plane)
__device__ __forceinline__ void store4(float* plane, size_t p0, int n, bool vec, float a, float b, float c, float d) {
  if (vec) {
    *reinterpret_cast<float4*>(plane + p0) = make_float4(a, b, c, d);
  } else {
    plane[p0] = a;
    if (n > 1) plane[p0 + 1] = b;
    if (n > 2) plane[p0 + 2] = c;
    if (n > 3) plane[p0 + 3] = d;
  }
}

__device__ __forceinline__ void expand_rgb(const uint8_t* src_plane, size_t g, float* dst, size_t HW, int n, bool vec) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src_plane) + g * 3;
  // (the last group of a plane: only the dwords that carry some of its 3 n bytes)
  const uint32_t w[3] = {s[0], n * 3 > 4 ? s[1] : 0u, n * 3 > 8 ? s[2] : 0u};
#pragma unroll
  for (int c = 0; c < 3; ++c)
    store4(dst + (size_t)c * HW, g * 4, n, vec, level(byte_of(w, c)), level(byte_of(w, 3 + c)),
           level(byte_of(w, 6 + c)), level(byte_of(w, 9 + c)));
}

__device__ __forceinline__ void copy4(const float* src, float* dst, size_t p0, int n, bool vec) {
  if (vec) {
    *reinterpret_cast<float4*>(dst + p0) = *reinterpret_cast<const float4*>(src + p0);
  } else {
    for (int k = 0; k < n; ++k) dst[p0 + k] = src[p0 + k];
  }
}

__device__ __forceinline__ void store_mask(uint8_t* dst, size_t p0, int n, uint32_t m, int bit) {
  const uint32_t v = (m >> bit) & 0x01010101u;
  if (n == 4) {
    *reinterpret_cast<uint32_t*>(dst + p0) = v;    // p0 % 4 == 0 and the tensor starts 256-byte aligned
  } else {
    for (int k = 0; k < n; ++k) dst[p0 + k] = (uint8_t)((v >> (8 * k)) & 1u);
  }
}

// blocks [0, pixel_blocks): four pixels per thread; the blocks behind them: the record and the audio window
__global__ void __launch_bounds__(256) frame_unpack_kernel(UnpackK A) {
  const size_t HW = (size_t)A.H * A.W;
  if ((int)blockIdx.x < A.pixel_blocks) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (HW + 3) / 4) return;
    const size_t p0 = g * 4;
    const int n = (int)(HW - p0 < 4 ? HW - p0 : 4);
    const bool vec = A.vec != 0;
    const size_t P3 = plane_bytes(HW * 3);
    expand_rgb(A.frame, g, reinterpret_cast<float*>(A.dst + A.off_image), HW, n, vec);
    if (A.off_background >= 0)
      expand_rgb(A.frame + P3, g, reinterpret_cast<float*>(A.dst + A.off_background), HW, n, vec);
    const uint32_t m = reinterpret_cast<const uint32_t*>(A.frame + 2 * P3)[g];
    store_mask(A.dst + A.off_face, p0, n, m, 0);
    store_mask(A.dst + A.off_hair, p0, n, m, 1);
    store_mask(A.dst + A.off_mouth, p0, n, m, 2);
    if (A.normal != nullptr) {
      float* dn = reinterpret_cast<float*>(A.dst + A.off_normal);
#pragma unroll
      for (int c = 0; c < 3; ++c) copy4(A.normal + (size_t)c * HW, dn + (size_t)c * HW, p0, n, vec);
      copy4(A.depth, reinterpret_cast<float*>(A.dst + A.off_depth), p0, n, vec);
    }
    return;
  }
  const int t = ((int)blockIdx.x - A.pixel_blocks) * 256 + threadIdx.x;
  if (t < REC_USED) {
    // world_view_transform 0..15, full_proj_transform 16..31, camera_center 32..34, au_exp 35..40, lips_rect 41..44
    const int seg = t < 16 ? 0 : t < 32 ? 1 : t < 35 ? 2 : t < 41 ? 3 : 4;
    const int first = seg == 0 ? 0 : seg == 1 ? 16 : seg == 2 ? 32 : seg == 3 ? 35 : 41;
    reinterpret_cast<uint32_t*>(A.dst + A.off_record[seg])[t - first] = A.record[t];
  } else if (t >= REC_DWORDS && t < REC_DWORDS + 8 * A.row) {
    const int e = t - REC_DWORDS;
    const int r = e / A.row, j = e - r * A.row;
    const int src = A.audio_index - 4 + r;         // rows index - 4 .. index + 3, zero outside the table
    reinterpret_cast<float*>(A.dst + A.off_auds)[e] =
        (src >= 0 && src < A.T) ? A.audio[(size_t)src * A.row + j] : 0.0f;
  }
}

inline bool fits(int64_t off, int64_t bytes, int64_t total) {
  return off >= 0 && (off & 3) == 0 && bytes >= 0 && off <= total - bytes;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

int64_t instag_frame_store_stride(int32_t H, int32_t W) {
  if (H < 1 || W < 1) return 0;
  const size_t HW = (size_t)H * W;
  return (int64_t)(2 * plane_bytes(HW * 3) + plane_bytes(HW));
}

int32_t instag_frame_record_dwords(void) { return REC_DWORDS; }

int instag_frame_ingest(const uint8_t* gt, const uint8_t* torso, const uint8_t* bc, const uint8_t* parsing,
                        const uint8_t* teeth, int32_t F, int32_t H, int32_t W, uint8_t* store, int32_t* counts,
                        instag_stream_t stream) {
  INSTAG_REQUIRE(gt && torso && bc && parsing && teeth && store && counts, "frame_ingest: NULL tensor");
  INSTAG_REQUIRE(H >= 1 && W >= 1, "frame_ingest: bad image size");
  INSTAG_REQUIRE(F >= 1 && F <= 65535, "frame_ingest: 1 .. 65535 frames per call");
  const size_t groups = ((size_t)H * W + 3) / 4;
  INSTAG_REQUIRE(div_up(groups, (size_t)256) <= 0x7fffffffull, "frame_ingest: image too large");
  INSTAG_REQUIRE((((uintptr_t)gt | (uintptr_t)torso | (uintptr_t)bc | (uintptr_t)parsing | (uintptr_t)teeth |
                   (uintptr_t)counts) & 3) == 0 && ((uintptr_t)store & 255) == 0,
                 "frame_ingest: inputs must be 4-byte aligned, the store 256-byte aligned");
  INSTAG_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)F * 3 * sizeof(int32_t), (hipStream_t)stream));
  const IngestArgs a{gt, torso, bc, parsing, teeth, store, counts, F, H, W};
  frame_ingest_kernel<<<dim3((unsigned)div_up(groups, (size_t)256), F), 256, 0, (hipStream_t)stream>>>(a);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_frame_unpack(const instag_frame_unpack_args* u, instag_stream_t stream) {
  INSTAG_REQUIRE(u != nullptr, "frame_unpack: NULL arguments");
  INSTAG_REQUIRE(u->store && u->records && u->audio && u->dst, "frame_unpack: NULL tensor");
  INSTAG_REQUIRE(u->H >= 1 && u->W >= 1, "frame_unpack: bad image size");
  INSTAG_REQUIRE(u->F >= 1 && u->idx >= 0 && u->idx < u->F, "frame_unpack: idx outside [0, F)");
  INSTAG_REQUIRE(u->T >= 1 && u->audio_row >= 1 && u->audio_row <= (1 << 20), "frame_unpack: bad audio table");
  // (index == T is a window the reference accepts, dataset_readers.py:253-256: four rows, then four zero rows)
  INSTAG_REQUIRE(u->audio_index >= 0 && u->audio_index <= u->T, "frame_unpack: audio index outside [0, T]");
  const int64_t HW = (int64_t)u->H * u->W, total = u->dst_bytes;
  const size_t groups = ((size_t)HW + 3) / 4;
  INSTAG_REQUIRE(div_up(groups, (size_t)256) <= 0x7ffffffull, "frame_unpack: image too large");
  const bool want_priors = u->off_normal >= 0 || u->off_depth >= 0;
  INSTAG_REQUIRE(!want_priors || (u->off_normal >= 0 && u->off_depth >= 0 && u->normal && u->depth),
                 "frame_unpack: layout asks for priors the store does not hold");
  const bool ok = fits(u->off_image, HW * 12, total) && (u->off_background < 0 || fits(u->off_background, HW * 12, total)) &&
                  fits(u->off_face, HW, total) && fits(u->off_hair, HW, total) && fits(u->off_mouth, HW, total) &&
                  fits(u->off_world_view, 64, total) && fits(u->off_full_proj, 64, total) &&
                  fits(u->off_camera_center, 12, total) && fits(u->off_au_exp, 24, total) &&
                  fits(u->off_lips_rect, 16, total) && fits(u->off_auds, (int64_t)u->audio_row * 32, total) &&
                  (!want_priors || (fits(u->off_normal, HW * 12, total) && fits(u->off_depth, HW * 4, total)));
  INSTAG_REQUIRE(ok, "frame_unpack: layout does not fit the destination buffer");
  INSTAG_REQUIRE(((uintptr_t)u->store & 255) == 0 && (((uintptr_t)u->records | (uintptr_t)u->audio |
                  (uintptr_t)u->normal | (uintptr_t)u->depth | (uintptr_t)u->dst) & 3) == 0,
                 "frame_unpack: misaligned tensor");
  UnpackK k{};
  k.frame = u->store + (size_t)u->idx * (size_t)instag_frame_store_stride(u->H, u->W);
  k.record = reinterpret_cast<const uint32_t*>(u->records) + (size_t)u->idx * REC_DWORDS;
  k.normal = want_priors ? u->normal + (size_t)u->idx * 3 * HW : nullptr;
  k.depth = want_priors ? u->depth + (size_t)u->idx * HW : nullptr;
  k.audio = u->audio;
  k.dst = u->dst;
  k.off_image = u->off_image; k.off_background = u->off_background;
  k.off_face = u->off_face; k.off_hair = u->off_hair; k.off_mouth = u->off_mouth;
  k.off_record[0] = u->off_world_view; k.off_record[1] = u->off_full_proj; k.off_record[2] = u->off_camera_center;
  k.off_record[3] = u->off_au_exp; k.off_record[4] = u->off_lips_rect;
  k.off_auds = u->off_auds; k.off_normal = u->off_normal; k.off_depth = u->off_depth;
  k.H = u->H; k.W = u->W; k.T = u->T; k.row = u->audio_row; k.audio_index = u->audio_index;
  // float4 accesses: every fp32 plane (and the priors of frame idx) on a 16-byte boundary
  bool vec = HW % 4 == 0 && ((uintptr_t)u->dst & 15) == 0 && (u->off_image & 15) == 0 &&
             (u->off_background < 0 || (u->off_background & 15) == 0);
  if (want_priors)
    vec = vec && (u->off_normal & 15) == 0 && (u->off_depth & 15) == 0 &&
          (((uintptr_t)k.normal | (uintptr_t)k.depth) & 15) == 0;
  k.vec = vec ? 1 : 0;
  k.pixel_blocks = (int)div_up(groups, (size_t)256);
  const int extra = div_up(REC_DWORDS + 8 * u->audio_row, 256);
  frame_unpack_kernel<<<k.pixel_blocks + extra, 256, 0, (hipStream_t)stream>>>(k);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
