"""Rendered frames as a video file: a baseline JPEG encoder on the device (csrc/mjpeg.hip), and a Motion-JPEG AVI with
a PCM track around it.  What synthesize_fuse.py:76-90 does with ``imageio.mimwrite`` ends here in an ``.avi`` every
player, ffmpeg and PIL read; h264 is not provided.

The statement is ``jpeg_encode_torch``: integers only, so the device and this file agree to the bit.  Its stages are
public (``planes_torch``, ``coefficients_torch``, ``scan_torch``, ``header_bytes``).  The tables are those of ITU T.81
Annex K, scaled by the IJG quality rule; the colour transform, the edge rule, the chroma mean and the integer DCT are
this project's (``planes_torch``, ``coefficients_torch``): a JPEG decoder does not see which were used.

    JpegEncoder(H, W, device)          uint8 [B,H,W,3] -> JPEG bytes, on the device
    AviWriter(path, H, W)              JPEG bytes (and audio) -> RIFF AVI, on the host
    VideoWriter(path, H, W, device)    both: ``.append(frames_u8)``
    write_video(renderer, frames, path)   synthesize_fuse.py's render_set
    read_avi(path)                     -> frames, fps, audio (PIL decodes, or a jpeg_decode.JpegDecoder)
"""
from __future__ import annotations

import io
import struct
import numpy as np
import torch

from .device_op import DeviceOperator
from .jpeg_common import (MAX_BATCH, MAX_SIDE, MCU_COMPONENTS, SUBSAMPLING, ZIGZAG, block_components, block_count,
                          blocks_from_planes, check_size, code_ranges, mcu_grid, sub_of)

# ---- ITU T.81 Annex K ---------------------------------------------------------------------------------------------------
LUMA_QUANT = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
              14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHROMA_QUANT = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
DC_LUMA_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_CHROMA_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
DC_VALS = tuple(range(12))
AC_LUMA_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D)
AC_LUMA_VALS = tuple(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)
AC_CHROMA_VALS = tuple(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
# round(16384 C), C the orthonormal 8-point DCT-II matrix: C[u][j] = c(u) cos((2 j + 1) u pi / 16)
DCT_Q14 = ((5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793), (8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035),
           (7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568), (6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811),
           (5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793), (4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551),
           (3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135), (1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598))
BLOCK_BITS = 1660                                   # 11 + 11 bits of DC, 63 x (16 + 10) of AC: no block codes longer


def quant_tables(quality: int):
    """-> (luma, chroma), int64 [64] row by row: Annex K scaled by the IJG rule, ``s = 5000 // q`` below 50 and
    ``200 - 2 q`` from there, ``clip((t s + 50) // 100, 1, 255)``."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality in 1..100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(t, np.int64) * s + 50) // 100, 1, 255) for t in (LUMA_QUANT, CHROMA_QUANT))


def huffman_codes(bits, vals):
    """Annex C: symbol -> (code, length) of the table with ``bits[l - 1]`` codes of length l over ``vals``."""
    return {vals[k + i]: (code + i, length) for length, (code, n, k) in enumerate(code_ranges(bits), 1) for i in range(n)}


def _code_arrays(bits, vals):
    code, length = np.zeros(256, np.uint64), np.zeros(256, np.int64)
    for sym, (c, n) in huffman_codes(bits, vals).items():
        code[sym], length[sym] = c, n
    return code, length


_DC = (_code_arrays(DC_LUMA_BITS, DC_VALS), _code_arrays(DC_CHROMA_BITS, DC_VALS))
_AC = (_code_arrays(AC_LUMA_BITS, AC_LUMA_VALS), _code_arrays(AC_CHROMA_BITS, AC_CHROMA_VALS))


# ---- stages -------------------------------------------------------------------------------------------------------------
def _frames(frames_u8):
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3 or frames_u8.shape[0] < 1:
        raise ValueError(f"frames are uint8 [B,H,W,3] with B >= 1, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    check_size(frames_u8.shape[1], frames_u8.shape[2])
    return frames_u8


def planes_torch(frames_u8, subsampling="4:2:0"):
    """-> (Y [B,Hp,Wp], Cb, Cr [B,Hp/s,Wp/s]) int64 in 0..255, Hp and Wp the sides rounded up to the MCU (8 s).

    The rules are this project's, not a library's: ``Y = (19595 R + 38470 G + 7471 B + 32768) >> 16``,
    ``Cb = ((-11059 R - 21709 G + 32768 B + 32767) >> 16) + 128``, ``Cr = ((32768 R - 27439 G - 5329 B + 32767) >> 16)
    + 128`` (the JFIF matrix in 16 fraction bits, the shift an arithmetic one; the half less one keeps 0..255 without a
    clamp); the last row and column are repeated up to the MCU multiple; 4:2:0 chroma is ``(a + b + c + d + 2) >> 2``
    of the 2 x 2 full-resolution Cb / Cr values."""
    s = sub_of(subsampling)
    x = _frames(frames_u8).to(torch.int64)
    B, H, W, _ = x.shape
    Hp, Wp = (8 * s * n for n in mcu_grid(H, W, s))
    rows = torch.arange(Hp, device=x.device).clamp(max=H - 1)
    cols = torch.arange(Wp, device=x.device).clamp(max=W - 1)
    x = x[:, rows][:, :, cols]
    R, G, Bl = x[..., 0], x[..., 1], x[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16
    Cb = ((-11059 * R - 21709 * G + 32768 * Bl + 32767) >> 16) + 128
    Cr = ((32768 * R - 27439 * G - 5329 * Bl + 32767) >> 16) + 128
    if s == 2:
        Cb, Cr = ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + 2) >> 2 for c in (Cb, Cr))
    return Y, Cb, Cr


def coefficients_torch(frames_u8, quality=90, subsampling="4:2:0"):
    """-> int16 [B, nblk, 64]: the quantised DCT coefficients in zig-zag order, the blocks in scan order (per MCU its Y
    blocks row by row, Cb, Cr).

    With X the block minus 128 and Q = ``DCT_Q14``: rows ``T = (X Q^T + 512) >> 10``, columns ``U = Q T`` (the
    orthonormal DCT times 2^18), ``coef = sign(U) ((|U| + (q << 17)) // (q << 18))``: division by the table entry q,
    halves away from zero.  Every intermediate fits 32 bits; integer sums do not depend on their order."""
    X = blocks_from_planes(*planes_torch(frames_u8, subsampling), sub_of(subsampling)) - 128
    Q = torch.tensor(DCT_Q14, dtype=torch.int64, device=X.device)
    T = (X @ Q.t() + 512) >> 10
    U = Q @ T
    luma, chroma = (torch.from_numpy(t).to(X.device).view(8, 8) for t in quant_tables(quality))
    comp = torch.from_numpy(block_components(frames_u8.shape[1], frames_u8.shape[2], subsampling)).to(X.device)
    q = torch.where((comp == 0)[:, None, None], luma, chroma)
    coef = torch.sign(U) * ((U.abs() + (q << 17)) // (q << 18))
    zz = torch.tensor(ZIGZAG, device=X.device)
    return coef.reshape(X.shape[0], -1, 64)[:, :, zz].to(torch.int16)


def _size(mag):
    """Bit length of a non-negative int64 array (0 -> 0)."""
    n = np.zeros(mag.shape, np.int64)
    m = mag.copy()
    while m.any():
        n += m > 0
        m >>= 1
    return n


def scan_torch(coef, subsampling="4:2:0", H=None, W=None):
    """One frame's entropy-coded segment.  ``coef`` int16 [nblk, 64] (``coefficients_torch``) -> (bytes, counters).

    DC: the difference to the previous block of the component, as (size, bits).  AC: per nonzero coefficient the run of
    zeros in front, 16 at a time as ZRL, then (run, size) and the bits; EOB unless position 63 is nonzero.  Annex K
    codes, MSB first, 0xFF followed by 0x00, the last byte filled with ones.  Counters: ``zrl`` symbols, ``stuffed``
    bytes, ``dc_size`` and ``ac_size`` the largest categories, ``bits`` before the fill.  The block-to-component map
    follows from the block count and ``subsampling`` alone (``H``, ``W`` are not needed)."""
    per = MCU_COMPONENTS[sub_of(subsampling)]
    c = np.asarray(coef.cpu() if torch.is_tensor(coef) else coef).astype(np.int64)
    nblk = c.shape[0]
    if c.ndim != 2 or c.shape[1] != 64 or nblk % len(per):
        raise ValueError(f"coef is [nblk, 64] with nblk a multiple of {len(per)}, got {c.shape}")
    comp = np.tile(np.asarray(per), nblk // len(per))
    tab = (comp > 0).astype(np.int64)                                           # Huffman table of the block

    # DC differences
    diff = np.zeros(nblk, np.int64)
    for k in range(3):
        idx = np.nonzero(comp == k)[0]
        dc = c[idx, 0]
        diff[idx] = dc - np.concatenate([[0], dc[:-1]])
    dsize = _size(np.abs(diff))
    dcode = np.stack([_DC[0][0], _DC[1][0]])[tab, dsize]
    dlen = np.stack([_DC[0][1], _DC[1][1]])[tab, dsize]
    dbits = np.where(diff >= 0, diff, diff + (1 << dsize) - 1).astype(np.uint64)
    ev_key = [np.arange(nblk) * 65]
    ev_val = [(dcode << dsize.astype(np.uint64)) | dbits]
    ev_len = [dlen + dsize]

    # AC symbols
    blk, pos = np.nonzero(c[:, 1:])
    pos = pos + 1
    first = np.ones(blk.shape, bool)
    first[1:] = blk[1:] != blk[:-1]
    prev = np.where(first, 0, np.concatenate([[0], pos[:-1]]))
    run = pos - prev - 1
    v = c[blk, pos]
    asize = _size(np.abs(v))
    if asize.size and asize.max() > 10:
        raise ValueError("an AC coefficient beyond 10 bits: not a baseline JPEG block")
    if dsize.max() > 11:
        raise ValueError("a DC difference beyond 11 bits: not a baseline JPEG block")
    acode, alen = np.stack([_AC[0][0], _AC[1][0]]), np.stack([_AC[0][1], _AC[1][1]])
    t = tab[blk]
    sym = ((run & 15) << 4) | asize
    nz = run >> 4
    val = np.zeros(blk.shape, np.uint64)
    n = np.zeros(blk.shape, np.int64)
    for i in range(3):
        on = nz > i
        val = np.where(on, (val << alen[t, 0xF0].astype(np.uint64)) | acode[t, 0xF0], val)
        n = n + on * alen[t, 0xF0]
    val = (val << alen[t, sym].astype(np.uint64)) | acode[t, sym]
    val = (val << asize.astype(np.uint64)) | np.where(v >= 0, v, v + (1 << asize) - 1).astype(np.uint64)
    ev_key.append(blk * 65 + pos)
    ev_val.append(val)
    ev_len.append(n + alen[t, sym] + asize)

    # EOB
    last = np.zeros(nblk, np.int64)
    last[blk] = pos                                                              # (ascending per block: the last one stays)
    e = np.nonzero(last < 63)[0]
    ev_key.append(e * 65 + last[e] + 1)
    ev_val.append(acode[tab[e], 0])
    ev_len.append(alen[tab[e], 0])

    key, val, n = np.concatenate(ev_key), np.concatenate(ev_val).astype(np.uint64), np.concatenate(ev_len)
    order = np.argsort(key, kind="stable")
    val, n = val[order], n[order]
    total = int(n.sum())
    start = np.cumsum(n) - n
    which = np.repeat(np.arange(n.size), n)
    shift = (n[which] - 1 - (np.arange(total) - start[which])).astype(np.uint64)
    bits = ((val[which] >> shift) & np.uint64(1)).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-total % 8, np.uint8)])
    raw = np.packbits(bits)
    ff = np.nonzero(raw == 0xFF)[0]
    out = np.insert(raw, ff + 1, 0)
    counters = dict(zrl=int(nz.sum()), stuffed=int(ff.size), dc_size=int(dsize.max()),
                    ac_size=int(asize.max()) if asize.size else 0, bits=total)
    return out.tobytes(), counters


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def header_bytes(H, W, quality=90, subsampling="4:2:0") -> bytes:
    """SOI, JFIF APP0 (1.01, aspect 1:1), the luma and chroma DQT (zig-zag order), SOF0, the four Annex K DHT, SOS."""
    check_size(H, W)
    s = sub_of(subsampling)
    luma, chroma = quant_tables(quality)
    zz = np.asarray(ZIGZAG)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, b"\x00" + bytes(luma[zz].astype(np.uint8))) + _segment(0xDB, b"\x01" + bytes(chroma[zz].astype(np.uint8)))
    out += _segment(0xC0, struct.pack(">BHHB", 8, int(H), int(W), 3) + bytes([1, s << 4 | s, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def max_bytes(H, W, subsampling="4:2:0") -> int:
    """No frame of this size is longer: the header, ``BLOCK_BITS`` per block with every byte stuffed, EOI."""
    return len(header_bytes(H, W, 90, subsampling)) + 2 * -(-block_count(H, W, subsampling) * BLOCK_BITS // 8) + 2


def jpeg_encode_torch(frames_u8, quality=90, subsampling="4:2:0"):
    """uint8 [B,H,W,3] -> one baseline JFIF file per frame (the statement of ``JpegEncoder``)."""
    B, H, W, _ = _frames(frames_u8).shape
    head = header_bytes(H, W, quality, subsampling)
    coef = coefficients_torch(frames_u8.cpu(), quality, subsampling)
    return [head + scan_torch(coef[b], subsampling)[0] + b"\xff\xd9" for b in range(B)]


# ---- the device path ----------------------------------------------------------------------------------------------------
class _Header:
    """What ``DeviceOperator`` keeps on the device for the encoder: the frame header (its "weights")."""

    def __init__(self, data: bytes):
        self.data = data

    def device_pack(self, device):
        t = torch.frombuffer(bytearray(self.data), dtype=torch.uint8).to(device)
        return None, (t,)


class JpegEncoder(DeviceOperator):
    """Baseline JPEG of uint8 [B,H,W,3] frames of one size, on ``device`` (a CPU device runs the statement).

    ``capacity``: bytes per frame of ``encode``'s output, default ``H W 3 // 2 + len(header)``; ``max_batch``: frames per
    launch (default: as many as keep the workspace near 256 MB, at most 64).  ``encode`` never synchronises; a frame
    that does not fit sets its flag in ``.overflow`` (uint8 [B], of the last ``encode``) and reports the length it
    needs.  ``encode_bytes`` encodes such a chunk again at ``max_bytes``."""

    def __init__(self, H, W, device, quality=90, subsampling="4:2:0", max_batch=None, capacity=None):
        check_size(H, W)
        self.H, self.W, self.quality, self.subsampling = int(H), int(W), int(quality), subsampling
        self.sub = sub_of(subsampling)
        quant_tables(quality)
        self.header = header_bytes(H, W, quality, subsampling)
        self.max_bytes = max_bytes(H, W, subsampling)
        self.nblk = block_count(H, W, subsampling)
        self.capacity = self._at_least_one(capacity, "capacity") or (self.H * self.W * 3 // 2 + len(self.header))
        super().__init__(_Header(self.header), device)
        self.max_batch = self._at_least_one(max_batch)
        self.overflow = None
        if self.device.type == "cuda":
            from . import _lib
            self._header = self._keep[0]
            per = _lib.workspace_bytes(self._L.instag_mjpeg_workspace_bytes(1, self.H, self.W, self.sub))
            if self.max_batch is None:
                self.max_batch = max(1, min(MAX_BATCH, (256 << 20) // per))
            if self.max_batch > MAX_BATCH:
                raise ValueError(f"JpegEncoder: max_batch <= {MAX_BATCH}, got {self.max_batch}")
        elif self.max_batch is None:
            self.max_batch = MAX_BATCH

    def _check(self, frames):
        here = frames.device.type == self.device.type and self.device.index in (None, frames.device.index)
        if tuple(_frames(frames).shape[1:]) != (self.H, self.W, 3) or not here:
            raise ValueError(f"JpegEncoder: frames uint8 [B,{self.H},{self.W},3] on {self.device}, got "
                             f"{tuple(frames.shape)} on {frames.device}")
        return frames.contiguous()

    def coefficients(self, frames):
        """-> int16 [B, nblk, 64] (``coefficients_torch``)."""
        frames = self._check(frames)
        if self.device.type != "cuda":
            return coefficients_torch(frames, self.quality, self.subsampling)
        from . import _lib
        B = frames.shape[0]
        coef = torch.empty(B, self.nblk, 64, dtype=torch.int16, device=self.device)
        self._each_chunk(B, 0, lambda sl, m, p, size: self._L.instag_mjpeg_coefficients(
            _lib.ptr(frames[sl]), m, self.H, self.W, self.quality, self.sub, _lib.ptr(coef[sl]), _lib.current_stream()),
            "mjpeg_coefficients")
        return coef

    def encode(self, frames, capacity=None):
        """-> (data uint8 [B, capacity], length int32 [B]) on the device: frame b is ``data[b, :length[b]]``."""
        frames = self._check(frames)
        B, cap = frames.shape[0], int(capacity or self.capacity)
        if self.device.type != "cuda":
            files = jpeg_encode_torch(frames, self.quality, self.subsampling)
            data = torch.zeros(B, cap, dtype=torch.uint8)
            for b, f in enumerate(files):
                data[b, :min(cap, len(f))] = torch.frombuffer(bytearray(f[:cap]), dtype=torch.uint8)
            length = torch.tensor([len(f) for f in files], dtype=torch.int32)
            self.overflow = (length > cap).to(torch.uint8)
            return data, length
        from . import _lib
        data = torch.empty(B, cap, dtype=torch.uint8, device=self.device)
        length = torch.empty(B, dtype=torch.int32, device=self.device)
        self.overflow = torch.empty(B, dtype=torch.uint8, device=self.device)
        self.encode_into(frames, data, length, self.overflow)
        return data, length

    def encode_into(self, frames, data, length, overflow):
        """``encode`` into the caller's tensors: ``data`` uint8 [B, >= 1] whose row stride may exceed its width (a frame
        writes ``data.shape[1]`` bytes of its row at the most), ``length`` int32 [B], ``overflow`` uint8 [B]."""
        from . import _lib
        frames = self._check(frames)
        B, cap = frames.shape[0], int(data.shape[1])
        if (data.dtype != torch.uint8 or data.shape[0] != B or data.stride(1) != 1 or length.dtype != torch.int32
                or overflow.dtype != torch.uint8 or not length.is_contiguous() or not overflow.is_contiguous()):
            raise ValueError("JpegEncoder: data uint8 [B, capacity] with unit column stride, length int32 [B], overflow uint8 [B]")
        if B > 1 and data.stride(0) != cap:                                     # rows apart: a launch per frame
            for b in range(B):
                self.encode_into(frames[b:b + 1], data[b:b + 1], length[b:b + 1], overflow[b:b + 1])
            return
        nbytes = _lib.workspace_bytes(self._L.instag_mjpeg_workspace_bytes(min(B, self.max_batch), self.H, self.W, self.sub))
        self._each_chunk(B, nbytes, lambda sl, m, p, size: self._L.instag_mjpeg_encode(
            _lib.ptr(frames[sl]), m, self.H, self.W, self.quality, self.sub, _lib.ptr(self._header), len(self.header),
            _lib.ptr(data[sl]), cap, _lib.ptr(length[sl]), _lib.ptr(overflow[sl]), p, size, _lib.current_stream()),
            "mjpeg_encode")

    def encode_bytes(self, frames):
        """-> one JPEG file per frame, as bytes: the lengths, then one copy of the used prefix, to the host."""
        frames = self._check(frames)
        out = []
        for i in range(0, frames.shape[0], self.max_batch):
            chunk = frames[i:i + self.max_batch]
            data, length = self.encode(chunk)
            n, over = length.cpu(), self.overflow.cpu()
            if bool(over.any()):
                data, length = self.encode(chunk, self.max_bytes)
                n = length.cpu()
                assert not bool(self.overflow.any())
            host = data[:, :int(n.max())].cpu().numpy()
            out += [host[b, :int(n[b])].tobytes() for b in range(chunk.shape[0])]
        return out


# ---- the container ------------------------------------------------------------------------------------------------------
AVI_LIMIT = (1 << 31) - (1 << 20)


def _fps_ratio(fps):
    """fps -> (rate, scale) of the stream header."""
    if float(fps) <= 0:
        raise ValueError(f"fps > 0, got {fps}")
    return (int(fps), 1) if float(fps) == int(fps) else (int(round(float(fps) * 1000)), 1000)


def pcm16(audio) -> np.ndarray:
    """fp32 samples in [-1, 1] (``load_wav16k``) -> little-endian int16: ``round(x 32768)`` clipped, which gives a
    16-bit wav its samples back."""
    a = np.asarray(audio.detach().cpu() if torch.is_tensor(audio) else audio, np.float64).reshape(-1)
    return np.clip(np.rint(a * 32768.0), -32768, 32767).astype("<i2")


class AviWriter:
    """A RIFF ``AVI `` file of JPEG frames (stream 0, ``MJPG``) and, with ``audio``, PCM16 mono at ``rate`` Hz (stream
    1), on the host.  ``hdrl`` (``avih``, one ``strl`` per stream), ``movi`` with one ``00dc`` chunk per frame followed by
    the ``01wb`` chunk of that frame's samples, ``idx1``.  Frame i carries the samples ``[e(i), e(i + 1))``, ``e(i) =
    round(i rate / fps)`` in integers, so the counts differ by one at the most and never drift; audio past the last
    frame is not written, frames past the audio carry none.  Sizes and counts are patched by ``close()``.

    The file is a plain AVI 1.0 (OpenDML is not provided): ``append`` raises before a chunk that would take it past
    2^31 - 2^20 bytes (``AVI_LIMIT``), index included."""

    def __init__(self, path, H, W, fps=25, audio=None, rate=16000):
        check_size(H, W)
        self.H, self.W, self.rate = int(H), int(W), int(rate)
        self.fps_rate, self.fps_scale = _fps_ratio(fps)
        self.audio = None if audio is None else pcm16(audio)
        self.frames, self.samples, self._index, self._largest = 0, 0, [], [0, 0]
        self._f = open(path, "wb")
        streams = 1 if self.audio is None else 2
        strl = self._strl(b"vids", b"MJPG", self.fps_scale, self.fps_rate, 0, struct.pack(
            "<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0), (self.W, self.H))
        if self.audio is not None:
            strl += self._strl(b"auds", b"\0\0\0\0", 1, self.rate, 2, struct.pack(
                "<HHIIHH", 1, 1, self.rate, 2 * self.rate, 2, 16), (0, 0))
        avih = struct.pack("<14I", 1000000 * self.fps_scale // self.fps_rate, 0, 0, 0x10, 0, 0, streams, 0, self.W,
                           self.H, 0, 0, 0, 0)
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        self._f.write(b"RIFF\0\0\0\0AVI LIST" + struct.pack("<I", len(hdrl)) + hdrl)
        self._movi = self._f.tell()                                              # of "LIST"; the fourcc "movi" is at + 8
        self._f.write(b"LIST\0\0\0\0movi")
        self._pos = self._f.tell()

    @staticmethod
    def _strl(kind, handler, scale, rate, sample_size, fmt, frame):
        strh = struct.pack("<4s4sIHHIIIIIIII4h", kind, handler, 0, 0, 0, 0, scale, rate, 0, 0, 0, 0xFFFFFFFF, sample_size,
                           0, 0, *frame)
        body = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(fmt)) + fmt
        return b"LIST" + struct.pack("<I", len(body)) + body

    def _chunk(self, fourcc, data, flags):
        size = 8 + len(data) + (len(data) & 1)
        if self._pos + size + 8 + 16 * (len(self._index) + 1) > AVI_LIMIT:
            raise ValueError(f"AviWriter: the file would pass {AVI_LIMIT} bytes (an AVI 1.0 file ends below 2 GiB; "
                             f"OpenDML is not provided): start a new file")
        self._f.write(fourcc + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1))
        self._index.append((fourcc, flags, self._pos - (self._movi + 8), len(data)))
        self._pos += size

    def _upto(self, i):
        return (2 * i * self.rate * self.fps_scale + self.fps_rate) // (2 * self.fps_rate)

    def append(self, jpeg: bytes):
        """One frame: a whole JPEG file."""
        if self._f is None:
            raise ValueError("AviWriter: closed")
        self._chunk(b"00dc", bytes(jpeg), 0x10)
        self._largest[0] = max(self._largest[0], len(jpeg))
        if self.audio is not None:
            a, b = (min(self._upto(self.frames + k), self.audio.size) for k in (0, 1))
            if b > a:
                self._chunk(b"01wb", self.audio[a:b].tobytes(), 0x10)
                self._largest[1] = max(self._largest[1], 2 * (b - a))
                self.samples = b
        self.frames += 1

    def close(self):
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
            for fourcc, flags, off, size in self._index:
                f.write(fourcc + struct.pack("<III", flags, off, size))
            end = f.tell()
            def patch(at, fmt, *v):
                f.seek(at)
                f.write(struct.pack(fmt, *v))
            patch(4, "<I", end - 8)
            patch(self._movi + 4, "<I", self._pos - self._movi - 8)
            avih = 32                                                            # RIFF 12, LIST 8, "hdrl" 4, "avih" + size 8
            patch(avih + 16, "<I", self.frames)                                  # dwTotalFrames
            patch(avih + 28, "<I", self._largest[0])                             # dwSuggestedBufferSize
            strh = avih + 56 + 12 + 8                                            # LIST, size, "strl", "strh", size
            patch(strh + 32, "<II", self.frames, self._largest[0])               # dwLength, dwSuggestedBufferSize
            if self.audio is not None:
                strh += 56 + 8 + 40 + 12 + 8
                patch(strh + 32, "<II", self.samples, self._largest[1])
        finally:
            f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _riff_chunks(buf, start, end):
    pos = start
    while pos + 8 <= end:
        fourcc, size = buf[pos:pos + 4], struct.unpack_from("<I", buf, pos + 4)[0]
        yield fourcc, pos + 8, size
        pos += 8 + size + (size & 1)


def read_avi(path, decoder=None):
    """-> (frames uint8 [N,H,W,3], fps, audio fp32 [L] in [-1, 1] or None) of a file ``AviWriter`` wrote (or any AVI 1.0
    with an MJPG stream 0 and PCM16 mono stream 1): walks ``movi`` in file order, PIL decodes the frames on the host.
    Two written videos go to ``metrics.frame_metrics`` this way, as the reference's metrics.py:189-217 reads its two.
    ``decoder``: a ``jpeg_decode.JpegDecoder``; the frames are then decoded on its device and come back there, with the
    same bytes (PIL's, uploaded, where its parser refuses a frame or the frames differ in size)."""
    from PIL import Image
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:4] != b"RIFF" or buf[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    fps, frames, audio = None, [], []
    for fourcc, at, size in _riff_chunks(buf, 12, len(buf)):
        if fourcc != b"LIST":
            continue
        kind = buf[at:at + 4]
        if kind == b"hdrl":
            for cc, a, n in _riff_chunks(buf, at + 4, at + size):
                if cc == b"LIST" and buf[a:a + 4] == b"strl" and buf[a + 12:a + 16] == b"vids" and fps is None:
                    scale, rate = struct.unpack_from("<II", buf, a + 12 + 20)
                    fps = rate / scale
        elif kind == b"movi":
            for cc, a, n in _riff_chunks(buf, at + 4, at + size):
                if cc == b"00dc":
                    frames.append(buf[a:a + n])
                elif cc == b"01wb":
                    audio.append(np.frombuffer(buf, "<i2", n // 2, a))
    if fps is None or not frames:
        raise ValueError(f"{path}: no video stream or no frame")
    sound = torch.from_numpy(np.concatenate(audio).astype(np.float32) / 32768.0) if audio else None
    got = decoder.decode_uniform(frames) if decoder is not None else None
    if got is not None:
        return got[0], fps, sound
    pixels = torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in frames]))
    return pixels if decoder is None else pixels.to(decoder.device), fps, sound


class VideoWriter:
    """``JpegEncoder`` and ``AviWriter`` together: ``append(frames_u8 [B,H,W,3] or [H,W,3])`` on ``device`` encodes
    there and writes the bytes.  A context manager; ``frames`` counts what was written."""

    def __init__(self, path, H, W, device, fps=25, quality=90, subsampling="4:2:0", audio=None, rate=16000, max_batch=None):
        self.encoder = JpegEncoder(H, W, device, quality=quality, subsampling=subsampling, max_batch=max_batch)
        self.avi = AviWriter(path, H, W, fps=fps, audio=audio, rate=rate)

    @property
    def frames(self):
        return self.avi.frames

    def append(self, frames_u8):
        for jpeg in self.encoder.encode_bytes(frames_u8[None] if frames_u8.dim() == 3 else frames_u8):
            self.avi.append(jpeg)

    def close(self):
        self.avi.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@torch.no_grad()
def write_video(renderer, frames, path, scene_backgrounds=None, audio=None, group=None, **kw) -> int:
    """synthesize_fuse.py:53-85, ``render_set``: renders ``frames`` with ``renderer`` (``infer.FuseRenderer(as_uint8=
    True)``) and writes them to ``path`` with ``audio`` (``load_wav16k``) beside them.  Rendered in groups as
    ``metrics.Evaluator`` does (``group``, default the renderer's ``frames_per_replay``, 1 without a graph); a short last
    group is padded with its last frame, which is not written.  ``kw`` goes to ``VideoWriter`` (fps, quality,
    subsampling).  -> the number of frames written."""
    if not getattr(renderer, "as_uint8", False):
        raise ValueError("write_video: the renderer must produce 8-bit frames (FuseRenderer(as_uint8=True))")
    if scene_backgrounds is not None and len(scene_backgrounds) != len(frames):
        raise ValueError("write_video: one scene background per frame")
    K = int(group or getattr(renderer, "frames_per_replay", 1))
    writer = None
    try:
        for g0 in range(0, len(frames), K):
            idx = [min(g0 + k, len(frames) - 1) for k in range(K)]
            n = min(K, len(frames) - g0)
            _, u8 = renderer.render_batch([frames[j] for j in idx],
                                          None if scene_backgrounds is None else [scene_backgrounds[j] for j in idx])
            if writer is None:
                writer = VideoWriter(path, u8.shape[1], u8.shape[2], u8.device, audio=audio, **kw)
            writer.append(u8[:n])
    finally:
        if writer is not None:
            writer.close()
    return 0 if writer is None else writer.frames
