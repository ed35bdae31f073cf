"""JPEG frames to pixels: a baseline JPEG decoder on the device (csrc/jpeg_decode.hip), the other direction of mjpeg.py.
What every preprocessing stage does first with ``PIL.Image.open`` on one host core ends here in a ``uint8 [B,H,W,3]``
tensor on the device, from the files' bytes.

The statement is ``jpeg_decode_torch``: integers only, and the rules are those of libjpeg's default decode path (what PIL
gives): the "islow" inverse DCT, "fancy" h2v2 upsampling, the 16-bit YCbCr -> RGB rule.  The device, this file and PIL
agree to the byte.  Its stages are public (``parse_jpeg``, ``coefficients_from_scan_torch``, ``pixels_torch``).

    parse_jpeg(data)                   -> JpegInfo, or UnsupportedJpeg naming the marker or field
    jpeg_decode_torch(files)           -> uint8 [B,H,W,3]
    JpegDecoder(device)                files (bytes) -> frames on the device: ``.decode``, ``.decode_checked``

Accepted: baseline sequential (SOF0, 8 bit), three components in one interleaved scan, 4:4:4 or 4:2:0, 8-bit quantisation
tables, any Huffman tables (per file), sides up to 4096.  Refused (``UnsupportedJpeg``): progressive and every other
SOFn, restart intervals, 16-bit tables, grayscale and CMYK, 4:2:2 and every other sampling, more than one scan, a missing
table, a scan that does not end in EOI.
"""
from __future__ import annotations

import dataclasses
import struct

import numpy as np
import torch

from .device_op import DeviceOperator
from .jpeg_common import (MAX_BATCH, MAX_SIDE, MCU_COMPONENTS, SUBSAMPLING, ZIGZAG, block_count, code_ranges, mcu_grid,
                          planes_from_blocks, sub_of)

STATUS = {1: "a code that is in no Huffman table", 2: "a coefficient index past 63",
          3: "the scan ends before the last block"}
SUB_BITS = 1024                                     # bits per subsequence of the parallel decode
# jidctint.c, 13 fraction bits: FIX(0.298631336) ... FIX(3.072711026)
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


class UnsupportedJpeg(ValueError):
    """A file ``parse_jpeg`` does not take; the message names the marker or the field."""


@dataclasses.dataclass
class JpegInfo:
    H: int
    W: int
    subsampling: str
    quant: torch.Tensor                             # int64 [3, 64], per component, row by row
    dc: tuple                                       # per component (bits 16 ints, vals)
    ac: tuple
    scan: tuple                                     # (offset, length) of the entropy-coded bytes between SOS and EOI


# ---- the file -----------------------------------------------------------------------------------------------------------
def _check_table(bits, vals, what):
    """Annex C: the codes of every length fit that length."""
    for length, (code, n, _) in enumerate(code_ranges(bits), 1):
        if code + n > 1 << length:
            raise UnsupportedJpeg(f"DHT {what}: more codes of length {length} than there are")
    if len(vals) > 256:
        raise UnsupportedJpeg(f"DHT {what}: more than 256 symbols")


def parse_jpeg(data: bytes) -> JpegInfo:
    """The headers of one file -> ``JpegInfo``; ``UnsupportedJpeg`` for everything outside the module's scope."""
    data = bytes(data)
    n = len(data)
    if data[:2] != b"\xff\xd8":
        raise UnsupportedJpeg("no SOI at the start: not a JPEG file")
    quant, huff, frame, restart = {}, {}, None, 0
    jfif, adobe = False, None
    pos = 2
    while True:
        if pos + 4 > n:
            raise UnsupportedJpeg("the file ends before SOS (truncated)")
        if data[pos] != 0xFF:
            raise UnsupportedJpeg(f"byte {pos}: a marker was expected")
        m = data[pos + 1]
        if m == 0xFF:                                                           # fill byte in front of a marker
            pos += 1
            continue
        if m == 0xD9:
            raise UnsupportedJpeg("EOI before any scan")
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            raise UnsupportedJpeg(f"marker 0xFF{m:02X} between the segments")
        length = struct.unpack_from(">H", data, pos + 2)[0]
        body, end = pos + 4, pos + 2 + length
        if length < 2 or end > n:
            raise UnsupportedJpeg(f"segment 0xFF{m:02X} runs past the end of the file (truncated)")
        seg = data[body:end]
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            if m == 0xE0 and seg[:5] == b"JFIF\0":
                jfif = True
            if m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    raise UnsupportedJpeg(f"DQT: Pq={pq} (16-bit quantisation table)")
                if tq > 3 or at + 65 > len(seg):
                    raise UnsupportedJpeg("DQT: table slot past 3, or a short segment")
                table = np.zeros(64, np.int64)
                table[np.asarray(ZIGZAG)] = np.frombuffer(seg, np.uint8, 64, at + 1)
                quant[tq] = table
                at += 65
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                tc, th = seg[at] >> 4, seg[at] & 15
                if tc > 1 or th > 3 or at + 17 > len(seg):
                    raise UnsupportedJpeg("DHT: table class past 1, slot past 3, or a short segment")
                bits = tuple(seg[at + 1:at + 17])
                count = sum(bits)
                if at + 17 + count > len(seg):
                    raise UnsupportedJpeg("DHT: a short segment")
                vals = tuple(seg[at + 17:at + 17 + count])
                _check_table(bits, vals, f"{'DA'[tc]}C {th}")
                huff[(tc, th)] = (bits, vals)
                at += 17 + count
        elif m == 0xC0:
            if frame is not None:
                raise UnsupportedJpeg("a second SOF0")
            if len(seg) < 6:
                raise UnsupportedJpeg("SOF0: a short segment")
            p, H, W, nf = struct.unpack_from(">BHHB", seg, 0)
            if p != 8:
                raise UnsupportedJpeg(f"SOF0: {p}-bit samples")
            if nf != 3:
                raise UnsupportedJpeg(f"SOF0: {nf} component{'s' if nf != 1 else ''} (grayscale and CMYK are not decoded)")
            if len(seg) != 6 + 3 * nf:
                raise UnsupportedJpeg("SOF0: a short segment")
            if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                raise UnsupportedJpeg(f"SOF0: 1 <= H, W <= {MAX_SIDE}, got {H} x {W}")
            frame = (H, W, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(3)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC8, 0xCC):
            names = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless"}
            raise UnsupportedJpeg(f"SOF{m - 0xC0} ({names.get(m, 'differential or arithmetic')}): only baseline SOF0")
        elif m == 0xDD:
            restart = struct.unpack_from(">H", seg, 0)[0] if len(seg) >= 2 else 1
            if restart != 0:
                raise UnsupportedJpeg(f"DRI: restart interval {restart} (restart markers are not decoded)")
        elif m == 0xDA:
            break
        else:
            raise UnsupportedJpeg(f"marker 0xFF{m:02X}")
        pos = end
    if frame is None:
        raise UnsupportedJpeg("SOS before SOF0")
    H, W, comps = frame
    if adobe is not None and adobe != 1 and not jfif:
        raise UnsupportedJpeg(f"APP14 Adobe transform {adobe}: not YCbCr")
    if adobe is None and not jfif and bytes(c[0] for c in comps) == b"RGB":
        raise UnsupportedJpeg("component ids R, G, B: not YCbCr")
    if len(seg) < 1 or seg[0] != 3:
        raise UnsupportedJpeg(f"SOS: {seg[0] if seg else 0} component(s) in the scan: more than one scan")
    if len(seg) != 10:
        raise UnsupportedJpeg("SOS: a short segment")
    if [seg[1 + 2 * i] for i in range(3)] != [c[0] for c in comps]:
        raise UnsupportedJpeg("SOS: the scan's components are not the frame's, in order")
    if tuple(seg[7:10]) != (0, 63, 0):
        raise UnsupportedJpeg(f"SOS: Ss, Se, Ah/Al = {tuple(seg[7:10])}, baseline has 0, 63, 0")
    sampling = tuple((c[1], c[2]) for c in comps)
    if sampling == ((1, 1),) * 3:
        subsampling = "4:4:4"
    elif sampling == ((2, 2), (1, 1), (1, 1)):
        subsampling = "4:2:0"
    else:
        raise UnsupportedJpeg("sampling " + "/".join(f"{h}x{v}" for h, v in sampling) + ": only 4:4:4 and 4:2:0")
    dc, ac, q = [], [], []
    for i, c in enumerate(comps):
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if c[3] not in quant or (0, td) not in huff or (1, ta) not in huff:
            raise UnsupportedJpeg(f"component {i}: a missing table (DQT {c[3]}, DHT DC {td}, DHT AC {ta})")
        q.append(quant[c[3]])
        dc.append(huff[(0, td)])
        ac.append(huff[(1, ta)])
    # the entropy-coded bytes: up to the first 0xFF that no 0x00 follows
    start = at = end
    while True:
        at = data.find(b"\xff", at)
        if at < 0 or at + 1 >= n:
            raise UnsupportedJpeg("the scan does not end in EOI (truncated)")
        if data[at + 1] != 0:
            break
        at += 2
    m = data[at + 1]
    if 0xD0 <= m <= 0xD7:
        raise UnsupportedJpeg(f"RST{m - 0xD0} in the scan (restart markers are not decoded)")
    if m == 0xDA:
        raise UnsupportedJpeg("a second SOS: more than one scan")
    if m != 0xD9:
        raise UnsupportedJpeg(f"marker 0xFF{m:02X} in the scan")
    return JpegInfo(H, W, subsampling, torch.from_numpy(np.stack(q)), tuple(dc), tuple(ac), (start, at - start))


# ---- the scan -----------------------------------------------------------------------------------------------------------
def unstuff(scan: bytes) -> bytes:
    """The scan without the 0x00 behind every 0xFF."""
    a = np.frombuffer(bytes(scan), np.uint8)
    drop = np.zeros(a.size, bool)
    drop[1:] = (a[1:] == 0) & (a[:-1] == 0xFF)
    return a[~drop].tobytes()


def decode_tables(bits, vals):
    """The canonical description of a Huffman table the device reads (include/instag_jpeg_decode.h): int32 limit[16],
    base[16] and uint8 vals[256]."""
    limit, base = np.zeros(16, np.int32), np.zeros(16, np.int32)
    for length, (code, n, k) in enumerate(code_ranges(bits), 1):
        limit[length - 1] = (code + n) << (16 - length)
        base[length - 1] = k - code
    v = np.zeros(256, np.uint8)
    v[:len(vals)] = vals
    return limit, base, v


def _lookup(bits, vals):
    """The next 16 bits -> length << 8 | symbol, 0 where they start no code."""
    out = np.zeros(65536, np.int32)
    for length, (code, n, k) in enumerate(code_ranges(bits), 1):
        for i in range(n):                                                      # every 16 bits that begin with code + i
            out[(code + i) << (16 - length):(code + i + 1) << (16 - length)] = vals[k + i] | length << 8
    return out.tolist()


def coefficients_from_scan_torch(info: JpegInfo, data: bytes) -> torch.Tensor:
    """-> int16 [nblk, 64]: the quantised coefficients in zig-zag order, the blocks in scan order, the DC summed per
    component (the layout of ``mjpeg.coefficients_torch``).  ITU T.81 Annex F, sequentially: a DC category s and its s
    bits v, ``v < 2^(s-1) ? v - 2^s + 1 : v``; AC symbols (run, size), ZRL (15, 0) for sixteen zeros, (r, 0) the end of
    the block.  Stops by block count; bits past the end read as 1.  ValueError: a code in no table (or a DC category
    past 15), a coefficient index past 63, the scan ending before the last block."""
    raw = unstuff(bytes(data)[info.scan[0]:info.scan[0] + info.scan[1]])
    nbits = 8 * len(raw)
    raw += b"\xff" * 8
    nblk = block_count(info.H, info.W, info.subsampling)
    per = MCU_COMPONENTS[sub_of(info.subsampling)]
    dc = [_lookup(*t) for t in info.dc]
    ac = [_lookup(*t) for t in info.ac]
    out = np.zeros((nblk, 64), np.int64)
    pred = [0, 0, 0]
    p = 0
    for blk in range(nblk):
        c = per[blk % len(per)]
        k = 0
        while k < 64:
            v = int.from_bytes(raw[p >> 3:(p >> 3) + 5], "big") >> (8 - (p & 7)) & 0xFFFFFFFF
            e = (dc[c] if k == 0 else ac[c])[v >> 16]
            n, sym = e >> 8, e & 255
            if n == 0 or (k == 0 and sym > 15):
                raise ValueError(f"block {blk}: {STATUS[1]}")
            run, size = (0, sym) if k == 0 else (sym >> 4, sym & 15)
            if k and size == 0:
                if run != 15:
                    k = 64
                else:
                    k += 16
                    if k > 64:
                        raise ValueError(f"block {blk}: {STATUS[2]}")
                p += n
            else:
                k += run
                if k > 63:
                    raise ValueError(f"block {blk}: {STATUS[2]}")
                bitsv = (v << n & 0xFFFFFFFF) >> (32 - size) if size else 0
                out[blk, k] = bitsv if size == 0 or bitsv >> (size - 1) else bitsv - (1 << size) + 1
                p += n + size
                k += 1
            if p > nbits:
                raise ValueError(f"block {blk}: {STATUS[3]}")
        pred[c] += int(out[blk, 0])
        out[blk, 0] = pred[c]
    return torch.from_numpy(((out + 32768) % 65536 - 32768).astype(np.int16))


# ---- the pixels ---------------------------------------------------------------------------------------------------------
def _idct_pass(x, up, shift):
    """One pass of jidctint.c's jpeg_idct_islow over the eight tensors ``x``: the even part's x0, x4 scaled by 2^13
    (``up``), the result descaled by ``shift`` with rounding."""
    z1 = (x[2] + x[6]) * F_0_541
    tmp2 = z1 - x[6] * F_1_847
    tmp3 = z1 + x[2] * F_0_765
    tmp0, tmp1 = (x[0] + x[4]) << up, (x[0] - x[4]) << up
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2 = -z1 * F_0_899, -z2 * F_2_562
    z3, z4 = z5 - z3 * F_1_961, z5 - z4 * F_0_390
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    half = 1 << (shift - 1)
    return [(v + half) >> shift for v in (tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0,
                                          tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3)]


def idct_torch(coef, quant):
    """coef [..., 64] in zig-zag order, quant [..., 64] row by row (broadcast) -> samples int64 [..., 8, 8] in 0..255:
    ``d = coef q``; columns, ``(x + 1024) >> 11``; rows, ``(x + 131072) >> 18``; + 128, clamped."""
    zz = torch.tensor(ZIGZAG, device=coef.device)
    d = torch.zeros(coef.shape, dtype=torch.int64, device=coef.device)
    d[..., zz] = coef.to(torch.int64)
    d = (d * quant.to(torch.int64)).reshape(*coef.shape[:-1], 8, 8)
    ws = torch.stack(_idct_pass([d[..., r, :] for r in range(8)], 13, 11), -2)
    out = torch.stack(_idct_pass([ws[..., :, c] for c in range(8)], 13, 18), -1)
    return (out + 128).clamp(0, 255)


def upsample_torch(c, H, W):
    """One chroma plane int64 [h, w] of a 4:2:0 file -> [H, W].  libjpeg's h2v2 "fancy" rule on the plane cropped to
    ceil(H/2) x ceil(W/2), its edge rows and columns repeated: ``t = 3 cur + neighbour`` (the row above for the upper
    output row, below for the lower), ``out[2j] = (3 t[j] + t[j-1] + 8) >> 4``, ``out[2j+1] = (3 t[j] + t[j+1] + 7) >>
    4``.  As libjpeg does, a plane of one or two columns is repeated 2 x 2 instead."""
    ch, cw = -(-H // 2), -(-W // 2)
    c = c[:ch, :cw]
    if cw <= 2:
        return c.repeat_interleave(2, 0).repeat_interleave(2, 1)[:H, :W]
    rows = torch.arange(ch, device=c.device)
    t = torch.stack([3 * c + c[(rows - 1).clamp(min=0)], 3 * c + c[(rows + 1).clamp(max=ch - 1)]], 1).reshape(2 * ch, cw)
    cols = torch.arange(cw, device=c.device)
    out = torch.stack([(3 * t + t[:, (cols - 1).clamp(min=0)] + 8) >> 4,
                       (3 * t + t[:, (cols + 1).clamp(max=cw - 1)] + 7) >> 4], 2).reshape(2 * ch, 2 * cw)
    return out[:H, :W]


def colour_torch(Y, Cb, Cr):
    """int64 planes -> uint8 [..., 3]: ``R = Y + ((91881 cr + 32768) >> 16)``, ``B = Y + ((116130 cb + 32768) >> 16)``,
    ``G = Y + ((-22554 cb - 46802 cr + 32768) >> 16)`` with cb, cr the planes less 128, arithmetic shifts, each clamped."""
    cb, cr = Cb - 128, Cr - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return torch.stack([R, G, B], -1).clamp(0, 255).to(torch.uint8)


def pixels_torch(coef, quant, H, W, subsampling="4:2:0"):
    """coef int16 [nblk, 64] (``coefficients_from_scan_torch``), quant [3, 64] -> uint8 [H, W, 3]: inverse DCT per block
    (``idct_torch``), the planes put together, 4:2:0 chroma upsampled (``upsample_torch``), colour, cropped."""
    s = sub_of(subsampling)
    nblk = block_count(H, W, subsampling)
    if coef.dim() != 2 or tuple(coef.shape) != (nblk, 64) or tuple(quant.shape) != (3, 64):
        raise ValueError(f"coef is [{nblk}, 64] and quant [3, 64], got {tuple(coef.shape)} and {tuple(quant.shape)}")
    my, mx = mcu_grid(H, W, s)
    comp = torch.tensor(MCU_COMPONENTS[s] * (my * mx), device=coef.device)
    Y, Cb, Cr = planes_from_blocks(idct_torch(coef, quant.to(coef.device)[comp]), s, my, mx)
    if s == 2:
        Cb, Cr = upsample_torch(Cb, H, W), upsample_torch(Cr, H, W)
    return colour_torch(Y[:H, :W], Cb[:H, :W], Cr[:H, :W])


def jpeg_decode_torch(files) -> torch.Tensor:
    """Files of one size -> uint8 [B,H,W,3] (the statement of ``JpegDecoder``)."""
    out = []
    for f in files:
        info = parse_jpeg(f)
        out.append(pixels_torch(coefficients_from_scan_torch(info, f), info.quant, info.H, info.W, info.subsampling))
    if not out or any(o.shape != out[0].shape for o in out):
        raise ValueError("jpeg_decode_torch: at least one file, and all of one size")
    return torch.stack(out)


# ---- the device path ----------------------------------------------------------------------------------------------------
class _Nothing:
    """``DeviceOperator`` keeps nothing on the device for the decoder: the tables travel with every file."""

    def device_pack(self, device):
        return None, ()


class JpegDecoder(DeviceOperator):
    """Baseline JPEG files of one size to uint8 [B,H,W,3] frames on ``device`` (a CPU device runs the statement).

    ``max_batch``: files per launch (default and at most 64); ``sub_bits``: bits per subsequence of the parallel Huffman
    decode, a multiple of 32 in 64..4096 (default ``SUB_BITS``; the result does not depend on it).  ``decode`` never
    synchronises: a scan that cannot be decoded sets ``status`` (``STATUS``) and leaves its frame unspecified;
    ``decode_checked`` reads the status and raises."""

    CHECK = "check_arg"

    def __init__(self, device, max_batch=None, sub_bits=None):
        super().__init__(_Nothing(), device)
        self.max_batch = self._at_least_one(max_batch) or MAX_BATCH
        self.sub_bits = SUB_BITS if sub_bits is None else int(sub_bits)
        if self.max_batch > MAX_BATCH:
            raise ValueError(f"JpegDecoder: max_batch <= {MAX_BATCH}, got {self.max_batch}")
        if self.sub_bits % 32 or not 64 <= self.sub_bits <= 4096:
            raise ValueError(f"JpegDecoder: sub_bits is a multiple of 32 in 64..4096, got {sub_bits}")

    # -- host side
    @staticmethod
    def parse(files, infos=None):
        """-> ([JpegInfo], H, W, subsampling): ValueError unless there is a file and all share the three.  ``infos``:
        what ``parse_jpeg`` gave for the files, where the caller has it."""
        infos = [parse_jpeg(f) for f in files] if infos is None else list(infos)
        if not infos:
            raise ValueError("JpegDecoder: at least one file")
        key = {(i.H, i.W, i.subsampling) for i in infos}
        if len(key) != 1:
            raise ValueError(f"JpegDecoder: the files of a call share (H, W, subsampling), got {sorted(key)}")
        return (infos,) + key.pop()

    def pack(self, files, infos, capacity=None):
        """The pinned staging tensors of a call: scans uint8 [B, capacity], scan_bytes int32 [B], huffman uint8 [B, 6,
        384] (``decode_tables`` of DC Y, Cb, Cr, AC Y, Cb, Cr), quant uint16 [B, 3, 64]."""
        B = len(files)
        cap = int(capacity or max(4, max(i.scan[1] for i in infos)))
        if any(i.scan[1] > cap for i in infos):
            raise ValueError(f"JpegDecoder: a scan of {max(i.scan[1] for i in infos)} bytes, capacity {cap}")
        pin = self.device.type == "cuda"
        scans = torch.zeros(B, cap, dtype=torch.uint8, pin_memory=pin)
        nbytes = torch.zeros(B, dtype=torch.int32, pin_memory=pin)
        huffman = torch.zeros(B, 6, 384, dtype=torch.uint8, pin_memory=pin)
        quant = torch.zeros(B, 3, 64, dtype=torch.uint16, pin_memory=pin)
        sv, hv, qv = scans.numpy(), huffman.numpy(), quant.numpy()
        cache = {}
        for b, (f, i) in enumerate(zip(files, infos)):
            sv[b, :i.scan[1]] = np.frombuffer(f, np.uint8, i.scan[1], i.scan[0])
            nbytes[b] = i.scan[1]
            qv[b] = i.quant.numpy().astype(np.uint16)
            for t, table in enumerate(i.dc + i.ac):
                if table not in cache:
                    limit, base, vals = decode_tables(*table)
                    cache[table] = np.concatenate([limit.view(np.uint8), base.view(np.uint8), vals])
                hv[b, t] = cache[table]
        return scans, nbytes, huffman, quant

    def _upload(self, *tensors):
        return tuple(t.to(self.device, non_blocking=True) for t in tensors)

    def _nbytes(self, B, H, W, sub, capacity):
        from . import _lib
        return _lib.workspace_bytes(self._L.instag_jpeg_decode_workspace_bytes(
            min(B, self.max_batch), H, W, sub, capacity, self.sub_bits))

    # -- the calls
    def decode(self, files, infos=None):
        """-> (frames uint8 [B,H,W,3], status int32 [B]) on the device; never synchronises."""
        infos, H, W, subsampling = self.parse(files, infos)
        if self.device.type != "cuda":
            return self._statement_decode(files, infos, H, W, subsampling)
        scans, nbytes, huffman, quant = self._upload(*self.pack(files, infos))
        frames = torch.empty(len(files), H, W, 3, dtype=torch.uint8, device=self.device)
        status = torch.empty(len(files), dtype=torch.int32, device=self.device)
        self.decode_into(scans, nbytes, huffman, quant, subsampling, frames, status)
        return frames, status

    def decode_into(self, scans, scan_bytes, huffman, quant, subsampling, frames, status):
        """``decode`` from packed device tensors (``pack``) into the caller's ``frames`` uint8 [B,H,W,3] and ``status``
        int32 [B]: launches on the current stream only, so it can be captured."""
        from . import _lib
        B, H, W, _ = frames.shape
        sub, cap = sub_of(subsampling), int(scans.shape[1])
        self._check_packed(B, scans, scan_bytes, huffman, quant)
        if (frames.dtype != torch.uint8 or frames.shape[3] != 3 or not frames.is_contiguous() or status.dtype != torch.int32
                or tuple(status.shape) != (B,) or not status.is_contiguous()):
            raise ValueError("JpegDecoder: frames uint8 [B,H,W,3] and status int32 [B], contiguous")
        self._each_chunk(B, self._nbytes(B, H, W, sub, cap), lambda sl, m, p, size: self._L.instag_jpeg_decode(
            _lib.ptr(scans[sl]), cap, _lib.ptr(scan_bytes[sl]), _lib.ptr(huffman[sl]), _lib.ptr(quant[sl]), m, H, W, sub,
            self.sub_bits, _lib.ptr(frames[sl]), _lib.ptr(status[sl]), p, size, _lib.current_stream()), "jpeg_decode")

    def _check_packed(self, B, scans, scan_bytes, huffman, quant):
        ok = (scans.dtype == torch.uint8 and scans.dim() == 2 and scans.shape[0] == B and scans.is_contiguous()
              and scan_bytes.dtype == torch.int32 and tuple(scan_bytes.shape) == (B,) and scan_bytes.is_contiguous()
              and (huffman is None or (huffman.dtype == torch.uint8 and tuple(huffman.shape) == (B, 6, 384)
                                       and huffman.is_contiguous()))
              and (quant is None or (quant.dtype == torch.uint16 and tuple(quant.shape) == (B, 3, 64)
                                     and quant.is_contiguous())))
        if not ok or B < 1:
            raise ValueError("JpegDecoder: scans uint8 [B, capacity], scan_bytes int32 [B], huffman uint8 [B,6,384], quant "
                             "uint16 [B,3,64], contiguous, B >= 1")

    def _statement_decode(self, files, infos, H, W, subsampling):
        frames = torch.zeros(len(files), H, W, 3, dtype=torch.uint8)
        status = torch.zeros(len(files), dtype=torch.int32)
        for b, (f, i) in enumerate(zip(files, infos)):
            try:
                frames[b] = pixels_torch(coefficients_from_scan_torch(i, f), i.quant, H, W, subsampling)
            except ValueError as e:
                status[b] = next(k for k, v in STATUS.items() if v in str(e))
        return frames, status

    def coefficients(self, files, with_status=False):
        """-> int16 [B, nblk, 64] (``coefficients_from_scan_torch``); ``with_status``: and the status int32 [B]."""
        infos, H, W, subsampling = self.parse(files)
        B = len(files)
        if self.device.type != "cuda":
            coef = torch.stack([coefficients_from_scan_torch(i, f) for f, i in zip(files, infos)])
            return (coef, torch.zeros(B, dtype=torch.int32)) if with_status else coef
        scans, nbytes, huffman, _ = self._upload(*self.pack(files, infos))
        return self.coefficients_of(scans, nbytes, huffman, H, W, subsampling, with_status)

    def coefficients_of(self, scans, scan_bytes, huffman, H, W, subsampling, with_status=False, coef=None, status=None):
        """``coefficients`` of scans that are on the device already (rows of a ``JpegEncoder.encode`` behind the header):
        ``scans`` uint8 [B, capacity], ``scan_bytes`` int32 [B], ``huffman`` uint8 [B, 6, 384]."""
        from . import _lib
        B, sub, cap = int(scans.shape[0]), sub_of(subsampling), int(scans.shape[1])
        self._check_packed(B, scans, scan_bytes, huffman, None)
        nblk = block_count(H, W, subsampling)
        coef = torch.empty(B, nblk, 64, dtype=torch.int16, device=self.device) if coef is None else coef
        status = torch.empty(B, dtype=torch.int32, device=self.device) if status is None else status
        self._each_chunk(B, self._nbytes(B, H, W, sub, cap), lambda sl, m, p, size: self._L.instag_jpeg_decode_coefficients(
            _lib.ptr(scans[sl]), cap, _lib.ptr(scan_bytes[sl]), _lib.ptr(huffman[sl]), m, H, W, sub, self.sub_bits,
            _lib.ptr(coef[sl]), _lib.ptr(status[sl]), p, size, _lib.current_stream()), "jpeg_decode_coefficients")
        return (coef, status) if with_status else coef

    def pixels(self, coef, quant, H, W, subsampling="4:2:0", frames=None):
        """coef int16 [B, nblk, 64], quant [3, 64] or [B, 3, 64] -> uint8 [B,H,W,3] (``pixels_torch`` per frame)."""
        sub, nblk = sub_of(subsampling), block_count(H, W, subsampling)
        if coef.dtype != torch.int16 or coef.dim() != 3 or tuple(coef.shape[1:]) != (nblk, 64) or coef.shape[0] < 1:
            raise ValueError(f"JpegDecoder: coef int16 [B,{nblk},64], got {coef.dtype} {tuple(coef.shape)}")
        B = coef.shape[0]
        quant = torch.as_tensor(quant)
        packed = quant.dtype == torch.uint16                                    # (``pack``'s: 8-bit tables by construction)
        if quant.dim() == 2:
            quant = quant[None].expand(B, 3, 64)
        if tuple(quant.shape) != (B, 3, 64) or (not packed and (int(quant.min()) < 1 or int(quant.max()) > 255)):
            raise ValueError("JpegDecoder: quant [3, 64] or [B, 3, 64] of 1..255")
        if self.device.type != "cuda":
            return torch.stack([pixels_torch(coef[b], quant[b], H, W, subsampling) for b in range(B)])
        from . import _lib
        coef = coef.to(self.device).contiguous()
        q16 = (quant if packed else quant.to(torch.int32).to(torch.uint16)).contiguous().to(self.device)
        frames = torch.empty(B, H, W, 3, dtype=torch.uint8, device=self.device) if frames is None else frames
        nbytes = _lib.workspace_bytes(self._L.instag_jpeg_decode_workspace_bytes(min(B, self.max_batch), H, W, sub, 1, 64))
        self._each_chunk(B, nbytes, lambda sl, m, p, size: self._L.instag_jpeg_decode_pixels(
            _lib.ptr(coef[sl]), _lib.ptr(q16[sl]), m, H, W, sub, _lib.ptr(frames[sl]), p, size, _lib.current_stream()),
            "jpeg_decode_pixels")
        return frames

    def decode_checked(self, files, infos=None):
        """``decode`` -> frames, after one synchronisation: ValueError naming the first file whose scan is damaged."""
        frames, status = self.decode(files, infos)
        bad = status.cpu().tolist()
        for b, s in enumerate(bad):
            if s:
                raise ValueError(f"JpegDecoder: file {b} of the call: {STATUS.get(s, f'status {s}')}")
        return frames

    def decode_uniform(self, files, want=None):
        """-> (``decode_checked``'s frames, ``MAX_BATCH`` files at a time, (W, H)); None where ``parse_jpeg`` refuses a file,
        the files do not share (H, W, subsampling) or their size is not ``want`` (a (W, H)).  A damaged scan still raises."""
        try:
            infos, H, W, _ = self.parse(files)
        except ValueError:                                                      # (UnsupportedJpeg is one)
            return None
        if want is not None and tuple(want) != (W, H):
            return None
        pieces = [self.decode_checked(files[i:i + MAX_BATCH], infos[i:i + MAX_BATCH]) for i in range(0, len(files), MAX_BATCH)]
        return pieces[0] if len(pieces) == 1 else torch.cat(pieces), (W, H)
