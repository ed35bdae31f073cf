"""What the JPEG encoder and decoder (mjpeg.py, jpeg_decode.py) share: the zig-zag order, the limits, the MCU grid and
the order of its blocks, the layout between planes and scan-order blocks, and the Annex C walk over a Huffman table's
``bits``.  csrc/jpeg_common.hpp is the same on the C side."""
import functools

import numpy as np
import torch

# zig-zag position k -> index in the 8 x 8 block, row by row
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63)
SUBSAMPLING = {"4:4:4": 1, "4:2:0": 2}              # -> the C side's `sub`: the chroma planes' divisor
MCU_COMPONENTS = {1: (0, 1, 2), 2: (0, 0, 0, 0, 1, 2)}   # sub -> 0 (Y), 1 (Cb) or 2 (Cr) per block of an MCU in scan order
MAX_SIDE, MAX_BATCH = 4096, 64


def sub_of(subsampling) -> int:
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling is '4:2:0' or '4:4:4', got {subsampling!r}")
    return SUBSAMPLING[subsampling]


def check_size(H, W):
    if not (1 <= int(H) <= MAX_SIDE and 1 <= int(W) <= MAX_SIDE):
        raise ValueError(f"1 <= H, W <= {MAX_SIDE}, got {H} x {W}")


def mcu_grid(H, W, s):
    """-> (my, mx): the MCUs (8 s x 8 s pixels) down and across a frame."""
    return -(-int(H) // (8 * s)), -(-int(W) // (8 * s))


def block_count(H, W, subsampling="4:2:0") -> int:
    """Blocks of one frame's scan: 3 per 8 x 8 MCU at 4:4:4, 6 per 16 x 16 MCU at 4:2:0."""
    check_size(H, W)
    my, mx = mcu_grid(H, W, sub_of(subsampling))
    return my * mx * len(MCU_COMPONENTS[sub_of(subsampling)])


def block_components(H, W, subsampling="4:2:0") -> np.ndarray:
    """int64 [nblk]: 0 (Y), 1 (Cb) or 2 (Cr) for every block in scan order."""
    per = MCU_COMPONENTS[sub_of(subsampling)]
    return np.tile(np.asarray(per, np.int64), block_count(H, W, subsampling) // len(per))


def blocks_from_planes(Y, Cb, Cr, s):
    """Y [B, 8 s my, 8 s mx], Cb, Cr [B, 8 my, 8 mx] -> [B, nblk, 8, 8]: the blocks in scan order, MCU by MCU row by
    row, per MCU its s x s Y blocks row by row, Cb, Cr (``block_components``).  The inverse of ``planes_from_blocks``."""
    B = Y.shape[0]
    Yb, Cbb, Crb = (p.view(B, p.shape[1] // 8, 8, p.shape[2] // 8, 8).permute(0, 1, 3, 2, 4) for p in (Y, Cb, Cr))
    my, mx = Cbb.shape[1], Cbb.shape[2]
    Yb = Yb.reshape(B, my, s, mx, s, 8, 8).permute(0, 1, 3, 2, 4, 5, 6).reshape(B, my * mx, s * s, 8, 8)
    return torch.cat([Yb, Cbb.reshape(B, my * mx, 1, 8, 8), Crb.reshape(B, my * mx, 1, 8, 8)], 2).reshape(B, -1, 8, 8)


def planes_from_blocks(px, s, my, mx):
    """px [..., nblk, 8, 8] in scan order -> (Y [..., 8 s my, 8 s mx], Cb, Cr [..., 8 my, 8 mx]).  The inverse of
    ``blocks_from_planes``."""
    lead = tuple(px.shape[:-3])
    px = px.reshape(-1, my, mx, s * s + 2, 8, 8)
    Y = px[:, :, :, :s * s].reshape(-1, my, mx, s, s, 8, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(*lead, my * s * 8, mx * s * 8)
    Cb, Cr = (px[:, :, :, s * s + i].permute(0, 1, 3, 2, 4).reshape(*lead, my * 8, mx * 8) for i in (0, 1))
    return Y, Cb, Cr


@functools.lru_cache(maxsize=256)
def _code_ranges(bits):
    out, code, k = [], 0, 0
    for n in bits:
        out.append((code, n, k))
        code, k = (code + n) << 1, k + n
    return tuple(out)


def code_ranges(bits):
    """Annex C: per code length 1..16 of the table with ``bits[l - 1]`` codes of length l, (the first code, the number
    of codes, the index of the first one's symbol).  The codes of a length count up from the first.  (Kept per ``bits``:
    the files of a video share their tables, and the parser walks each file's four.)"""
    return _code_ranges(tuple(bits))
