"""CPU: what the JPEG encoder and decoder share (instag_amd/jpeg_common.py): the layout pair between planes and
scan-order blocks, the Annex C walk under the three table functions, and ``JpegDecoder.decode_uniform``."""
import numpy as np
import pytest
import torch

from tests import jpeg_decode_helpers as J
from tests import mjpeg_helpers as Hh


# ---- the layout pair ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", Hh.SUBS)
def test_blocks_from_planes_and_planes_from_blocks_are_inverses_in_the_stated_order(sub):
    """24 x 40 pixels per chroma sample: 3 x 5 MCUs, more than one each way and my != mx.  Every sample carries its
    component, MCU row and column, block and position, so a block in the wrong place or turned shows."""
    from instag_amd import jpeg_common as C
    s = C.sub_of(sub)
    my, mx = 3, 5
    H, W = 8 * s * my, 8 * s * mx
    assert C.mcu_grid(H, W, s) == (my, mx) and C.mcu_grid(H - 1, W - 8 * s + 1, s) == (my, mx)

    def plane(comp, h, w):
        y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        return torch.stack([(comp * 10000 + y * 100 + x) * (b + 1) for b in range(2)])

    Y, Cb, Cr = plane(0, H, W), plane(1, H // s, W // s), plane(2, H // s, W // s)
    blocks = C.blocks_from_planes(Y, Cb, Cr, s)
    comp = C.block_components(H, W, sub)
    assert tuple(blocks.shape) == (2, C.block_count(H, W, sub), 8, 8) and comp.shape == (blocks.shape[1],)
    assert torch.equal(blocks[:, :, 0, 0] // 10000, torch.from_numpy(comp)[None] * torch.tensor([[1], [2]]))
    per = s * s + 2
    for g in range(blocks.shape[1]):                                          # block g holds the 8 x 8 samples at its place
        m, j = divmod(g, per)
        src, r, c = ((Y, (m // mx * s + j // s) * 8, (m % mx * s + j % s) * 8) if j < s * s else
                     ((Cb, Cr)[j - s * s], m // mx * 8, m % mx * 8))
        assert torch.equal(blocks[:, g], src[:, r:r + 8, c:c + 8]), g
    back = C.planes_from_blocks(blocks, s, my, mx)
    assert all(torch.equal(a, b) for a, b in zip(back, (Y, Cb, Cr)))
    one = C.planes_from_blocks(blocks[1], s, my, mx)                          # (no batch: what pixels_torch passes)
    assert all(torch.equal(a, b[1]) for a, b in zip(one, (Y, Cb, Cr)))
    assert torch.equal(C.blocks_from_planes(*back, s), blocks)


# ---- the Annex C walk ---------------------------------------------------------------------------------------------------
# the three functions as they stood before they shared ``code_ranges``
def _old_huffman_codes(bits, vals):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _old_check_table(bits, vals, what):
    from instag_amd.jpeg_decode import UnsupportedJpeg
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > 1 << length:
            raise UnsupportedJpeg(f"DHT {what}: more codes of length {length} than there are")
        code <<= 1
    if len(vals) > 256:
        raise UnsupportedJpeg(f"DHT {what}: more than 256 symbols")


def _old_decode_tables(bits, vals):
    limit, base = np.zeros(16, np.int32), np.zeros(16, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        limit[length - 1] = (code + bits[length - 1]) << (16 - length)
        base[length - 1] = k - code
        code, k = (code + bits[length - 1]) << 1, k + bits[length - 1]
    v = np.zeros(256, np.uint8)
    v[:len(vals)] = vals
    return limit, base, v


def _outcome(fn, *args):
    try:
        return fn(*args)
    except ValueError as e:
        return type(e), str(e)


def _tables():
    from instag_amd import jpeg_decode as D, mjpeg as M
    info = D.parse_jpeg(J.pil_encode(J.content(40, 56).numpy(), quality=90, optimize=True))
    assert info.ac[0] != (M.AC_LUMA_BITS, M.AC_LUMA_VALS)                     # (PIL's own table, not Annex K's)
    return {"dc_luma": (M.DC_LUMA_BITS, M.DC_VALS), "dc_chroma": (M.DC_CHROMA_BITS, M.DC_VALS),
            "ac_luma": (M.AC_LUMA_BITS, M.AC_LUMA_VALS), "ac_chroma": (M.AC_CHROMA_BITS, M.AC_CHROMA_VALS),
            "pil_optimised_ac": info.ac[0]}


@pytest.mark.parametrize("name", ("dc_luma", "dc_chroma", "ac_luma", "ac_chroma", "pil_optimised_ac"))
def test_code_ranges_and_the_three_table_functions_on_it(name):
    from instag_amd import jpeg_common as C, jpeg_decode as D, mjpeg as M
    bits, vals = _tables()[name]
    ranges = C.code_ranges(bits)
    assert len(ranges) == 16 and [n for _, n, _ in ranges] == list(bits) and ranges[0][0] == 0 and ranges[0][2] == 0
    for (code, n, k), (code1, _, k1) in zip(ranges, ranges[1:]):              # Annex C, figure C.2
        assert code1 == (code + n) << 1 and k1 == k + n
    want = _old_huffman_codes(bits, vals)
    got = M.huffman_codes(bits, vals)
    assert got == want and list(got) == list(want) and len(got) == len(vals) == sum(bits)
    for length, (code, n, k) in enumerate(ranges, 1):
        assert all(got[vals[k + i]] == (code + i, length) for i in range(n))
    for a, b in zip(D.decode_tables(bits, vals), _old_decode_tables(bits, vals)):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    assert D._check_table(bits, vals, "AC 0") is None and _old_check_table(bits, vals, "AC 0") is None


def test_check_table_refuses_what_it_refused():
    """Too many codes of a length (the first such length is named), and too many symbols."""
    from instag_amd import jpeg_decode as D
    crowded = (0, 2, 5) + (0,) * 13                                           # 2 of length 2 leave 4 of length 3
    late = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3)                    # only the last length overflows
    many = (0,) * 8 + (255,) + (0,) * 6 + (2,)
    for bits, vals in ((crowded, tuple(range(7))), (late, tuple(range(18))), (many, tuple(range(257))), ((3,) + (0,) * 15, (1, 2, 3))):
        want = _outcome(_old_check_table, bits, vals, "DC 1")
        assert want[0] is D.UnsupportedJpeg and _outcome(D._check_table, bits, vals, "DC 1") == want, bits


# ---- decode_uniform -----------------------------------------------------------------------------------------------------
def test_decode_uniform_on_a_cpu_decoder():
    from instag_amd import jpeg_decode as D
    dec = D.JpegDecoder(torch.device("cpu"))
    frames = [J.content(24, 40, seed).numpy() for seed in range(3)]
    files = [J.pil_encode(f, quality=90, optimize=bool(i & 1)) for i, f in enumerate(frames)]
    got = dec.decode_uniform(files)
    assert got is not None and got[1] == (40, 24)                             # (width, height)
    assert got[0].dtype == torch.uint8 and tuple(got[0].shape) == (3, 24, 40, 3)
    assert all(torch.equal(got[0][i], J.pil_pixels(f)) for i, f in enumerate(files))
    same = dec.decode_uniform(files, want=(40, 24))
    assert same[1] == (40, 24) and torch.equal(same[0], got[0])
    assert dec.decode_uniform(files, want=(24, 40)) is None                   # another size is wanted
    assert dec.decode_uniform(files[:2] + [J.pil_encode(frames[2], progressive=True)]) is None
    assert dec.decode_uniform(files[:2] + [J.pil_encode(J.content(24, 48).numpy())]) is None
    assert dec.decode_uniform(files[:2] + [J.pil_encode(frames[2], subsampling=0)]) is None
    with pytest.raises(ValueError, match="file 1 of the call: the scan ends before the last block") as e:
        dec.decode_uniform([files[0], J.cut_scan(files[1]), files[2]])
    assert not isinstance(e.value, D.UnsupportedJpeg)
