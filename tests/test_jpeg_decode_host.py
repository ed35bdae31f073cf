"""CPU: the statement of the JPEG decoder (instag_amd/jpeg_decode.py) against PIL, byte for byte: this project's encoder's
files and PIL's own; the scan decoder against the encoder's coefficients; what the parser refuses; the C entry points'
argument checks."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_decode_helpers as J
from tests import mjpeg_helpers as Hh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_jpeg_decode.npz")


# ---- the statement against PIL ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", Hh.SUBS)
@pytest.mark.parametrize("name", Hh.CASES)
def test_encoder_files_decode_to_pil_s_bytes_and_the_encoder_s_coefficients(name, sub):
    from instag_amd import jpeg_decode as D
    data, coef, _ = Hh.statement(name, sub)
    info = D.parse_jpeg(data)
    frame = Hh.cases()[name][0]
    assert (info.H, info.W, info.subsampling) == (frame.shape[0], frame.shape[1], sub)
    got = J.statement_coefficients(data)
    assert got.dtype == torch.int16 and torch.equal(got, coef)               # shares no code with scan_torch
    px = J.statement_pixels(data)
    assert px.dtype == torch.uint8 and tuple(px.shape) == tuple(frame.shape) and torch.equal(px, J.pil_pixels(data))


@pytest.mark.parametrize("subsampling", sorted(J.PIL_SUBS))
@pytest.mark.parametrize("size", J.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pil_written_files_decode_to_pil_s_bytes(size, subsampling):
    """Quality 30 / 75 / 95 / 100, standard and optimised Huffman tables."""
    from instag_amd import jpeg_decode as D
    files = J.pil_files(size, subsampling)
    assert len(files) == 8 and len(set(files)) == 8
    optimised = [D.parse_jpeg(f).ac for f in files]
    assert optimised[0] == optimised[2] != optimised[1]                      # (per-file tables are in play)
    for f in files:
        info = D.parse_jpeg(f)
        assert (info.H, info.W, info.subsampling) == (*size, J.PIL_SUBS[subsampling])
        assert torch.equal(J.statement_pixels(f), J.pil_pixels(f))
    batch = D.jpeg_decode_torch(list(files))
    assert tuple(batch.shape) == (8, *size, 3) and all(torch.equal(batch[i], J.pil_pixels(f)) for i, f in enumerate(files))


@pytest.mark.parametrize("size", ((40, 3), (40, 4), (40, 5), (3, 40), (2, 2)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_narrow_4_2_0_planes_are_repeated_as_libjpeg_does(size):
    """libjpeg takes the "fancy" rule only for chroma planes of more than two columns."""
    f = J.pil_encode(J.content(*size).numpy(), quality=95, subsampling=2)
    assert torch.equal(J.statement_pixels(f), J.pil_pixels(f))


def test_golden_fixture():
    """Four files and PIL's pixels of them, stored: the statement does not follow the PIL of the machine."""
    from instag_amd import jpeg_decode as D
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 << 10
    for i in range(4):
        data = g[f"file{i}"].tobytes()
        assert torch.equal(D.jpeg_decode_torch([data])[0], torch.from_numpy(g[f"pixels{i}"]))
    subs = [D.parse_jpeg(g[f"file{i}"].tobytes()).subsampling for i in range(4)]
    assert subs == ["4:2:0", "4:4:4", "4:2:0", "4:2:0"]


def test_stages_are_public_and_take_a_batch_free_frame():
    from instag_amd import jpeg_decode as D, mjpeg as M
    frame, q = Hh.cases()["sinus33x47"]
    coef = M.coefficients_torch(frame[None], q, "4:2:0")[0]
    quant = torch.from_numpy(np.stack([t for t in M.quant_tables(q)] + [M.quant_tables(q)[1]]))
    data = Hh.statement("sinus33x47", "4:2:0")[0]
    assert torch.equal(D.parse_jpeg(data).quant, quant)
    assert torch.equal(D.pixels_torch(coef, quant, 33, 47, "4:2:0"), J.pil_pixels(data))
    with pytest.raises(ValueError):
        D.pixels_torch(coef[:-1], quant, 33, 47, "4:2:0")
    with pytest.raises(ValueError):
        D.jpeg_decode_torch([data, Hh.statement("one", "4:2:0")[0]])
    assert D.unstuff(b"\xff\x00\x00\xff\x00") == b"\xff\x00\xff" and D.unstuff(b"\x00\xff") == b"\x00\xff"


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("progressive", "restart", "4:2:2", "grayscale", "cut"))
def test_parse_refuses_and_names_the_cause(name):
    from instag_amd import jpeg_decode as D
    data, word = J.refused()[name]
    with pytest.raises(D.UnsupportedJpeg, match=word):
        D.parse_jpeg(data)
    assert issubclass(D.UnsupportedJpeg, ValueError)


def test_parse_refuses_more(tmp_path):
    from instag_amd import jpeg_decode as D
    data = Hh.statement("sinus24x40", "4:4:4")[0]
    sof = data.index(b"\xff\xc0")
    dqt = data.index(b"\xff\xdb")
    dht = data.index(b"\xff\xc4")
    sos = data.index(b"\xff\xda")
    def patched(at, value):
        b = bytearray(data)
        b[at] = value
        return bytes(b)
    for bad, word in ((b"not a jpeg", "SOI"), (patched(dqt + 4, 0x10), "Pq=1"), (patched(sof + 4, 12), "12-bit"),
                      (patched(sof + 9, 4), "4 components"), (patched(sos + 11, 1), "Ss, Se"),
                      (patched(sos + 4, 1), "more than one scan"), (patched(sof + 11, 0x21), "2x1"),
                      (patched(dqt + 4, 3), "missing table"), (patched(dht + 4, 0x03), "missing table"),
                      (data[:-2] + b"\xff\xda", "more than one scan"), (data[:-2] + b"\xff\xd0", "RST0"),
                      (data[:sos], "truncated"), (data[:dqt + 30], "truncated"),
                      (patched(sof + 5, 0x20), "4096")):
        with pytest.raises(D.UnsupportedJpeg, match=word):
            D.parse_jpeg(bad)
    # APPn and COM segments are skipped, a DHT segment may hold several tables
    com = data[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe1\x00\x04xy" + data[2:]
    assert torch.equal(D.jpeg_decode_torch([com])[0], J.pil_pixels(data))


def test_damaged_scans_raise_from_the_statement():
    from instag_amd import jpeg_decode as D
    data = J.pil_files((40, 56), 2)[3]
    cut = J.cut_scan(data)
    with pytest.raises(ValueError, match="ends before the last block"):
        D.coefficients_from_scan_torch(D.parse_jpeg(cut), cut)
    # a table of one code only: most bit patterns are in no table
    info = D.parse_jpeg(data)
    info.ac = (((0, 1) + (0,) * 14, (0,)),) * 3
    with pytest.raises(ValueError, match="in no Huffman table|ends before"):
        D.coefficients_from_scan_torch(info, data)
    # runs that walk past coefficient 63
    info = D.parse_jpeg(data)
    info.ac = (((1,) + (0,) * 15, (0xF1,)),) * 3
    with pytest.raises(ValueError, match="past 63|in no Huffman table"):
        D.coefficients_from_scan_torch(info, data)


# ---- the device's tables and the C entry points ---------------------------------------------------------------------------------
def test_decode_tables_give_every_code_its_symbol():
    from instag_amd import jpeg_decode as D, mjpeg as M
    for bits, vals in ((M.AC_LUMA_BITS, M.AC_LUMA_VALS), (M.DC_CHROMA_BITS, M.DC_VALS), D.parse_jpeg(J.pil_files((40, 56), 2)[1]).ac[0]):
        limit, base, v = D.decode_tables(bits, vals)
        assert limit.dtype == np.int32 and base.dtype == np.int32 and v.dtype == np.uint8 and v.size == 256
        assert (np.diff(limit) >= 0).all() and limit[-1] <= 65536
        for sym, (code, n) in M.huffman_codes(bits, vals).items():
            for tail in (0, (1 << (16 - n)) - 1):
                v16 = code << (16 - n) | tail
                length = 1 + int(np.argmax(v16 < limit))
                assert length == n and v[(v16 >> (16 - n)) + base[n - 1]] == sym


def test_header_and_argument_checks():
    from instag_amd import _cabi, _lib, jpeg_decode as D, mjpeg as M
    structs, protos, constants = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_jpeg_decode.h"))
    assert not structs and list(protos) == ["instag_jpeg_decode_workspace_bytes", "instag_jpeg_decode_coefficients",
                                            "instag_jpeg_decode_pixels", "instag_jpeg_decode"] == list(_lib._JPEG_DECODE_PROTOTYPES)
    assert constants == _lib.JPEG_DECODE
    assert constants["INSTAG_JPEG_DECODE_MAX_SIDE"] == M.MAX_SIDE and constants["INSTAG_JPEG_DECODE_MAX_BATCH"] == M.MAX_BATCH
    assert [constants[f"INSTAG_JPEG_DECODE_STATUS_{k}"] for k in ("CODE", "INDEX", "END")] == [1, 2, 3] == list(D.STATUS)
    assert constants["INSTAG_JPEG_DECODE_TABLE_BYTES"] == 384 == sum(a.nbytes for a in D.decode_tables(M.DC_LUMA_BITS, M.DC_VALS))
    L = _lib.lib()
    size = L.instag_jpeg_decode_workspace_bytes(2, 512, 512, 2, 100000, 1024)
    assert size > 2 * (6144 * 128 + 512 * 512 * 3 // 2 + 100000)
    for args in ((0, 8, 8, 1, 64, 64), (65, 8, 8, 1, 64, 64), (1, 0, 8, 1, 64, 64), (1, 8, 4097, 1, 64, 64), (1, 8, 8, 3, 64, 64),
                 (1, 8, 8, 1, 0, 64), (1, 8, 8, 1, (1 << 28) + 1, 64), (1, 8, 8, 1, 64, 32), (1, 8, 8, 1, 64, 96 + 16),
                 (1, 8, 8, 1, 64, 4128)):
        assert L.instag_jpeg_decode_workspace_bytes(*args) == 0 and L.instag_last_error()
    one = 8                                                                   # (a non-NULL pointer nothing reads)
    coef = lambda B=1, H=8, W=8, sub=2, cap=64, sb=64, scans=one, ws=one, size=1 << 30: L.instag_jpeg_decode_coefficients(
        scans, cap, one, one, B, H, W, sub, sb, one, one, ws, size, None)
    pixels = lambda B=1, H=8, W=8, sub=2, c=one, ws=one, size=1 << 30: L.instag_jpeg_decode_pixels(c, one, B, H, W, sub, one, ws, size, None)
    decode = lambda B=1, H=8, W=8, sub=2, cap=64, sb=64, q=one, ws=one, size=1 << 30: L.instag_jpeg_decode(
        one, cap, one, one, q, B, H, W, sub, sb, one, one, ws, size, None)
    for call in (coef, decode):
        for kw in (dict(B=0), dict(B=65), dict(H=0), dict(W=4097), dict(sub=3), dict(cap=0), dict(sb=48), dict(sb=8192), dict(ws=None)):
            assert call(**kw) == _lib.E_ARG, kw
        assert call(size=16) not in (0, _lib.E_ARG) and b"workspace too small" in L.instag_last_error()
    assert coef(scans=None) == decode(q=None) == pixels(c=None) == pixels(sub=0) == pixels(B=65) == _lib.E_ARG
    assert pixels(size=16) not in (0, _lib.E_ARG)


def test_decoder_arguments_and_the_cpu_device():
    """A CPU-device JpegDecoder runs the statement."""
    from instag_amd import jpeg_decode as D
    for kw in (dict(max_batch=0), dict(max_batch=65), dict(sub_bits=48), dict(sub_bits=32), dict(sub_bits=8192)):
        with pytest.raises(ValueError):
            D.JpegDecoder("cpu", **kw)
    dec = D.JpegDecoder("cpu", max_batch=2)
    files = list(J.pil_files((33, 47), 2)[:3])
    frames, status = dec.decode(files)
    assert frames.dtype == torch.uint8 and status.tolist() == [0, 0, 0]
    assert all(torch.equal(frames[i], J.pil_pixels(f)) for i, f in enumerate(files))
    assert torch.equal(dec.decode_checked(files), frames)
    coef = dec.coefficients(files)
    assert torch.equal(coef[1], J.statement_coefficients(files[1]))
    info = D.parse_jpeg(files[1])
    assert torch.equal(dec.pixels(coef[1:2], info.quant, 33, 47, "4:2:0")[0], J.pil_pixels(files[1]))
    with pytest.raises(ValueError, match="share"):
        dec.decode([files[0], J.pil_files((40, 56), 2)[0]])
    with pytest.raises(ValueError, match="share"):
        dec.decode([files[0], J.pil_files((33, 47), 0)[0]])
    with pytest.raises(D.UnsupportedJpeg):
        dec.decode([files[0], J.refused()["progressive"][0]])
    damaged = [files[0], J.cut_scan(files[1]), files[2]]
    frames, status = dec.decode(damaged)
    assert status.tolist() == [0, 3, 0] and torch.equal(frames[2], J.pil_pixels(files[2]))
    with pytest.raises(ValueError, match="file 1 .*ends before"):
        dec.decode_checked(damaged)


def test_frame_batches_and_read_avi_with_a_cpu_decoder(tmp_path):
    from instag_amd import convnet, jpeg_decode as D, mjpeg as M
    os.makedirs(tmp_path / "ori_imgs")
    frames = [J.content(40, 56, seed).numpy() for seed in range(6)]
    for i, f in enumerate(frames):
        (tmp_path / "ori_imgs" / f"{i}.jpg").write_bytes(J.pil_encode(f, quality=90, progressive=(i == 3), optimize=bool(i & 1)))
    dec = D.JpegDecoder("cpu")
    calls = []
    dec.decode_checked = lambda files, infos=None, f=dec.decode_checked: calls.append(len(files)) or f(files, infos)
    plain = list(convnet.frame_batches(str(tmp_path), 2))
    device = list(convnet.frame_batches(str(tmp_path), 2, decoder=dec))
    assert calls == [2, 2]                                                    # (the batch with the progressive file is PIL's)
    assert [a[0] for a in plain] == [b[0] for b in device] == [[0, 1], [2, 3], [4, 5]]
    assert all(torch.equal(a[1], b[1]) and a[2] == b[2] == (56, 40) for a, b in zip(plain, device))
    assert list(convnet.frame_batches(str(tmp_path), 4, resize=64, decoder=dec))[0][1].shape == (4, 64, 64, 3) and calls == [2, 2]
    path = str(tmp_path / "v.avi")
    with M.AviWriter(path, 40, 56) as w:
        for f in M.jpeg_encode_torch(torch.from_numpy(np.stack(frames[:3])), 90, "4:2:0"):
            w.append(f)
    a, b = M.read_avi(path), M.read_avi(path, decoder=dec)
    assert calls == [2, 2, 3] and torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] is None and b[2] is None
