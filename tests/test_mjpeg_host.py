"""The JPEG statement (instag_amd/mjpeg.py), the AVI container and the argument checks of the C entry points: no GPU.

The reference for the bytes is not the code under test: the tables are compared with the DHT / DQT segments PIL's
libjpeg writes, a scan is written out by hand from the Annex K codes, every file opens in PIL with warnings as errors,
and the decoded error is held against PIL's own encoder on the same tables."""
import ctypes as C
import io
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import mjpeg_helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _segments(data):
    """[(marker, body)] of a JPEG file up to SOS."""
    out, i = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[i] == 0xFF
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((data[i + 1], data[i + 4:i + 2 + n]))
        i += 2 + n
        if out[-1][0] == 0xDA:
            return out, i


# ---- tables and header ------------------------------------------------------------------------------------------------
def test_tables_are_annex_k_as_libjpeg_writes_them():
    from PIL import Image
    from instag_amd import mjpeg as M
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG", quality=50, subsampling=2)
    theirs, _ = _segments(buf.getvalue())
    ours, _ = _segments(M.header_bytes(16, 16, 50, "4:2:0"))
    pick = lambda segs, m: sorted(body for marker, body in segs if marker == m)
    assert pick(ours, 0xC4) == pick(theirs, 0xC4) and len(pick(ours, 0xC4)) == 4          # the four Huffman tables
    assert pick(ours, 0xDB) == pick(theirs, 0xDB) and len(pick(ours, 0xDB)) == 2          # quality 50: Annex K itself
    assert pick(ours, 0xC0) == pick(theirs, 0xC0) and pick(ours, 0xDA) == pick(theirs, 0xDA)
    assert [m for m, _ in ours] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]


def test_quality_rule_zigzag_and_dct_matrix():
    from instag_amd import mjpeg as M
    luma, chroma = M.quant_tables(50)
    assert tuple(luma) == M.LUMA_QUANT and tuple(chroma) == M.CHROMA_QUANT
    assert all((t == 1).all() for t in M.quant_tables(100))
    luma, chroma = M.quant_tables(90)                                          # s = 20
    assert luma[0] == 3 and luma[63] == 20 and chroma[0] == 3 and chroma[63] == 20 and luma[1] == 2
    luma, _ = M.quant_tables(10)                                               # s = 500
    assert luma[0] == 80 and luma[63] == 255
    assert M.quant_tables(1)[0].min() == 255 and M.quant_tables(49)[0][0] == (16 * 102 + 50) // 100
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            M.quant_tables(bad)
    assert sorted(M.ZIGZAG) == list(range(64)) and M.ZIGZAG[:6] == (0, 1, 8, 16, 9, 2) and M.ZIGZAG[-3:] == (55, 62, 63)
    c = np.array([[(np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * j + 1) * u * np.pi / 16) for j in range(8)]
                  for u in range(8)])
    assert (np.rint(16384 * c).astype(np.int64) == np.asarray(M.DCT_Q14)).all()
    codes = M.huffman_codes(M.AC_LUMA_BITS, M.AC_LUMA_VALS)
    assert codes[0x00] == (0b1010, 4) and codes[0xF0] == (0b11111111001, 11) and len(codes) == 162
    codes = M.huffman_codes(M.AC_CHROMA_BITS, M.AC_CHROMA_VALS)
    assert codes[0x00] == (0b00, 2) and codes[0xF0] == (0b1111111010, 10) and len(codes) == 162


@pytest.mark.parametrize("sub, sampling", [("4:2:0", 0x22), ("4:4:4", 0x11)])
def test_header_fields_and_max_bytes(sub, sampling):
    from instag_amd import mjpeg as M
    head = M.header_bytes(33, 47, 75, sub)
    segs, end = _segments(head)
    assert end == len(head) == 623
    sof = dict(segs)[0xC0]
    assert struct.unpack(">BHHB", sof[:6]) == (8, 33, 47, 3) and sof[6:] == bytes([1, sampling, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert dict(segs)[0xE0] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert dict(segs)[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    zz = list(M.ZIGZAG)
    dqt = [body for m, body in segs if m == 0xDB]
    assert [d[0] for d in dqt] == [0, 1] and [list(d[1:]) for d in dqt] == [list(t[zz]) for t in M.quant_tables(75)]
    # 33 x 47: 3 x 3 MCUs of 6 blocks at 4:2:0, 5 x 6 MCUs of 3 at 4:4:4
    nblk = 54 if sub == "4:2:0" else 90
    assert M.block_count(33, 47, sub) == nblk
    assert M.max_bytes(33, 47, sub) == 623 + 2 * ((nblk * 1660 + 7) // 8) + 2 == (23035 if sub == "4:2:0" else 37975)
    for H, W in ((0, 8), (8, 4097)):
        with pytest.raises(ValueError):
            M.header_bytes(H, W)
    with pytest.raises(ValueError):
        M.header_bytes(8, 8, 90, "4:2:2")


# ---- the scan ------------------------------------------------------------------------------------------------------------
def test_hand_computed_scan_of_a_grey_block():
    """8 x 8 of (200, 200, 200) at 4:4:4, quality 90.  Y = 200: the block minus 128 is 72 everywhere, its DC 8 x 72 = 576,
    over the table's 3: 192, category 8 -> luma DC code 111110, bits 11000000, then the luma EOB 1010.  Cb = Cr = 128:
    difference 0 -> chroma DC code 00, chroma EOB 00, twice.  26 bits, six ones fill the byte:
    11111011 00000010 10000000 00111111."""
    from instag_amd import mjpeg as M
    frame = torch.full((1, 8, 8, 3), 200, dtype=torch.uint8)
    coef = M.coefficients_torch(frame, 90, "4:4:4")
    assert coef.shape == (1, 3, 64) and coef.dtype == torch.int16
    assert coef[0, :, 0].tolist() == [192, 0, 0] and int(coef[0, :, 1:].abs().max()) == 0
    scan, counters = M.scan_torch(coef[0], "4:4:4")
    assert scan == bytes([0xFB, 0x02, 0x80, 0x3F])
    assert counters == dict(zrl=0, stuffed=0, dc_size=8, ac_size=0, bits=26)
    assert M.jpeg_encode_torch(frame, 90, "4:4:4") == [M.header_bytes(8, 8, 90, "4:4:4") + scan + b"\xff\xd9"]


def test_planes_rules():
    from instag_amd import mjpeg as M
    frame = torch.tensor([[[255, 0, 0], [0, 255, 0], [0, 0, 255]], [[255, 255, 255], [0, 0, 0], [10, 20, 30]]], dtype=torch.uint8)
    Y, Cb, Cr = M.planes_torch(frame[None], "4:4:4")
    assert Y.shape == (1, 8, 8) and Y[0, :2, :3].tolist() == [[76, 150, 29], [255, 0, 18]]
    assert Cb[0, 0, :3].tolist() == [85, 44, 255] and Cr[0, 0, :3].tolist() == [255, 21, 107]
    assert Cb[0, 1, :2].tolist() == [128, 128] and Cr[0, 1, :2].tolist() == [128, 128]
    assert torch.equal(Y[0, 2:], Y[0, 1:2].expand(6, 8)) and torch.equal(Y[0, :, 3:], Y[0, :, 2:3].expand(8, 5))      # edges repeat
    Y2, Cb2, _ = M.planes_torch(frame[None], "4:2:0")
    assert Y2.shape == (1, 16, 16) and Cb2.shape == (1, 8, 8)
    assert int(Cb2[0, 0, 0]) == (85 + 44 + 128 + 128 + 2) >> 2 and int(Cb2[0, 0, 1]) == (255 + 255 + Cb[0, 1, 2] * 2 + 2) >> 2
    with pytest.raises(ValueError):
        M.planes_torch(frame[None].float())


@pytest.mark.parametrize("sub", Hh.SUBS)
def test_crafted_cases_reach_their_branches(sub):
    from instag_amd import mjpeg as M
    count = lambda name: Hh.statement(name, sub)[2]
    c = count("constant128")                                   # DC difference 0 and EOB: 2 + 4 bits in luma, 2 + 2 in chroma
    assert (c["dc_size"], c["ac_size"], c["zrl"]) == (0, 0, 0) and c["bits"] == (4 * 6 + 2 * 4 if sub == "4:2:0" else 4 * 14)
    c = count("checkerboard")
    assert c["ac_size"] == 10 and c["stuffed"] == 80
    assert count("blocks8")["dc_size"] == 11
    coef = Hh.statement("thirds", sub)[1].to(torch.int64)
    comp = torch.from_numpy(M.block_components(32, 48, sub))
    for k in (1, 2):                                           # DC category 11 in both chroma components
        dc = coef[comp == k, 0]
        assert int((dc[1:] - dc[:-1]).abs().max()) >= 1024
    assert count("thirds")["dc_size"] == 11
    for name in ("sinus64x48", "noise40x24", "typical128"):
        assert count(name)["zrl"] >= 1, name
    assert count("noise32")["ac_size"] >= 8
    for name in Hh.CASES:
        frame, q = Hh.cases()[name]
        data, coef, c = Hh.statement(name, sub)
        assert coef.shape == (M.block_count(frame.shape[0], frame.shape[1], sub), 64)
        assert len(data) <= M.max_bytes(frame.shape[0], frame.shape[1], sub)
        scan = data[623:-2]
        assert len(scan) == (c["bits"] + 7) // 8 + c["stuffed"] and scan.count(b"\xff\x00") == c["stuffed"]
        assert b"\xff" not in scan.replace(b"\xff\x00", b"")


@pytest.mark.parametrize("sub", Hh.SUBS)
@pytest.mark.parametrize("name", Hh.CASES)
def test_statement_opens_in_pil_and_meets_the_bar(name, sub):
    """mse <= 1.10 mse_pil + 0.25, PIL's encoder having the same tables and subsampling."""
    frame, q = Hh.cases()[name]
    decoded = Hh.pil_decode(Hh.statement(name, sub)[0])
    assert decoded.shape == tuple(frame.shape) and decoded.dtype == np.uint8
    m, p = Hh.mse(decoded, frame), Hh.pil_mse(name, sub)
    print(f"\n[mjpeg parity] {name} {sub}: mse {m:.4f}, PIL {p:.4f}")
    assert Hh.within_bar(m, p), (m, p)


def test_recorded_parity_is_what_the_statement_gives():
    with open(os.path.join(ROOT, "profiles", "mjpeg_parity.json")) as f:
        rec = json.load(f)
    assert rec["bar"] == "mse <= 1.10 * mse_pil + 0.25"
    assert {(r["case"], r["subsampling"]) for r in rec["cases"]} == {(n, s) for n in Hh.CASES for s in Hh.SUBS}
    for r in rec["cases"]:
        assert r["bytes"] == len(Hh.statement(r["case"], r["subsampling"])[0])          # (no decoder in this one)
        assert Hh.within_bar(r["mse"], r["mse_pil"])


def test_cpu_encoder_runs_the_statement():
    from instag_amd import mjpeg as M
    frames = torch.stack([Hh.cases()[n][0] for n in ("blocks8", "thirds")])
    enc = M.JpegEncoder(32, 48, "cpu", quality=100, subsampling="4:4:4", capacity=740)
    want = M.jpeg_encode_torch(frames, 100, "4:4:4")
    assert [len(w) for w in want] == [723, 757] and enc.encode_bytes(frames) == want
    data, length = enc.encode(frames)
    assert length.tolist() == [723, 757] and enc.overflow.tolist() == [0, 1] and bytes(data[0, :723].numpy()) == want[0]
    assert torch.equal(enc.coefficients(frames), M.coefficients_torch(frames, 100, "4:4:4"))
    assert M.JpegEncoder(32, 48, "cpu").capacity == 32 * 48 * 3 // 2 + 623
    with pytest.raises(ValueError):
        enc.encode(frames[:, :16])
    with pytest.raises(ValueError):
        M.JpegEncoder(32, 48, "cpu", max_batch=0)


# ---- the container -------------------------------------------------------------------------------------------------------
def _jpegs(n):
    from instag_amd import mjpeg as M
    base = Hh.cases()["sinus24x40"][0]
    return M.jpeg_encode_torch(torch.stack([base.roll(3 * i, 1) for i in range(n)]), 90, "4:2:0")


@pytest.mark.parametrize("fps, n", [(25, 5), (30, 7), (29.97, 4)])
def test_avi_writer_walked_by_the_helper(tmp_path, fps, n):
    from instag_amd import mjpeg as M
    jpegs = _jpegs(n)
    rate, scale = (int(fps), 1) if fps == int(fps) else (29970, 1000)
    samples = (2 * n * 16000 * scale + rate) // (2 * rate)                    # round(n * 16000 / fps)
    audio = torch.from_numpy(np.random.default_rng(1).integers(-32768, 32768, samples).astype(np.float32) / 32768.0)
    path = str(tmp_path / "a.avi")
    with M.AviWriter(path, 24, 40, fps=fps, audio=audio) as w:
        for j in jpegs:
            w.append(j)
        assert w.frames == n
    got = Hh.walk_avi(path)
    assert got["video"] == jpegs and got["order"] == [b"00dc", b"01wb"] * n
    avih = got["avih"]
    assert avih[0] == 1000000 * scale // rate and avih[3] == 0x10 and avih[4] == n and avih[6] == 2
    assert (avih[8], avih[9]) == (40, 24) and avih[7] == max(map(len, jpegs))
    (kind, handler, v), (akind, _, a) = got["strh"]
    assert (kind, handler) == (b"vids", b"MJPG") and (v[4], v[5], v[7]) == (scale, rate, n)       # dwScale, dwRate, dwLength
    assert akind == b"auds" and (a[4], a[5], a[7], a[10]) == (1, 16000, samples, 2)
    assert struct.unpack("<IiiHH4sI", got["strf"][0][:24]) == (40, 40, 24, 1, 24, b"MJPG", 40 * 24 * 3)
    assert struct.unpack("<HHIIHH", got["strf"][1]) == (1, 1, 16000, 32000, 2, 16)
    pcm = np.frombuffer(b"".join(got["audio"]), "<i2")
    assert (pcm == np.rint(audio.numpy().astype(np.float64) * 32768)).all() and pcm.size == samples
    per_frame = [len(c) // 2 for c in got["audio"]]
    assert max(per_frame) - min(per_frame) <= 1 and len(per_frame) == n

    frames, got_fps, sound = M.read_avi(path)
    assert frames.shape == (n, 24, 40, 3) and frames.dtype == torch.uint8 and abs(got_fps - fps) < 1e-9
    assert all((frames[i].numpy() == Hh.pil_decode(jpegs[i])).all() for i in range(n))
    assert torch.equal(sound, audio)


def test_avi_without_audio_and_short_audio(tmp_path):
    from instag_amd import mjpeg as M
    jpegs = _jpegs(3)
    path = str(tmp_path / "v.avi")
    w = M.AviWriter(path, 24, 40)
    for j in jpegs:
        w.append(j)
    w.close()
    w.close()
    with pytest.raises(ValueError):
        w.append(jpegs[0])
    got = Hh.walk_avi(path)
    assert got["video"] == jpegs and got["audio"] == [] and got["avih"][6] == 1 and len(got["strh"]) == 1
    assert M.read_avi(path)[2] is None
    with M.AviWriter(path, 24, 40, audio=torch.zeros(1000)) as w:              # audio ends inside the second frame
        for j in jpegs:
            w.append(j)
    got = Hh.walk_avi(path)
    assert [len(c) // 2 for c in got["audio"]] == [640, 360] and got["order"] == [b"00dc", b"01wb"] * 2 + [b"00dc"]
    assert got["strh"][1][2][7] == 1000


def test_avi_oversize_guard(tmp_path, monkeypatch):
    from instag_amd import mjpeg as M
    jpegs = _jpegs(2)
    assert M.AVI_LIMIT == 2 ** 31 - 2 ** 20
    path = str(tmp_path / "big.avi")
    # headers up to and with "movi" 224, one chunk of 8 + len (even), idx1 8 + 16: exactly enough for one frame
    need = 224 + 8 + len(jpegs[0]) + (len(jpegs[0]) & 1) + 8 + 16
    monkeypatch.setattr(M, "AVI_LIMIT", need)
    with M.AviWriter(path, 24, 40) as w:
        w.append(jpegs[0])
        with pytest.raises(ValueError, match="OpenDML"):
            w.append(jpegs[1])
    assert os.path.getsize(path) == need and Hh.walk_avi(path)["video"] == jpegs[:1]
    monkeypatch.setattr(M, "AVI_LIMIT", need - 1)
    with M.AviWriter(path, 24, 40) as w:
        with pytest.raises(ValueError):
            w.append(jpegs[0])
    assert Hh.walk_avi(path)["video"] == []


def test_write_video_with_a_stub_renderer(tmp_path):
    from instag_amd import mjpeg as M
    base = Hh.cases()["sinus24x40"][0]

    class Renderer:
        as_uint8, calls = True, []

        def render_batch(self, frames, scenes=None):
            self.calls.append((list(frames), scenes))
            u8 = torch.stack([base.roll(3 * f, 1) for f in frames])
            return u8.permute(0, 3, 1, 2).float() / 255, u8

    r = Renderer()
    path = str(tmp_path / "w.avi")
    assert M.write_video(r, list(range(5)), path, group=2, fps=30, quality=75, subsampling="4:4:4") == 5
    assert [c[0] for c in r.calls] == [[0, 1], [2, 3], [4, 4]]                 # the last group padded, the padding not written
    want = M.jpeg_encode_torch(torch.stack([base.roll(3 * f, 1) for f in range(5)]), 75, "4:4:4")
    assert Hh.walk_avi(path)["video"] == want and M.read_avi(path)[1] == 30
    r.as_uint8 = False
    with pytest.raises(ValueError, match="as_uint8"):
        M.write_video(r, [0], path)
    with pytest.raises(ValueError):
        M.write_video(Renderer(), [0, 1], path, scene_backgrounds=[None])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_c_abi_of_the_mjpeg_header():
    from instag_amd import _cabi, _lib
    from instag_amd import mjpeg as M
    structs, protos, constants = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_mjpeg.h"))
    assert not structs and list(protos) == ["instag_mjpeg_workspace_bytes", "instag_mjpeg_coefficients",
                                            "instag_mjpeg_encode"] == list(_lib._MJPEG_PROTOTYPES)
    assert constants == _lib.MJPEG == {"INSTAG_MJPEG_MAX_SIDE": M.MAX_SIDE, "INSTAG_MJPEG_MAX_BATCH": M.MAX_BATCH,
                                       "INSTAG_MJPEG_BLOCK_BITS": M.BLOCK_BITS, "INSTAG_MJPEG_SCAN_BLOCKS": 1024,
                                       "INSTAG_MJPEG_SCAN_BYTES": 262144}
    assert not set(protos) & set(_lib.EXPORTED_SYMBOLS)                        # instag_hip.h's list is as it was
    L = _lib.lib()
    for name, (res, args) in protos.items():
        fn = getattr(L, name)                                                  # every declared name is exported
        assert fn.restype == res and list(fn.argtypes) == args
    assert L.instag_mjpeg_workspace_bytes(1, 512, 512, 2) > 6144 * 128 + 6144 * 1660 // 8
    for B, H, W, sub in ((0, 8, 8, 1), (65, 8, 8, 1), (1, 0, 8, 2), (1, 8, 4097, 2), (1, 8, 8, 3), (1, 8, 8, 0)):
        assert L.instag_mjpeg_workspace_bytes(B, H, W, sub) == 0 and b"sub 1 (4:4:4) or 2" in L.instag_last_error()
    one, big = C.c_void_p(256), 1 << 40
    enc = lambda B=1, H=8, W=8, q=90, sub=2, frames=one, head=one, hb=623, out=one, cap=4096, n=one, o=one, ws=one, size=big: \
        L.instag_mjpeg_encode(frames, B, H, W, q, sub, head, hb, out, cap, n, o, ws, size, None)
    for kw in (dict(H=0), dict(q=0), dict(q=101), dict(sub=3), dict(B=65), dict(B=0), dict(W=4097), dict(frames=None),
               dict(head=None), dict(out=None), dict(n=None), dict(o=None), dict(ws=None), dict(hb=0), dict(cap=0)):
        assert enc(**kw) == _lib.E_ARG, kw
    assert enc(size=16) == 3 and b"workspace too small" in L.instag_last_error()             # INSTAG_E_SPACE
    coef = lambda B=1, H=8, W=8, q=90, sub=2, frames=one, out=one: L.instag_mjpeg_coefficients(frames, B, H, W, q, sub, out, None)
    for kw in (dict(H=0), dict(q=0), dict(sub=3), dict(B=65), dict(frames=None), dict(out=None)):
        assert coef(**kw) == _lib.E_ARG, kw
