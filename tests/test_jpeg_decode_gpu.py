"""The JPEG decoder on the device (csrc/jpeg_decode.hip) against its integer statement (instag_amd/jpeg_decode.py) and PIL:
the same coefficients and the same pixels, byte for byte, whatever the subsequence length, the batch or the call; damaged
scans flagged and kept inside their own rows."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_decode_helpers as J
from tests import mjpeg_helpers as Hh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SUB_BITS = (None, 64)                                                        # the default, and the shortest


def _decoder(sub_bits=None, **kw):
    from instag_amd import jpeg_decode as D
    return D.JpegDecoder(DEV, sub_bits=sub_bits, **kw)


def _check(dec, files):
    """decode, coefficients and status of ``files`` against the statement and PIL."""
    frames, status = dec.decode(list(files))
    coef, cstatus = dec.coefficients(list(files), with_status=True)
    assert status.tolist() == cstatus.tolist() == [0] * len(files)
    assert frames.dtype == torch.uint8 and coef.dtype == torch.int16 and frames.device.type == coef.device.type == "cuda"
    frames, coef = frames.cpu(), coef.cpu()
    for i, f in enumerate(files):
        assert torch.equal(coef[i], J.statement_coefficients(f)), i
        assert torch.equal(frames[i], J.statement_pixels(f)) and torch.equal(frames[i], J.pil_pixels(f)), i


@pytest.mark.parametrize("sub_bits", SUB_BITS)
@pytest.mark.parametrize("sub", Hh.SUBS)
@pytest.mark.parametrize("name", Hh.CASES)
def test_encoder_files_equal_the_statement(name, sub, sub_bits):
    """Among them noise32 at quality 100 (blocks without EOB, many 0xFF bytes), noise40x24 at quality 50 (ZRL),
    checkerboard at quality 100 (the largest categories) and the 1 x 1 frame (a scan shorter than a subsequence); at 64
    bits a 32 x 32 frame is tens of subsequences, which synchronise over several rounds."""
    data, coef, counters = Hh.statement(name, sub)
    if name == "noise40x24":
        assert counters["zrl"] > 0
    if name == "noise32":
        assert counters["stuffed"] > 0 and counters["bits"] > 20 * 64
    if name == "one":
        assert counters["bits"] < 128                                          # (six blocks at 4:2:0: two subsequences of 64)
    _check(_decoder(sub_bits), [data])


@pytest.mark.parametrize("sub_bits", SUB_BITS)
@pytest.mark.parametrize("subsampling", sorted(J.PIL_SUBS))
@pytest.mark.parametrize("size", J.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pil_written_files_equal_the_statement(size, subsampling, sub_bits):
    """Eight files per call: quality 30 / 75 / 95 / 100, standard and optimised tables side by side in one batch."""
    _check(_decoder(sub_bits), J.pil_files(size, subsampling))


@pytest.mark.parametrize("sub_bits", (None, 64, 4096))
def test_more_subsequences_than_lanes_and_more_than_one_step_of_the_unstuff_scan(sub_bits):
    """256 x 320 of noise at quality 100, 4:4:4: 3840 blocks in a scan of some 330 KB: beyond the 256 KiB one step of the
    per-frame scan of dropped-byte counts takes, and at 64 bits per subsequence some 40,000 subsequences for 1024 lanes.
    Several of its 0xFF 0x00 pairs lie across the boundary of two 1 KiB counts."""
    from instag_amd import _lib
    from instag_amd import jpeg_decode as D, mjpeg as M
    data, want = J.big_noise()
    info = D.parse_jpeg(data)
    assert M.block_count(256, 320, "4:4:4") == 3840
    assert info.scan[1] > 262144 == _lib.JPEG_DECODE["INSTAG_JPEG_DECODE_SCAN_BYTES"]
    assert info.scan[1] * 8 // (sub_bits or D.SUB_BITS) > (_lib.JPEG_DECODE["INSTAG_JPEG_DECODE_LANES"] if sub_bits != 4096 else 512)
    scan = data[info.scan[0]:info.scan[0] + info.scan[1]]
    assert scan.count(b"\xff\x00") > 1000
    assert sum(scan[i] == 0xFF for i in range(1023, len(scan) - 1, 1024)) >= 3   # pairs split across two 1 KiB counts
    dec = _decoder(sub_bits)
    frames, status = dec.decode([data])
    assert status.tolist() == [0] and torch.equal(frames[0].cpu(), want)
    assert torch.equal(dec.coefficients([data])[0].cpu(), J.statement_coefficients(data))


def test_a_batch_with_max_batch_2_each_alone_and_again():
    """Five frames of one size, standard and optimised tables, scans from a few dozen bytes to kilobytes."""
    frames = [Hh._u8(np.full((40, 56, 3), 77.0)).numpy(), Hh._u8(Hh._noise(40, 56, 2)).numpy(), J.content(40, 56).numpy(),
              Hh._u8(Hh._sinus(40, 56, 1)).numpy(), Hh._u8(Hh._checker(40, 56)).numpy()]
    files = [J.pil_encode(f, quality=q, optimize=o) for f, q, o in zip(frames, (90, 100, 75, 95, 100), (False, True, False, True, True))]
    from instag_amd import jpeg_decode as D
    sizes = [D.parse_jpeg(f).scan[1] for f in files]
    assert max(sizes) > 8 * min(sizes)
    dec = _decoder(max_batch=2)
    batch, status = dec.decode(files)
    assert status.tolist() == [0] * 5
    for i, f in enumerate(files):
        alone, s = dec.decode([f])
        assert s.tolist() == [0] and torch.equal(alone[0], batch[i]) and torch.equal(alone[0].cpu(), J.pil_pixels(f))
    again, status = dec.decode(files)
    assert status.tolist() == [0] * 5 and torch.equal(again, batch)
    assert torch.equal(_decoder(64, max_batch=3).decode(files)[0], batch)


@pytest.mark.parametrize("sub", Hh.SUBS)
def test_coefficients_of_the_encoder_s_device_output(sub):
    """JpegEncoder's bytes never leave the device: the rows behind the header are the scans."""
    from instag_amd import jpeg_decode as D, mjpeg as M
    frames = torch.stack([Hh._u8(Hh._sinus(40, 56, 1)), Hh._u8(Hh._noise(40, 56, 2)), Hh._u8(Hh._typical(40, 56, 4))])
    enc = M.JpegEncoder(40, 56, DEV, quality=90, subsampling=sub)
    data, length = enc.encode(frames.to(DEV), enc.max_bytes)
    assert enc.overflow.tolist() == [0, 0, 0]
    head = len(enc.header)
    info = D.parse_jpeg(M.jpeg_encode_torch(frames[:1], 90, sub)[0])             # (the tables: the header's, for every frame)
    dec = _decoder()
    _, _, huffman, _ = dec.pack([b""] * 3, [D.JpegInfo(40, 56, sub, info.quant, info.dc, info.ac, (0, 0))] * 3)
    scans = data[:, head:].contiguous()
    coef, status = dec.coefficients_of(scans, (length - head - 2).to(torch.int32), huffman.to(DEV), 40, 56, sub, with_status=True)
    assert status.tolist() == [0, 0, 0]
    assert torch.equal(coef.cpu(), M.coefficients_torch(frames, 90, sub))
    assert torch.equal(coef, enc.coefficients(frames.to(DEV)))


@pytest.mark.parametrize("sub", Hh.SUBS)
def test_pixels_of_given_coefficients(sub):
    from instag_amd import jpeg_decode as D, mjpeg as M
    frames = torch.stack([Hh._u8(Hh._sinus(33, 47, 3)), Hh._u8(Hh._noise(33, 47, 2)), Hh._u8(Hh._checker(33, 47))])
    files = M.jpeg_encode_torch(frames, 75, sub)
    coef = M.coefficients_torch(frames, 75, sub)
    quant = D.parse_jpeg(files[0]).quant
    got = _decoder(max_batch=2).pixels(coef.to(DEV), quant, 33, 47, sub)
    assert got.dtype == torch.uint8 and all(torch.equal(got[i].cpu(), J.pil_pixels(f)) for i, f in enumerate(files))
    with pytest.raises(ValueError):
        _decoder().pixels(coef.to(DEV)[:, :-1], quant, 33, 47, sub)


def _canaried(dec, files, scans, nbytes, huffman, quant, H, W, sub):
    """decode and coefficients into tensors with 64 canary bytes behind them -> (frames, coef, status)."""
    from instag_amd import mjpeg as M
    B, nblk = len(files), M.block_count(H, W, sub)
    flat = torch.full((B * H * W * 3 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    cflat = torch.full((B * nblk * 64 + 32,), 0x5A5A, dtype=torch.int16, device=DEV)
    status = torch.full((B + 16,), -7, dtype=torch.int32, device=DEV)
    frames, coef = flat[:B * H * W * 3].view(B, H, W, 3), cflat[:B * nblk * 64].view(B, nblk, 64)
    dec.decode_into(scans, nbytes, huffman, quant, sub, frames, status[:B])
    dec.coefficients_of(scans, nbytes, huffman, H, W, sub, coef=coef, status=status[:B])
    torch.cuda.synchronize()
    assert bool((flat[B * H * W * 3:] == 0xA5).all()) and bool((cflat[B * nblk * 64:] == 0x5A5A).all())
    assert bool((status[B:] == -7).all())
    return frames, coef, status[:B]


@pytest.mark.parametrize("sub_bits", SUB_BITS)
def test_damaged_scans_are_flagged_and_stay_in_their_rows(sub_bits):
    from instag_amd import jpeg_decode as D
    good = [J.pil_encode(J.content(40, 56, s).numpy(), quality=95, optimize=bool(s & 1)) for s in (1, 2, 3)]
    dec = _decoder(sub_bits)
    # the middle scan cut to half its bytes
    files = [good[0], J.cut_scan(good[1]), good[2]]
    infos = [D.parse_jpeg(f) for f in files]
    assert infos[1].scan[1] <= D.parse_jpeg(good[1]).scan[1] // 2
    packed = [t.to(DEV) for t in dec.pack(files, infos)]
    frames, coef, status = _canaried(dec, files, *packed, 40, 56, "4:2:0")
    assert status.tolist() == [0, 3, 0]
    for b in (0, 2):
        assert torch.equal(frames[b].cpu(), J.pil_pixels(files[b])) and torch.equal(coef[b].cpu(), J.statement_coefficients(files[b]))
    with pytest.raises(ValueError, match="file 1 "):
        dec.decode_checked(files)
    frames, status = dec.decode(files)
    assert status.tolist() == [0, 3, 0] and torch.equal(frames[2].cpu(), J.pil_pixels(files[2]))
    # one byte of the middle scan inverted, on the packed tensors: a status or a decoded frame, the neighbours exact
    infos = [D.parse_jpeg(f) for f in good]
    scans, nbytes, huffman, quant = dec.pack(good, infos)
    scans[1, infos[1].scan[1] // 2] ^= 0xFF
    frames, coef, status = _canaried(dec, good, scans.to(DEV), nbytes.to(DEV), huffman.to(DEV), quant.to(DEV), 40, 56, "4:2:0")
    s = status.tolist()
    assert s[0] == s[2] == 0 and s[1] in (0, 1, 2, 3)
    for b in (0, 2):
        assert torch.equal(frames[b].cpu(), J.pil_pixels(good[b])) and torch.equal(coef[b].cpu(), J.statement_coefficients(good[b]))
    # a scan length beyond the row, and a negative one, are clamped on the device
    bad = nbytes.clone()
    bad[0], bad[2] = 1 << 30, -5
    _, _, status = _canaried(dec, good, scans.to(DEV), bad.to(DEV), huffman.to(DEV), quant.to(DEV), 40, 56, "4:2:0")
    assert status.tolist()[2] == 3


def test_captured_decode_replays_on_new_scans():
    """Nothing but launches on the caller's stream: a captured ``decode_into`` decodes whatever its inputs hold at replay."""
    from instag_amd import _lib
    from instag_amd import jpeg_decode as D
    first = [J.pil_encode(J.content(40, 56, s).numpy(), quality=90) for s in (1, 2)]
    second = [J.pil_encode(Hh._u8(Hh._noise(40, 56, 5)).numpy(), quality=100, optimize=True),
              J.pil_encode(Hh._u8(Hh._sinus(40, 56, 2)).numpy(), quality=60, optimize=True)]
    dec = _decoder(max_batch=2)
    infos = {id(fs): [D.parse_jpeg(f) for f in fs] for fs in (first, second)}
    cap = max(i.scan[1] for v in infos.values() for i in v)
    packed = {id(fs): dec.pack(fs, infos[id(fs)], capacity=cap) for fs in (first, second)}
    static = [t.to(DEV) for t in packed[id(first)]]
    frames = torch.zeros(2, 40, 56, 3, dtype=torch.uint8, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    dec.decode_into(*static, "4:2:0", frames, status)                        # (the workspace exists from here on)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _lib.graph_capture(graph):
        dec.decode_into(*static, "4:2:0", frames, status)
    for fs in (second, first):
        for dst, src in zip(static, packed[id(fs)]):
            dst.copy_(src)
        frames.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert status.tolist() == [0, 0]
        assert all(torch.equal(frames[i].cpu(), J.pil_pixels(f)) for i, f in enumerate(fs))


def test_frame_batches_and_read_avi_with_a_decoder(tmp_path):
    from instag_amd import convnet, mjpeg as M
    os.makedirs(tmp_path / "ori_imgs")
    frames = [J.content(40, 56, seed).numpy() for seed in range(6)]
    for i, f in enumerate(frames):
        (tmp_path / "ori_imgs" / f"{i}.jpg").write_bytes(J.pil_encode(f, quality=90, progressive=(i == 3), optimize=bool(i & 1)))
    dec = _decoder()
    plain = list(convnet.frame_batches(str(tmp_path), 2))
    device = list(convnet.frame_batches(str(tmp_path), 2, decoder=dec))
    assert [b[1].device.type for b in device] == ["cuda", "cpu", "cuda"]    # (the batch with the progressive file is PIL's)
    assert [a[0] for a in plain] == [b[0] for b in device]
    assert all(torch.equal(a[1], b[1].cpu()) and a[2] == b[2] for a, b in zip(plain, device))
    path = str(tmp_path / "v.avi")
    with M.VideoWriter(path, 40, 56, DEV) as w:
        w.append(torch.from_numpy(np.stack(frames)).to(DEV))
    a, b = M.read_avi(path), M.read_avi(path, decoder=dec)
    assert b[0].device.type == "cuda" and torch.equal(a[0], b[0].cpu()) and a[1] == b[1] and tuple(a[0].shape) == (6, 40, 56, 3)
