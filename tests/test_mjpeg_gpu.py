"""The JPEG encoder on the device (csrc/mjpeg.hip) against its integer statement (instag_amd/mjpeg.py): the same
coefficients and the same bytes, whatever the batch, the capacity or the call; and the video around it."""
import numpy as np
import pytest
import torch

from tests import mjpeg_helpers as Hh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _encoder(name, sub, **kw):
    from instag_amd import mjpeg as M
    frame, q = Hh.cases()[name]
    return M.JpegEncoder(frame.shape[0], frame.shape[1], DEV, quality=q, subsampling=sub, **kw), frame.to(DEV)[None]


@pytest.mark.parametrize("sub", Hh.SUBS)
@pytest.mark.parametrize("name", Hh.CASES)
def test_coefficients_and_bytes_equal_the_statement(name, sub):
    enc, frame = _encoder(name, sub)
    want_bytes, want_coef, _ = Hh.statement(name, sub)
    got = enc.coefficients(frame)
    assert got.dtype == torch.int16 and torch.equal(got[0].cpu(), want_coef)
    got_bytes = enc.encode_bytes(frame)
    assert len(got_bytes) == 1 and len(got_bytes[0]) == len(want_bytes) and got_bytes[0] == want_bytes
    # the bar of the statement holds on the device's bytes
    m = Hh.mse(Hh.pil_decode(got_bytes[0]), Hh.cases()[name][0])
    assert Hh.within_bar(m, Hh.pil_mse(name, sub)), (m, Hh.pil_mse(name, sub))


def test_more_than_one_chunk_of_both_scans():
    """256 x 320 of noise at quality 100, 4:4:4: 32 x 40 x 3 = 3840 blocks, beyond the 1024 blocks one step of the
    per-frame scan of bit lengths takes, and a scan of some 330 KB, beyond the 256 KiB (256 counts of 1024 bytes) one
    step of the per-frame scan of 0xFF counts takes."""
    from instag_amd import _lib
    from instag_amd import mjpeg as M
    frame = Hh._u8(Hh._noise(256, 320, 11))[None]
    want = M.jpeg_encode_torch(frame, 100, "4:4:4")[0]
    assert M.block_count(256, 320, "4:4:4") == 3840 > 1024 == _lib.MJPEG["INSTAG_MJPEG_SCAN_BLOCKS"]
    assert len(want) - 623 > 262144 and _lib.MJPEG["INSTAG_MJPEG_SCAN_BYTES"] == 262144
    enc = M.JpegEncoder(256, 320, DEV, quality=100, subsampling="4:4:4")
    assert len(want) > enc.capacity                                           # (and so through the second pass)
    got = enc.encode_bytes(frame.to(DEV))[0]
    assert len(got) == len(want) and got == want
    assert Hh.pil_decode(got).shape == (256, 320, 3)


@pytest.mark.parametrize("sub", Hh.SUBS)
def test_a_frame_alone_in_a_batch_and_again(sub):
    from instag_amd import mjpeg as M
    frames = torch.stack([Hh._u8(Hh._sinus(40, 56, 1)), Hh._u8(Hh._noise(40, 56, 2)), Hh._u8(np.full((40, 56, 3), 77.0)),
                          Hh._u8(Hh._typical(40, 56, 4)), Hh._u8(Hh._checker(40, 56))])
    want = M.jpeg_encode_torch(frames, 90, sub)
    enc = M.JpegEncoder(40, 56, DEV, quality=90, subsampling=sub, max_batch=2)
    dev = frames.to(DEV)
    batch = enc.encode_bytes(dev)
    assert batch == want
    assert [enc.encode_bytes(dev[i:i + 1])[0] for i in range(5)] == want
    assert enc.encode_bytes(dev) == want
    assert torch.equal(enc.coefficients(dev).cpu(), M.coefficients_torch(frames, 90, sub))


def test_overflow_flag_length_and_canaries():
    from instag_amd import mjpeg as M
    small, large = Hh._u8(np.full((32, 48, 3), 90.0)), Hh._u8(Hh._noise(32, 48, 9))
    frames = torch.stack([small, large, small])
    want = M.jpeg_encode_torch(frames, 90, "4:2:0")
    cap = (len(want[0]) + len(want[1])) // 2
    assert len(want[0]) < cap < len(want[1])
    enc = M.JpegEncoder(32, 48, DEV, capacity=cap)
    data, length = enc.encode(frames.to(DEV))
    assert tuple(data.shape) == (3, cap) and length.tolist() == [len(w) for w in want] and enc.overflow.tolist() == [0, 1, 0]
    for b in (0, 2):
        assert bytes(data[b, :len(want[b])].cpu().numpy()) == want[b]
    # rows of a wider tensor: 64 canary bytes behind each row stay
    wide = torch.full((3, cap + 64), 0xA5, dtype=torch.uint8, device=DEV)
    n, over = torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros(3, dtype=torch.uint8, device=DEV)
    enc.encode_into(frames.to(DEV), wide[:, :cap], n, over)
    assert n.tolist() == [len(w) for w in want] and over.tolist() == [0, 1, 0]
    assert bool((wide[:, cap:] == 0xA5).all())
    assert bytes(wide[0, :len(want[0])].cpu().numpy()) == want[0] and bool((wide[0, len(want[0]):] == 0xA5).all())
    # a contiguous batch with the canaries behind the whole of it
    flat = torch.full((3 * cap + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    enc.encode_into(frames.to(DEV), flat[:3 * cap].view(3, cap), n, over)
    assert over.tolist() == [0, 1, 0] and bool((flat[3 * cap:] == 0x5A).all())
    assert bytes(flat[2 * cap:2 * cap + len(want[2])].cpu().numpy()) == want[2]
    # encode_bytes goes through its second pass
    assert enc.encode_bytes(frames.to(DEV)) == want


def test_captured_encode_replays_on_new_frames():
    """Nothing but launches on the caller's stream: a captured ``encode_into`` codes whatever its input holds at replay."""
    from instag_amd import _lib
    from instag_amd import mjpeg as M
    first = torch.stack([Hh._u8(Hh._sinus(40, 56, 1)), Hh._u8(Hh._checker(40, 56))])
    second = torch.stack([Hh._u8(Hh._noise(40, 56, 2)), Hh._u8(Hh._typical(40, 56, 4))])
    enc = M.JpegEncoder(40, 56, DEV, max_batch=2)
    static = first.to(DEV)
    data = torch.zeros(2, enc.capacity, dtype=torch.uint8, device=DEV)
    n, over = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.uint8, device=DEV)
    enc.encode_into(static, data, n, over)                                    # (the workspace exists from here on)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _lib.graph_capture(graph):
        enc.encode_into(static, data, n, over)
    for frames in (second, first):
        static.copy_(frames.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = M.jpeg_encode_torch(frames, 90, "4:2:0")
        assert n.tolist() == [len(w) for w in want] and over.tolist() == [0, 0]
        assert [bytes(data[b, :len(want[b])].cpu().numpy()) for b in range(2)] == want


def test_video_writer_with_audio(tmp_path):
    from instag_amd import mjpeg as M
    frames = torch.stack([Hh._u8(Hh._typical(48, 64, s)) for s in range(5)])
    audio = torch.from_numpy(np.random.default_rng(2).integers(-32768, 32768, 3200).astype(np.float32) / 32768.0)   # 0.2 s
    path = str(tmp_path / "v.avi")
    with M.VideoWriter(path, 48, 64, DEV, audio=audio, max_batch=2) as w:
        w.append(frames[:3].to(DEV))
        w.append(frames[3].to(DEV))
        w.append(frames[4:].to(DEV))
        assert w.frames == 5
    want = M.jpeg_encode_torch(frames, 90, "4:2:0")
    got = Hh.walk_avi(path)
    assert got["video"] == want and [len(c) for c in got["audio"]] == [1280] * 5
    assert (np.frombuffer(b"".join(got["audio"]), "<i2") == np.rint(audio.numpy() * 32768.0)).all()
    decoded, fps, sound = M.read_avi(path)
    assert fps == 25 and torch.equal(sound, audio) and tuple(decoded.shape) == (5, 48, 64, 3)
    for i in range(5):
        assert (decoded[i].numpy() == Hh.pil_decode(want[i])).all()


@pytest.fixture(scope="module")
def head():
    """The small synthetic fuse scene of test_metrics_gpu.py: 64 x 64, 5 frames."""
    from tests.test_stages_gpu import _frames, _mouth_setup
    pc, net, pcm, netm = _mouth_setup(DEV, n_face=3000, n_mouth=800, seed=21)
    with torch.no_grad():
        for mod in (net.sigma_net, netm.sigma_net, pc.neural_motion_grid.sigma_net, pc.neural_motion_grid.align_net,
                    pcm.neural_motion_grid.sigma_net, pcm.neural_motion_grid.align_net):
            mod.net[-1].weight.mul_(30.0)
    frames = _frames(64, 5, DEV, background=True)
    return dict(models=(pc, net, pcm, netm), frames=frames, bg=torch.zeros(3, device=DEV),
                scenes=[f.talking_dict["background"] for f in frames])


def test_write_video_of_a_rendered_head(head, tmp_path):
    import io
    from PIL import Image
    from instag_amd import mjpeg as M
    from instag_amd.infer import FuseRenderer
    pc, net, pcm, netm = head["models"]
    r = FuseRenderer(pc, net, pcm, netm, head["bg"], as_uint8=True)
    path = str(tmp_path / "head.avi")
    assert M.write_video(r, head["frames"], path, head["scenes"], group=2) == 5        # 2 + 2 + (1 and one padded)
    _, u8 = r.render_batch(head["frames"], head["scenes"])
    decoded, fps, sound = M.read_avi(path)
    assert tuple(decoded.shape) == (5, 64, 64, 3) and fps == 25 and sound is None
    assert Hh.walk_avi(path)["video"] == M.jpeg_encode_torch(u8.cpu(), 90, "4:2:0")
    tables = [[int(v) for v in t] for t in M.quant_tables(90)]
    for i in range(5):
        src = u8[i].cpu()
        buf = io.BytesIO()
        Image.fromarray(src.numpy()).save(buf, "JPEG", qtables=tables, subsampling=2)
        m, p = Hh.mse(decoded[i], src), Hh.mse(Hh.pil_decode(buf.getvalue()), src)
        print(f"\n[write_video] frame {i}: mse {m:.4f}, PIL {p:.4f}")
        assert Hh.within_bar(m, p), (i, m, p)
    with pytest.raises(ValueError):
        M.write_video(FuseRenderer(pc, net, pcm, netm, head["bg"]), head["frames"], path)
