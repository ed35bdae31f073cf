"""Host tests of the face detector's statement (instag_amd/face_detect.py): the network against golden G20 and the second
``nn.Module`` statement, the map sizes, the loader, hand-computed cases of the tail against ``post_torch`` and the loop
statement, the wiring into ``landmarks_identity`` and ``Evaluator``, and the C ABI of include/instag_face_detect.h.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import face_detect_helpers as H


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(f"{golden_dir}/g20_face_detect.npz")


@pytest.fixture(scope="module")
def weights():
    return H.weights()


# ---- the network ---------------------------------------------------------------------------------------------------------
def test_s3fd_torch_matches_g20_and_the_module(g20, weights):
    from instag_amd import face_detect as FD
    frame = torch.from_numpy(g20["frame"])[None]
    with torch.no_grad():
        got = FD.s3fd_torch(weights, FD.normalise_torch(frame, torch.float64))
        again = H.module(weights)(H.bgr_input(frame.numpy()))
    assert len(got) == 12
    for i, (m, a) in enumerate(zip(got, again)):
        want = g20[f"map{i}"]
        scale = np.abs(want).max()
        assert m.dtype == torch.float64 and tuple(m.shape[1:]) == want.shape
        assert np.abs(m[0].numpy() - want).max() <= 1e-12 * scale, i
        assert float((m - a).abs().max()) <= 1e-12 * scale, i
    t = H.tail_loops(got)
    assert np.array_equal(t["index"], g20["cand_index"]) and np.array_equal(t["det_index"], g20["det_index"])
    boxes, count, overflow, found = FD.post_torch(got, H.G20_H, H.G20_W, details=True)
    n = len(g20["det_index"])
    assert int(count[0]) == n >= 2 and not bool(overflow[0]) and np.array_equal(found[0].numpy(), g20["det_index"])
    assert H.within_one_ulp(boxes[0, :min(n, 16), :4].numpy(), g20["det_boxes"][:16])
    assert np.array_equal(boxes[0, :min(n, 16), 4].numpy(), g20["det_score"][:16])
    cand = FD.candidates_torch(got, H.G20_H, H.G20_W)[0]
    assert np.array_equal(cand[0].numpy(), g20["cand_index"]) and np.array_equal(cand[1].numpy(), g20["cand_score"])
    assert np.abs(cand[2].numpy() - g20["cand_boxes"]).max() < 1e-9


def test_table_keys_and_macs(g20, weights):
    from instag_amd import face_detect as FD
    layout = json.loads(bytes(g20["layout"]).decode())
    sd = weights.state_dict()
    assert sorted([k, list(v.shape)] for k, v in sd.items()) == layout and len(sd) == 65
    assert len(FD.TRUNK) == 19 and len(FD.HEADS) == 12 and len(FD.LAYERS) == 31
    assert FD.LAYERS[FD.INDEX["conv3_3_norm_mbox_conf"]][4] == 4 and FD.LAYERS[FD.INDEX["fc7_mbox_conf"]][4] == 2
    # by hand at 64 x 64: conv1 (27 + 576) 64 on 64^2 positions, ..., the heads on 16^2, 8^2, 4^2, 6^2, 3^2, 2^2
    trunk = (3 * 64 + 64 * 64) * 9 * 4096 + (64 * 128 + 128 * 128) * 9 * 1024 + (128 * 256 + 2 * 256 * 256) * 9 * 256 \
        + (256 * 512 + 2 * 512 * 512) * 9 * 64 + 3 * 512 * 512 * 9 * 16 + 512 * 1024 * 9 * 36 + 1024 * 1024 * 36 \
        + 1024 * 256 * 36 + 256 * 512 * 9 * 9 + 512 * 128 * 9 + 128 * 256 * 9 * 4
    heads = 256 * 8 * 9 * 256 + 512 * 6 * 9 * 64 + 512 * 6 * 9 * 16 + 1024 * 6 * 9 * 36 + 512 * 6 * 9 * 9 + 256 * 6 * 9 * 4
    assert FD.macs_per_frame(64, 64) == trunk + heads


@pytest.mark.parametrize("Hh,Ww", [(64, 64), (64, 96), (96, 64)])
def test_map_sizes(weights, Hh, Ww):
    """The + 4 of fc6 and the odd side into a stride-2 convolution: 64 -> 2 + 4 = 6 -> 3 -> 2, 96 -> 3 + 4 = 7 -> 4 -> 2."""
    from instag_amd import face_detect as FD
    side = {64: (16, 8, 4, 6, 3, 2), 96: (24, 12, 6, 7, 4, 2)}
    assert FD.level_sides(Hh) == side[Hh] and tuple(H.level_sides(Ww)) == side[Ww]
    with torch.no_grad():
        maps = FD.s3fd_torch(weights, FD.normalise_torch(H.seeded_frames(1, Hh, Ww, seed=1)))
    for l in range(6):
        assert tuple(maps[2 * l].shape) == (1, 4 if l == 0 else 2, side[Hh][l], side[Ww][l])
        assert tuple(maps[2 * l + 1].shape) == (1, 4, side[Hh][l], side[Ww][l])
    assert FD.check_maps(maps, Hh, Ww) == 1
    with pytest.raises(ValueError, match=r"maps\[6\]"):
        FD.check_maps(maps[:6] + [maps[6][:, :, :-1]] + maps[7:], Hh, Ww)
    with pytest.raises(ValueError, match="multiples of 32"):
        FD.s3fd_torch(weights, torch.zeros(1, 3, 80, 64))


def test_normalise_is_bgr_minus_the_mean():
    from instag_amd import face_detect as FD
    f = torch.tensor([[[[10, 20, 30]]]], dtype=torch.uint8)
    assert FD.normalise_torch(f, torch.float64).flatten().tolist() == [30 - 104.0, 20 - 117.0, 10 - 123.0]


def test_loader_round_trip_and_errors(tmp_path, weights):
    from instag_amd.face_detect import S3FDWeights
    sd = weights.state_dict()
    path = str(tmp_path / "s3fd.pth")
    torch.save({"module." + k: v for k, v in sd.items()}, path)
    back = S3FDWeights.load(path).state_dict()
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    for key in ("conv4_2.bias", "conv5_3_norm.weight", "conv6_2_mbox_loc.weight"):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            S3FDWeights.from_state_dict({k: v for k, v in sd.items() if k != key})
    with pytest.raises(ValueError, match="fc6 weight"):
        S3FDWeights.from_state_dict({**sd, "fc6.weight": sd["fc6.weight"][:, :, :1, :1]})
    with pytest.raises(ValueError, match="conv3_3_norm weight"):
        S3FDWeights.from_state_dict({**sd, "conv3_3_norm.weight": torch.ones(255)})
    with pytest.raises(ValueError, match="conv3_3_norm_mbox_conf bias"):
        S3FDWeights.from_state_dict({**sd, "conv3_3_norm_mbox_conf.bias": torch.ones(2)})
    shifted = S3FDWeights.random(H.SEED, conf_shift=1.5).state_dict()
    assert torch.equal(shifted["conv3_3_norm_mbox_conf.bias"] - sd["conv3_3_norm_mbox_conf.bias"],
                       torch.tensor([1.5, 1.5, 1.5, 0.0]))
    assert torch.equal(shifted["fc7_mbox_conf.bias"] - sd["fc7_mbox_conf.bias"], torch.tensor([1.5, 0.0]))
    assert torch.equal(shifted["fc7_mbox_loc.bias"], sd["fc7_mbox_loc.bias"])


# ---- the tail on crafted logits ------------------------------------------------------------------------------------------
CASES = H.tail_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_tail_on_hand_computed_cases(name):
    from instag_amd import face_detect as FD
    maps, Hh, Ww, want = CASES[name]
    boxes, count, overflow, found = FD.post_torch(maps, Hh, Ww, details=True)
    assert boxes.dtype == torch.float32 and count.dtype == torch.int32 and overflow.dtype == torch.bool
    assert overflow.tolist() == want["overflow"]
    if want["count"] is not None:
        assert count.tolist() == want["count"] and [f.tolist() for f in found] == want["index"]
    for b in range(len(want["overflow"])):
        t = H.tail_loops(maps, b)                                               # the loop statement says the same
        n = len(t["det_index"])
        assert int(count[b]) == n and np.array_equal(found[b].numpy(), t["det_index"]) and t["overflow"] == want["overflow"][b]
        assert H.within_one_ulp(boxes[b, :min(n, 16), :4].numpy(), t["det_boxes"][:16])
        assert np.array_equal(boxes[b, :min(n, 16), 4].numpy(), t["det_score"][:16])
        assert bool(torch.isnan(boxes[b, min(n, 16):]).all())
        if name.startswith("cap"):
            assert len(t["index"]) == 4096 and int(t["index"].max()) == 4095 and n > 16
    if "boxes" in want:
        assert H.within_one_ulp(boxes[0, 0, :4].numpy(), want["boxes"]) and boxes[0, 0, 4] == np.float32(want["score"])
    if name == "many":
        assert want["count"] == [20] and bool((boxes[0, :-1, 4] > boxes[0, 1:, 4]).all())


def test_the_0_05_threshold_is_float32():
    """p exactly float32(0.05) and the float32 below it are no candidates, the float32 above it is one."""
    from instag_amd import face_detect as FD
    for target, n in ((H.F05, 0), (np.nextafter(H.F05, np.float32(0)), 0), (np.nextafter(H.F05, np.float32(1)), 1)):
        maps = H.blank_maps(1, 64, 64)
        H.put_pair(maps, 0, 2, 1, 2, *H.logits_for(target))
        idx, sc, _, over = FD.candidates_torch(maps, 64, 64)[0]
        assert idx.tolist() == [320 + 6][:n] and not over and len(H.tail_loops(maps)["index"]) == n
        assert FD.scores_torch(maps)[2][0, 1, 2] == np.float32(target)
        if n:
            assert sc[0] == np.float32(target)


def test_first_and_last():
    from instag_amd import face_detect as FD
    maps, Hh, Ww, _ = CASES["overlap"]
    boxes, count, _ = FD.post_torch(maps, Hh, Ww)
    first, last = FD.pick(boxes, count), FD.pick(boxes, count, last=True)
    assert torch.equal(first, boxes[:, 0, :4]) and torch.equal(last[0], boxes[0, 0, :4]) and torch.equal(last[1], boxes[1, 1, :4])
    boxes, count, _ = FD.post_torch(CASES["empty"][0], 64, 64)
    assert bool(torch.isnan(FD.pick(boxes, count)).all()) and bool(torch.isnan(FD.pick(boxes, count, last=True)).all())
    boxes, count, _ = FD.post_torch(CASES["many"][0], 64, 64)
    assert torch.equal(FD.pick(boxes, count, last=True)[0], boxes[0, 15, :4])   # the last of those returned


def test_cpu_device_runs_the_statement(weights):
    from instag_amd import face_detect as FD
    frames = H.seeded_frames(2, 64, 64, seed=3)
    det = FD.FaceDetector(weights, "cpu")
    boxes, count, overflow = det.detect(frames)
    want = FD.detect_torch(weights, frames)
    assert torch.equal(count, want[1]) and torch.equal(torch.nan_to_num(boxes), torch.nan_to_num(want[0]))
    assert torch.equal(det.first(frames), FD.pick(boxes, count)) and len(det.maps(frames)) == 12
    with pytest.raises(ValueError, match="H and W"):
        det.detect(torch.zeros(1, 80, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        det.detect(torch.zeros(1, 64, 64, 3))


# ---- the wiring ----------------------------------------------------------------------------------------------------------
class StubDetector:
    """Stands where a FaceDetector does: a fixed box, none for a frame whose first pixel is 0."""
    calls = 0

    def _boxes(self, frames_u8):
        StubDetector.calls += 1
        out = torch.tensor([[10.0, 5.0, 50.0, 60.0]]).repeat(frames_u8.shape[0], 1)
        out[frames_u8[:, 0, 0, 0] == 0] = float("nan")
        return out

    first = last = _boxes


def test_landmarks_identity_with_a_detector(tmp_path):
    from PIL import Image
    from instag_amd import track
    from instag_amd.landmarks import FANWeights, landmarks_identity
    fan = FANWeights.random(19)
    os.makedirs(tmp_path / "ori_imgs")
    frames = H.seeded_frames(2, 64, 64, seed=2).numpy()
    frames[0] = 0                                                                # (survives the jpg as zeros)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(tmp_path / "ori_imgs" / f"{i}.jpg")
    with pytest.raises(ValueError, match="the face detector is not part of this project"):
        landmarks_identity(str(tmp_path), fan, "cpu")                           # the unchanged error
    got = landmarks_identity(str(tmp_path), fan, "cpu", detector=StubDetector())
    want = landmarks_identity(str(tmp_path), fan, "cpu", torch.tensor([[float("nan")] * 4, [10.0, 5.0, 50.0, 60.0]]), write=False)
    assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], want[1])
    lms, ids = track.read_landmarks(str(tmp_path / "ori_imgs"))
    assert ids == [1] and np.array_equal(lms[0], got[1].numpy())


def test_evaluator_detects_on_both_frames_and_counts_the_skipped():
    from instag_amd import landmarks as L
    from instag_amd.metrics import Evaluator

    class Renderer:
        bg = torch.zeros(3)
        frames_per_replay = 2

        def render_batch(self, frames, scene_backgrounds=None):
            return torch.stack(frames)

    class Net:
        def landmarks(self, frames_u8, rows):                                    # the box and the frame both enter
            base = frames_u8[:, 0, 0, 0].double()[:, None, None] + rows.double().sum(dim=1)[:, None, None]
            return base + torch.arange(68 * 2, dtype=torch.float64).view(1, 68, 2) * (1 + frames_u8[:, 1, 1, 1].double()[:, None, None])

    frames = [f.permute(2, 0, 1).float() / 255 for f in H.seeded_frames(3, 64, 64, seed=5)]
    gts = [f.permute(2, 0, 1).float() / 255 for f in H.seeded_frames(3, 64, 64, seed=6)]
    gts[1][:, 0, 0] = 0.0                                                        # the ground truth of frame 1 has no face
    frames[0][:, 0, 0], frames[2][:, 0, 0], gts[0][:, 0, 0], gts[2][:, 0, 0], frames[1][:, 0, 0] = 0.5, 0.6, 0.7, 0.8, 0.9
    StubDetector.calls = 0
    rep = Evaluator(Renderer(), lmd=(Net(), StubDetector())).evaluate(frames, gts)
    as_u8 = lambda ts, i: (ts[i].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0)[None]
    box = torch.tensor([[10.0, 5.0, 50.0, 60.0]])
    want = [float(L.lmd_torch(Net().landmarks(as_u8(frames, i), box), Net().landmarks(as_u8(gts, i), box))) for i in (0, 2)]
    assert rep["frames"] == 3 and rep["lmd_skipped"] == 1 and abs(rep["lmd"] - sum(want) / 2) < 1e-9 and rep["lmd"] > 0
    assert StubDetector.calls == 4                                              # rendered and ground truth, two groups
    plain = Evaluator(Renderer(), lmd=(Net(), box[0])).evaluate(frames, gts)
    assert "lmd_skipped" not in plain and "lmd" in plain and "lmd_skipped" not in Evaluator(Renderer()).evaluate(frames, gts)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_c_abi_of_the_face_detect_header():
    """include/instag_face_detect.h goes through the reader of instag_hip.h; the library exports what it declares and
    refuses bad arguments before any device work (no GPU needed)."""
    from instag_amd import _cabi, _lib
    from instag_amd import face_detect as FD
    path = os.path.join(os.path.dirname(_cabi.HEADER), "instag_face_detect.h")
    structs, protos, constants = _cabi.read(path)
    assert list(structs) == ["instag_face_detect_weights"] and _lib.FaceDetectWeights.__name__ == "FaceDetectWeights"
    assert constants == _lib.FACE_DETECT == {
        "INSTAG_FACE_DETECT_LAYERS": 25, "INSTAG_FACE_DETECT_LEVELS": 6, "INSTAG_FACE_DETECT_MAX_CANDIDATES": 4096,
        "INSTAG_FACE_DETECT_MAX_FACES": 16, "INSTAG_FACE_DETECT_MAX_BATCH": 64}
    assert (FD.MAX_CANDIDATES, FD.MAX_FACES, FD.N_LEVELS, len(FD.TRUNK) + FD.N_LEVELS) == (4096, 16, 6, 25)
    assert list(protos) == ["instag_face_detect_workspace_bytes", "instag_face_detect_forward", "instag_face_detect_post",
                            "instag_face_detect", "instag_face_detect_pool", "instag_face_detect_l2norm"] \
        == list(_lib._FACE_DETECT_PROTOTYPES)
    assert [(n, t._length_) for n, t in _lib.FaceDetectWeights._fields_] == [("w", 25), ("scale", 25), ("shift", 25), ("norm", 3)]
    assert not set(protos) & set(_lib.EXPORTED_SYMBOLS)                        # instag_hip.h's list is as it was
    L = _lib.lib()
    for name, (res, args) in _lib._FACE_DETECT_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args

    # the workspace: 144 floats per pixel and the six packed maps
    hs = FD.level_sides(64)
    maps = sum(-(-(8 if l == 0 else 6) * hs[l] * hs[l] // 64) * 64 for l in range(6))
    assert L.instag_face_detect_workspace_bytes(1, 64, 64) == 4 * (144 * 4096 + maps)
    assert 144 << 20 <= L.instag_face_detect_workspace_bytes(1, 512, 512) < 145 << 20
    assert (1 << 30) // L.instag_face_detect_workspace_bytes(1, 512, 512) == 7
    for B, Hh, Ww in ((0, 64, 64), (65, 64, 64), (1, 32, 64), (1, 80, 64), (1, 64, 4128), (9, 2048, 2048)):
        assert L.instag_face_detect_workspace_bytes(B, Hh, Ww) == 0 and b"multiples of 32" in L.instag_last_error()
    one = C.c_void_p(256)
    ptrs, s = (C.c_void_p * 6)(*[256] * 6), _lib.FaceDetectWeights()
    assert L.instag_face_detect_forward(C.byref(s), one, 1, 64, 64, ptrs, one, 1 << 40, None) == _lib.E_ARG
    assert b"NULL weight of layer 0" in L.instag_last_error()
    for l in range(25):
        s.w[l] = s.scale[l] = s.shift[l] = 256
    assert L.instag_face_detect(C.byref(s), one, 1, 64, 64, one, one, one, one, 1 << 40, None) == _lib.E_ARG
    assert b"NULL L2Norm weight" in L.instag_last_error()
    for i in range(3):
        s.norm[i] = 256
    for fn, mid in ((L.instag_face_detect_forward, (ptrs,)), (L.instag_face_detect, (one, one, one))):
        assert fn(C.byref(s), one, 1, 64, 64, *mid, one, 16, None) == 3                          # INSTAG_E_SPACE
        assert b"workspace too small" in L.instag_last_error()
        assert fn(C.byref(s), one, 1, 80, 64, *mid, one, 1 << 40, None) == _lib.E_ARG
        assert b"H and W multiples of 32" in L.instag_last_error()
        assert fn(C.byref(s), one, 65, 64, 64, *mid, one, 1 << 40, None) == _lib.E_ARG
        assert fn(C.byref(s), None, 1, 64, 64, *mid, one, 1 << 40, None) == _lib.E_ARG
        assert b"NULL tensor" in L.instag_last_error()
    assert L.instag_face_detect_forward(C.byref(s), one, 1, 64, 64, (C.c_void_p * 6)(256, 256, 0, 256, 256, 256), one,
                                        1 << 40, None) == _lib.E_ARG
    assert b"NULL map of level 2" in L.instag_last_error()
    assert L.instag_face_detect_post(ptrs, 1, 64, 72, one, one, one, None) == _lib.E_ARG
    assert L.instag_face_detect_post(ptrs, 1, 64, 64, one, None, one, None) == _lib.E_ARG
    assert L.instag_face_detect_pool(one, one, 1, 3, 4, 0, None) == _lib.E_ARG
    assert L.instag_face_detect_pool(one, one, 1, 4, 4, 9, None) == _lib.E_ARG
    assert L.instag_face_detect_l2norm(one, None, one, 1, 4, 4, None) == _lib.E_ARG
    assert L.instag_face_detect_l2norm(one, one, one, 1, 2048, 4, None) == _lib.E_ARG
