"""Host tests of instag_amd.landmarks (no GPU): the network statement against golden G19 and a second nn.Module
statement, the loader's keys, round trip, named errors and TorchScript route, the crop and the decode on hand-computed
cases, the .lms files, the metric, the stand-in boxes and the C ABI of include/instag_landmarks.h.

The package this restates (face_alignment) was not at hand: nothing here compares with it (landmarks.py's docstring).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import landmarks_helpers as H


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(f"{golden_dir}/g19_landmarks.npz")


@pytest.fixture(scope="module")
def weights():
    return H.weights()


# ---- the network and the loader ----------------------------------------------------------------------------------------
def test_fan_torch_matches_g19(g19, weights):
    from instag_amd import landmarks as L
    crop = torch.from_numpy(g19["crop"])[None]
    stacks = L.fan_torch(weights, L.normalise(crop, torch.float64), all_stacks=True)
    assert tuple(stacks.shape) == (1, 4, 68, 16, 16) and stacks.dtype == torch.float64
    want = torch.from_numpy(g19["heatmaps"])
    assert float((stacks[0, 3] - want).abs().max()) <= 1e-9 * float(want.abs().max())
    for i in range(4):
        assert abs(float(stacks[0, i].abs().max()) - g19["scales"][i]) <= 1e-9 * g19["scales"][i]
    assert torch.equal(L.fan_torch(weights, L.normalise(crop, torch.float64)), stacks[:, 3])
    # the whole chain from the golden's frame and box
    frame, box = torch.from_numpy(g19["frame"])[None], torch.from_numpy(g19["box"])[None]
    assert np.array_equal(L.crop_torch(frame, box, 64)[0].numpy(), g19["crop"])
    assert np.array_equal(L.landmarks_torch(weights, frame, box, torch.float64, S=64)[0].numpy(), g19["landmarks"])
    assert np.array_equal(L.LandmarkNet(weights, "cpu").landmarks(frame, box, S=64)[0].numpy(), g19["landmarks"])


def test_table_and_count():
    from instag_amd import landmarks as L
    assert len(L.LAYERS) == 194 and len(L.PRE) == 194 - 1 - 4 - 4 - 3 - 3
    assert L.LAYERS[0] == ("conv1", "bn1", True, 3, 64, 7, 2) and L.INDEX["conv4.downsample.2"] == 11
    assert L.LAYERS[L.INDEX["al2"]][3:6] == (68, 256, 1) and "al3" not in L.INDEX and "l3" in L.INDEX
    # per face at 256: the stem 0.154, conv2..4 2.80, per stack 5.58 (the hourglass 3.32) GMAC
    macs = L.macs_per_face()
    by_hand = 147 * 64 * 128 * 128 + (9 * (64 * 64 + 64 * 32 + 32 * 32) + 64 * 128) * 128 * 128 \
        + (9 * (128 * 64 + 64 * 32 + 32 * 32) + 9 * (128 * 128 + 128 * 64 + 64 * 64) + 128 * 256) * 64 * 64
    block = 9 * (256 * 128 + 128 * 64 + 64 * 64)
    pix = 64 * 64
    hourglass = block * (pix + 3 * (pix // 4) + 3 * (pix // 16) + 3 * (pix // 64) + 3 * (pix // 256))
    by_hand += 4 * (hourglass + block * pix + (256 * 256 + 256 * 68) * pix) + 3 * (256 * 256 + 68 * 256) * pix
    assert macs == by_hand and 25.0e9 < macs < 25.5e9
    assert L.macs_per_face(64) * 16 == macs


def test_state_dict_keys_round_trip_and_errors(g19, weights):
    import json
    from instag_amd.landmarks import FANWeights
    sd = weights.state_dict()
    layout = json.loads(bytes(g19["layout"]).decode())
    assert sorted((k, list(v.shape)) for k, v in sd.items()) == [(k, s) for k, s in layout]
    assert set(sd) == set(H.FAN(4).state_dict())                               # the second statement's modules' keys
    for key in ("conv2.bn1.running_var", "conv2.downsample.0.weight", "conv2.downsample.2.weight", "m0.b1_4.conv1.weight",
                "m3.b2_plus_1.bn3.bias", "m2.b3_1.conv3.weight", "top_m_1.bn2.running_mean", "conv_last0.bias",
                "bn_end3.num_batches_tracked", "l3.bias", "bl2.weight", "al0.weight"):
        assert key in sd, key
    assert tuple(sd["conv2.bn1.weight"].shape) == (64,) and tuple(sd["conv2.conv1.weight"].shape) == (64, 64, 3, 3)
    assert tuple(sd["conv4.downsample.0.bias"].shape) == (128,) and tuple(sd["al1.weight"].shape) == (256, 68, 1, 1)
    again = FANWeights.from_state_dict({"state_dict": {"module." + k: v for k, v in sd.items()}})
    for a, b in zip(again.layers, weights.layers):
        assert a.keys() == b.keys() and all(torch.equal(a[f], b[f]) for f in a)
    missing = {k: v for k, v in sd.items() if k != "m1.b3_2.bn2.running_mean"}
    with pytest.raises(ValueError, match="m1.b3_2.bn2.running_mean"):
        FANWeights.from_state_dict(missing)
    bad = dict(sd)
    bad["top_m_2.bn1.weight"] = torch.zeros(128)                               # a block's BatchNorm is over its inputs
    with pytest.raises(ValueError, match=r"top_m_2.conv1 gamma has shape \(128,\), expected \(256,\)"):
        FANWeights.from_state_dict(bad)
    bad = dict(sd)
    bad["al0.weight"] = torch.zeros(256, 64, 1, 1)
    with pytest.raises(ValueError, match="al0 weight"):
        FANWeights.from_state_dict(bad)


def test_fold(weights):
    """The fold in front of a block convolution and the one behind conv1, against BatchNorm itself."""
    import torch.nn.functional as F
    from instag_amd import landmarks as L
    folded = weights.folded()
    g = torch.Generator().manual_seed(1)
    for name in ("conv2.conv1", "conv4.downsample.2", "m2.b3_1.conv3"):
        l = L.INDEX[name]
        lay = {f: t.double() for f, t in weights.layers[l].items()}
        w, scale, shift, ps, pb = folded[l]
        assert bool((scale == 1).all()) and bool((shift == 0).all())
        x = torch.randn(2, w.shape[1], 5, 5, generator=g, dtype=torch.float64)
        want = F.relu(F.batch_norm(x, lay["mean"], lay["var"], lay["gamma"], lay["beta"], training=False, eps=L.BN_EPS))
        got = F.relu(x * ps.view(1, -1, 1, 1) + pb.view(1, -1, 1, 1))
        assert float((got - want).abs().max()) < 1e-12
    for name in ("conv1", "conv_last2", "l1", "al0"):
        w, scale, shift, ps, pb = folded[L.INDEX[name]]
        assert ps is None and pb is None
        lay = {f: t.double() for f, t in weights.layers[L.INDEX[name]].items()}
        if "gamma" in lay:
            y = torch.randn(1, w.shape[0], 3, 3, generator=g, dtype=torch.float64)
            want = F.batch_norm(y + lay["bias"].view(1, -1, 1, 1), lay["mean"], lay["var"], lay["gamma"], lay["beta"],
                                training=False, eps=L.BN_EPS)
            assert float((y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) - want).abs().max()) < 1e-12
        else:
            assert bool((scale == 1).all()) and torch.equal(shift, lay["bias"])


def test_torchscript_route(tmp_path, g19, weights):
    """A traced copy of the golden's module, saved and read back through ``FANWeights.load``; and the pickled route."""
    from instag_amd import landmarks as L
    net = H.module(dtype=torch.float32)
    x = L.normalise(torch.from_numpy(g19["crop"])[None])
    scripted = torch.jit.trace(net, x, check_trace=False)
    torch.jit.save(scripted, str(tmp_path / "2DFAN4.zip"))
    torch.save(net.state_dict(), str(tmp_path / "2DFAN4.pth.tar"))
    for name in ("2DFAN4.zip", "2DFAN4.pth.tar"):
        got = L.FANWeights.load(str(tmp_path / name))
        for a, b in zip(got.layers, weights.layers):
            assert all(torch.equal(a[f], b[f]) for f in b), name
    with torch.no_grad():
        assert float((L.fan_torch(got, x) - net(x)[-1]).abs().max()) <= 1e-4 * float(g19["scales"][3])


# ---- the crop ------------------------------------------------------------------------------------------------------------
def test_crop_on_hand_computed_cases():
    from instag_amd import landmarks as L
    frames, boxes = H.crop_frames()
    names = list(H.CROP_BOXES)
    got = L.crop_torch(frames, boxes, 64)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(names), 64, 64, 3)
    at = lambda n: got[names.index(n)]
    fr = lambda n: frames[names.index(n)]
    # (br - ul) = 64 = S: the resize is the identity and the crop is the frame's window
    assert torch.equal(at("identity"), fr("identity")[32:96, 32:96])
    for n in ("outside", "reversed", "nan"):
        assert int(at(n).sum()) == 0
    # the (br - ul) image of "left" has 79 columns (ul_x = trunc(-35.69) = -35, br_x = 44) of which the first 35 lie
    # outside the frame: output column ox reads source columns floor(((2 ox + 1) 79 - 64) / 128) and the next
    zero_cols = [ox for ox in range(64) if ((2 * ox + 1) * 79 - 64) // 128 + 1 < 35]
    assert len(zero_cols) == 28 and int(at("left")[:, zero_cols].sum()) == 0 and int(at("left")[:, 29:].min(dim=0).values.sum()) > 0
    assert int(at("top")[zero_cols].sum()) == 0 and int(at("top")[29:].sum()) > 0
    # "right": 80 columns from 84, the frame ends at 128: source columns from 44 on are outside
    zero_cols = [ox for ox in range(64) if ((2 * ox + 1) * 80 - 64) // 128 >= 44]
    assert len(zero_cols) == 28 and int(at("right")[:, zero_cols].sum()) == 0 and int(at("bottom")[zero_cols].sum()) == 0
    # a constant frame stays constant where the crop is inside it, whatever the scale
    flat = torch.full((2, 128, 128, 3), 201, dtype=torch.uint8)
    assert bool((L.crop_torch(flat, boxes[:2], 64) == 201).all()) and bool((L.crop_torch(flat, boxes[:2], 256) == 201).all())
    # 40 -> 64 along a ramp of step 8: source position (2 o + 1) 40 / 128 - 1 / 2; o = 1 sits at 0.4375: weight 224 of 512
    ramp = (torch.arange(128) * 2).clamp(max=255).to(torch.uint8).view(1, 1, 128, 1).expand(1, 128, 128, 3).contiguous()
    row = L.crop_torch(ramp, boxes[1:2], 64)[0, 10, :, 0].tolist()            # ul_x = 44: the ramp is 88, 90, 92, ...
    assert row[0] == 88 and row[1] == (288 * 88 + 224 * 90 + 256) >> 9 and row[63] == 88 + 2 * 39
    # every case against the pixel-by-pixel statement, and the frame index
    for i, n in enumerate(names):
        want = np.zeros((64, 64, 3), np.uint8) if n == "nan" else H.crop_loops(frames[i].numpy(), H.CROP_BOXES[n], 64)
        assert np.array_equal(got[i].numpy(), want), n
    index = torch.tensor([3, 3, 0])
    picked = L.crop_torch(frames, boxes[[0, 3, 4]], 64, frame_index=index)
    assert np.array_equal(picked[1].numpy(), H.crop_loops(frames[3].numpy(), H.CROP_BOXES["left"], 64))
    assert np.array_equal(picked[2].numpy(), H.crop_loops(frames[0].numpy(), H.CROP_BOXES["right"], 64))
    with pytest.raises(ValueError, match="boxes"):
        L.crop_torch(frames, boxes[:3], 64)


# ---- the decode ----------------------------------------------------------------------------------------------------------
def test_decode_on_crafted_heatmaps():
    from instag_amd import landmarks as L
    hm, boxes = H.decode_heatmaps()
    got = L.decode_torch(hm, boxes)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 68, 2)
    # box 0: centre (60, 36.1), h = 200, R = 16: landmark = trunc(p 12.5 + centre - 100)
    first = got[0].tolist()
    assert first[0] == [28.0, -57.0]              # peak (0, 5), a border: p = (5.5, 0.5); y = trunc(-57.65) toward zero
    assert first[1] == [28.0, 129.0]              # (15, 5): p_y = 15.5
    assert first[2] == [-33.0, 4.0]               # (5, 0): p_x = 0.5 -> trunc(-33.75)
    assert first[3] == [153.0, 4.0]               # (5, 15)
    assert first[4] == [56.0, 32.0]               # (7, 7) with (+, +): p = 7.75 -> 96.875 - 40, 96.875 - 63.9
    assert first[5] == [56.0, 26.0]               # (+, -): p_y = 7.25 -> 90.625 - 63.9
    assert first[6] == [50.0, 32.0] and first[7] == [50.0, 26.0]
    assert first[8] == [53.0, 29.0]               # zero differences: p = 7.5 -> 93.75
    assert first[9] == [19.0, -23.0]              # the tie: (3, 4) is the first maximum, not (9, 2); (+, -)
    # box 1: centre (-250, -243.9): every coordinate negative, the truncation is toward zero
    assert got[1, 8].tolist() == [-256.0, -250.0] and got[1, 4].tolist() == [-253.0, -247.0]
    assert bool((got[1] < 0).all())
    for b in range(2):
        assert np.array_equal(got[b].numpy(), H.decode_loops(hm[b].numpy(), H.DECODE_BOXES[b]))
    assert np.array_equal(L.decode_torch(hm.double(), boxes).numpy(), got.numpy())
    assert bool(torch.isnan(L.decode_torch(hm[:1], torch.tensor([[0.0, float("inf"), 1.0, 1.0]]))).all())


# ---- files, the metric, the stand-in boxes -------------------------------------------------------------------------------
def test_lms_round_trip(tmp_path):
    from instag_amd import track
    from instag_amd.landmarks import write_landmarks
    g = torch.Generator().manual_seed(4)
    lms = torch.randint(-50, 600, (3, 68, 2), generator=g).float().numpy()
    for i, v in zip((2, 11, 7), lms):
        write_landmarks(str(tmp_path / f"{i}.lms"), v)
    assert open(tmp_path / "2.lms").readline().strip() == f"{lms[0, 0, 0]:f} {lms[0, 0, 1]:f}"
    back, ids = track.read_landmarks(str(tmp_path))
    assert ids == [2, 7, 11] and np.array_equal(back, lms[[0, 2, 1]])


def test_landmarks_identity_on_a_cpu_device(tmp_path, weights):
    from PIL import Image
    from instag_amd import track
    from instag_amd.landmarks import landmarks_identity
    os.makedirs(tmp_path / "ori_imgs")
    for i, f in zip((0, 1), H.seeded_frames(2, 64, 64, seed=2).numpy()):
        Image.fromarray(f).save(tmp_path / "ori_imgs" / f"{i}.jpg")
    with pytest.raises(ValueError, match="boxes"):
        landmarks_identity(str(tmp_path), weights, "cpu")
    # (S is the package's 256 here: the statement on the CPU, one face)
    got = landmarks_identity(str(tmp_path), weights, "cpu", torch.tensor([[float("nan")] * 4, [10.0, 5.0, 50.0, 60.0]]))
    assert bool(torch.isnan(got[0]).all()) and not os.path.exists(tmp_path / "ori_imgs" / "0.lms")
    lms, ids = track.read_landmarks(str(tmp_path / "ori_imgs"))
    assert ids == [1] and np.array_equal(lms[0], got[1].numpy())


def test_lmd_matches_numpy():
    from instag_amd.landmarks import lmd_torch
    g = torch.Generator().manual_seed(6)
    pred, gt = torch.randn(4, 68, 2, generator=g, dtype=torch.float64) * 30, torch.randn(4, 68, 2, generator=g, dtype=torch.float64) * 30
    for region, cut in (("mouth", slice(48, 68)), ("face", slice(None))):
        got = lmd_torch(pred, gt, region)
        for i in range(4):
            p, t = pred[i].numpy()[cut], gt[i].numpy()[cut]                     # metrics.py:81-90
            p, t = p - p.mean(0), t - t.mean(0)
            assert abs(float(got[i]) - np.sqrt(((p - t) ** 2).sum(1)).mean(0)) < 1e-12
    assert float(lmd_torch(pred, pred + 3.0).abs().max()) < 1e-12             # a shift of the whole face costs nothing
    with pytest.raises(ValueError, match="region"):
        lmd_torch(pred, gt, "eyes")


def test_meter_lmd_slot():
    from instag_amd.metrics import Meter
    m = Meter("cpu")
    assert "lmd" not in m.report()
    m.add_lmd(torch.tensor([1.0, 2.0]))
    m.add_lmd(torch.tensor([6.0]))
    rep = m.report()
    assert rep["lmd"] == 3.0 and rep["lpips"] is None and rep["frames"] == 0


def test_evaluator_reports_lmd(weights):
    """``Evaluator(lmd=(net, boxes))`` on a stub renderer: the mean of ``lmd_torch`` over the frames whose box is usable,
    from the 8-bit frames as metrics.py:69 makes them; without ``lmd`` the report has no such entry."""
    from instag_amd import landmarks as L
    from instag_amd.metrics import Evaluator

    class Renderer:
        bg = torch.zeros(3)
        frames_per_replay = 2

        def render_batch(self, frames, scene_backgrounds=None):
            return torch.stack(frames)

    frames = [f.permute(2, 0, 1).float() / 255 for f in H.seeded_frames(3, 64, 64, seed=5)]
    gts = [f.permute(2, 0, 1).float() / 255 for f in H.seeded_frames(3, 64, 64, seed=6)]
    boxes = torch.tensor([[4.0, 2.0, 60.0, 62.0], [float("nan")] * 4, [10.0, 8.0, 50.0, 56.0]])

    class Net:                                                                  # S = 64 keeps the statement quick
        inner = L.LandmarkNet(weights, "cpu")

        def landmarks(self, frames_u8, rows):
            return self.inner.landmarks(frames_u8, rows, S=64)

    rep = Evaluator(Renderer(), lmd=(Net(), boxes)).evaluate(frames, gts)
    as_u8 = lambda ts, i: (ts[i].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0)[None]
    want = [float(L.lmd_torch(Net().landmarks(as_u8(frames, i), boxes[i:i + 1]), Net().landmarks(as_u8(gts, i), boxes[i:i + 1])))
            for i in (0, 2)]
    assert rep["frames"] == 3 and abs(rep["lmd"] - sum(want) / 2) < 1e-9 and rep["lmd"] > 0
    assert "lmd" not in Evaluator(Renderer()).evaluate(frames, gts)


def test_boxes_from_labels():
    from instag_amd.landmarks import boxes_from_labels
    lab = torch.zeros(3, 40, 50, dtype=torch.uint8)
    lab[0, 10:20, 12:30] = 1                                                   # skin
    lab[0, 22, 31] = 13                                                        # a lip pixel outside the skin's box
    lab[0, 2:38, 2:48][lab[0, 2:38, 2:48] == 0] = 17                           # hair, neck, cloth, ears do not count
    lab[0, 30:35, 5:10] = 14
    lab[0, 5:8, 40:45] = 7
    lab[2, 39, 49] = 10                                                        # one nose pixel in the corner
    got = boxes_from_labels(lab)
    assert got.dtype == torch.float32 and got[0].tolist() == [12.0, 10.0, 32.0, 23.0]
    assert bool(torch.isnan(got[1]).all()) and got[2].tolist() == [49.0, 39.0, 50.0, 40.0]
    with pytest.raises(ValueError, match="labels"):
        boxes_from_labels(lab[0])


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_c_abi_of_the_landmarks_header():
    """include/instag_landmarks.h goes through the reader of instag_hip.h; the library exports what it declares and
    refuses bad arguments before any device work (no GPU needed)."""
    from instag_amd import _cabi, _lib
    from instag_amd import landmarks as LM
    path = os.path.join(os.path.dirname(_cabi.HEADER), "instag_landmarks.h")
    structs, protos, constants = _cabi.read(path)
    assert list(structs) == ["instag_landmarks_weights"] and _lib.LandmarksWeights.__name__ == "LandmarksWeights"
    assert constants == _lib.LANDMARKS == {
        "INSTAG_LANDMARKS_LAYERS": 194, "INSTAG_LANDMARKS_POINTS": 68, "INSTAG_LANDMARKS_STACKS": 4,
        "INSTAG_LANDMARKS_MIN_SIDE": 64, "INSTAG_LANDMARKS_MAX_SIDE": 512, "INSTAG_LANDMARKS_SIDE_MULTIPLE": 64,
        "INSTAG_LANDMARKS_MAX_BATCH": 64, "INSTAG_LANDMARKS_MAX_FRAME": 8192, "INSTAG_LANDMARKS_MAX_COORD": 1 << 20}
    assert (LM.MIN_SIDE, LM.MAX_SIDE, LM.SIDE_MULTIPLE, LM.MAX_COORD, len(LM.LAYERS), LM.N_POINTS, LM.N_STACKS) == \
        (64, 512, 64, 1 << 20, 194, 68, 4)
    assert list(protos) == ["instag_landmarks_workspace_bytes", "instag_landmarks_forward", "instag_landmarks_crop",
                            "instag_landmarks_conv", "instag_landmarks_decode"] == list(_lib._LANDMARKS_PROTOTYPES)
    assert [n for n, _ in _lib.LandmarksWeights._fields_] == ["w", "scale", "shift", "pre_scale", "pre_shift"]
    assert all(t._length_ == 194 and t._type_ is C.c_void_p for _, t in _lib.LandmarksWeights._fields_)
    assert not set(protos) & set(_lib.EXPORTED_SYMBOLS)                        # instag_hip.h's list is as it was
    L = _lib.lib()
    for name, (res, args) in _lib._LANDMARKS_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args

    # the workspace: 3 x 256 + 512 + 256 + 128 + 68 + 3 x 256 (1/4 + 1/16 + 1/64 + 1/256) floats per position of S/4 x S/4
    assert L.instag_landmarks_workspace_bytes(1, 64) == 4 * 256 * (768 + 512 + 256 + 128 + 68 + 255)
    assert L.instag_landmarks_workspace_bytes(3, 256) == 3 * 256 * L.instag_landmarks_workspace_bytes(1, 64) // 16
    for B, S in ((0, 64), (65, 64), (1, 32), (1, 96), (1, 576)):
        assert L.instag_landmarks_workspace_bytes(B, S) == 0 and b"INSTAG_LANDMARKS_MAX_BATCH" in L.instag_last_error()
    one = C.c_void_p(256)
    s = _lib.LandmarksWeights()
    assert L.instag_landmarks_forward(C.byref(s), one, 1, 64, 0, one, one, 1 << 40, None) == _lib.E_ARG
    assert b"NULL weight of layer 0" in L.instag_last_error()
    for l in range(194):
        s.w[l] = s.scale[l] = s.shift[l] = 256
    assert L.instag_landmarks_forward(C.byref(s), one, 1, 64, 0, one, one, 1 << 40, None) == _lib.E_ARG
    assert b"pre-activation of layer 1 " in L.instag_last_error()
    for l in LM.PRE:
        s.pre_scale[l] = s.pre_shift[l] = 256
    assert L.instag_landmarks_forward(C.byref(s), one, 1, 64, 0, one, one, 16, None) == 3          # INSTAG_E_SPACE
    assert b"workspace too small" in L.instag_last_error()
    assert L.instag_landmarks_forward(C.byref(s), one, 1, 96, 0, one, one, 1 << 40, None) == _lib.E_ARG
    assert L.instag_landmarks_forward(C.byref(s), None, 1, 64, 0, one, one, 1 << 40, None) == _lib.E_ARG
    assert b"NULL tensor" in L.instag_last_error()
    s.pre_scale[LM.INDEX["l0"]] = s.pre_shift[LM.INDEX["l0"]] = 256
    assert L.instag_landmarks_forward(C.byref(s), one, 1, 64, 0, one, one, 1 << 40, None) == _lib.E_ARG
    assert b"pre-activation of layer 55 " in L.instag_last_error()
    assert L.instag_landmarks_crop(one, 1, 64, 64, one, None, 2, 64, one, None) == _lib.E_ARG      # two boxes, one frame
    assert L.instag_landmarks_crop(one, 1, 0, 64, one, one, 1, 64, one, None) == _lib.E_ARG
    assert L.instag_landmarks_crop(one, 1, 64, 64, one, one, 1, 100, one, None) == _lib.E_ARG
    assert L.instag_landmarks_crop(one, 1, 64, 64, None, one, 1, 64, one, None) == _lib.E_ARG
    assert L.instag_landmarks_decode(one, one, 1, 8, one, None) == _lib.E_ARG
    assert L.instag_landmarks_decode(one, one, 1, 144, one, None) == _lib.E_ARG
    assert L.instag_landmarks_decode(one, None, 1, 16, one, None) == _lib.E_ARG
    conv = lambda **kw: L.instag_landmarks_conv(*[{**dict(
        inp=one, w=one, scale=one, shift=one, ps=None, pb=None, res=None, res2=None, raw=None, out=one, B=1, cin=32, cout=32,
        H=4, W=4, ks=3, out_ch=64, out_off=0, relu=0, tile=0, stream=None), **kw}[k] for k in (
        "inp", "w", "scale", "shift", "ps", "pb", "res", "res2", "raw", "out", "B", "cin", "cout", "H", "W", "ks", "out_ch",
        "out_off", "relu", "tile", "stream")])
    for kw in (dict(inp=None), dict(ps=one), dict(out_off=33), dict(ks=5), dict(tile=3), dict(H=3, res2=one), dict(H=512),
               dict(cin=0), dict(B=65)):
        assert conv(**kw) == _lib.E_ARG, kw
