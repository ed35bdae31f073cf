"""GPU tests of the face detector (csrc/face_detect.hip) against golden G20, the fp64 CPU statement and the loop
statement of tests/face_detect_helpers.py: the 12 maps at three sizes, chunking and repeatability bit for bit, the pool
and the L2Norm kernels alone, the tail alone on the crafted host cases, the whole chain on seeded weights, ``first`` /
``last``, a directory, and bad shapes.

Maps: e32 = max|fp32 torch statement on the CPU - fp64| / max|fp64| is measured per map on each case's own frames, and
the operator must be within 8 x e32 of the fp64 map (relative to its largest entry) -- the bar of test_parsing_gpu.py,
test_teeth_gpu.py and test_landmarks_gpu.py for the same arithmetic: fp32 MFMA, K-tiled sums (K <= 9216 here), the bias
as a shift.  The L2Norm alone is held to 8 x its own e32.  The pool is exact.  The tail alone is exact in what it
decides -- which candidates, in which order, the count, the overflow flag -- and its boxes and scores are within one
float32 step of the loop statement's fp64 values rounded to float32 (the device's fp64 ``exp`` may differ from the
host's in the last place).  End to end the inputs are chosen so that no decision is at flip risk
(face_detect_helpers.flip_margins states the margins and why); that is asserted on the fp64 statement first, then the
operator's detections must be the statement's, no frame left out.  Every test prints what it observed beside the bar
before it asserts; INSTAG_FACE_DETECT_PARITY=<file> records it (profiles/face_detect_parity.json).  Observed on an
MI355X: e32 5.9e-7 .. 5.0e-6 over the 48 maps of the four cases, the operator at 0.16 .. 0.85 x e32; the L2Norm alone at
0.8 .. 1.2 x its e32; end to end 22, 23 and 23 candidates, 2, 2 and 3 detections, the smallest flip margin 2.2 x what is
required, boxes off the fp64 statement's by at most 5.8e-5 pixels and scores by 4.2e-7.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import face_detect_helpers as H

pytestmark = pytest.mark.gpu

RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    path = os.environ.get("INSTAG_FACE_DETECT_PARITY")
    if path and RECORD:
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(f"{golden_dir}/g20_face_detect.npz")


@pytest.fixture(scope="module")
def weights():
    return H.weights()


@pytest.fixture(scope="module")
def det(weights):
    from instag_amd.face_detect import FaceDetector
    return FaceDetector(weights, "cuda")


def _reference(w, frames):
    """The fp64 and the fp32 statement on the CPU: (maps64, maps32, e32 per map, largest entry per map)."""
    from instag_amd import face_detect as FD
    with torch.no_grad():
        m64 = FD.s3fd_torch(w, FD.normalise_torch(frames, torch.float64))
        m32 = FD.s3fd_torch(w, FD.normalise_torch(frames, torch.float32))
    scale = [float(m.abs().max()) for m in m64]
    e32 = [float((a.double() - b).abs().max()) / s for a, b, s in zip(m32, m64, scale)]
    assert all(1e-8 < e < 2e-5 for e in e32), e32
    return m64, m32, e32, scale


def _check_maps(name, got, m64, e32, scale):
    errs = [float((g.double().cpu() - m).abs().max()) / s for g, m, s in zip(got, m64, scale)]
    RECORD[name] = dict(e32=e32, operator=errs, scale=scale)
    for i, (err, e) in enumerate(zip(errs, e32)):
        print(f"{name} map {i}: operator {err:.3e} e32 {e:.3e} bar {H.FACTOR * e:.3e} scale {scale[i]:.3e}")
    for i, (g, m) in enumerate(zip(got, m64)):
        assert tuple(g.shape) == tuple(m.shape) and g.dtype == torch.float32 and g.is_cuda
        assert errs[i] <= H.FACTOR * e32[i], (name, i, errs[i], e32[i])


# ---- the maps ------------------------------------------------------------------------------------------------------------
def test_maps_match_g20(g20, weights, det):
    frames = torch.from_numpy(g20["frame"])[None]
    m64, _, e32, scale = _reference(weights, frames)
    for i, m in enumerate(m64):
        assert np.abs(m[0].numpy() - g20[f"map{i}"]).max() <= 1e-12 * scale[i]
    got = det.maps(frames)
    _check_maps("G20 64 x 96", got, m64, e32, scale)
    again = det.maps(frames)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                   # two runs, the same bits


@pytest.mark.parametrize("name,B,Hh,Ww,max_batch", [("B = 1 at 64 x 64", 1, 64, 64, None), ("B = 3 at 96 x 64 in chunks of 2", 3, 96, 64, 2)])
def test_maps_at_other_sizes_and_across_a_chunk_boundary(weights, det, name, B, Hh, Ww, max_batch):
    """64 x 64: pool5 is 2 x 2, fc6 sees mostly border, conv7_2 is 2 x 2.  96 x 64 in chunks of 2: the chunked maps are the
    unchunked ones bit for bit, and a frame's bits do not depend on its neighbours."""
    from instag_amd.face_detect import FaceDetector
    frames = H.seeded_frames(B, Hh, Ww, seed=7)
    m64, _, e32, scale = _reference(weights, frames)
    whole = det.maps(frames)
    _check_maps(name, whole, m64, e32, scale)
    if max_batch:
        chunked = FaceDetector(weights, "cuda", max_batch=max_batch).maps(frames)
        alone = det.maps(frames[1:2])
        assert all(torch.equal(a, b) for a, b in zip(whole, chunked))
        assert all(torch.equal(a[1:2], b) for a, b in zip(whole, alone))
    assert all(torch.equal(a, b) for a, b in zip(whole, det.maps(frames)))


# ---- the new kernels alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,border", [((2, 3, 6, 10), 0), ((2, 3, 6, 10), 2), ((1, 64, 64, 96), 0), ((3, 512, 4, 6), 2),
                                          ((1, 5, 2, 2), 1)])
def test_pool_is_max_pool2d(shape, border):
    from instag_amd.face_detect import pool_device
    g = torch.Generator().manual_seed(sum(shape) + border)
    x = torch.randn(*shape, generator=g) - 0.5                                   # mostly negative: a zero border shows
    got = pool_device(x.cuda(), border).cpu()
    want = F.pad(F.max_pool2d(x, 2, 2), (border,) * 4)
    assert got.shape == want.shape and torch.equal(got, want)
    if border:
        inner = torch.zeros(got.shape[2:], dtype=torch.bool)
        inner[border:-border, border:-border] = True
        assert bool((got[:, :, ~inner] == 0).all())


@pytest.mark.parametrize("B,Cn,h,w", [(1, 256, 16, 24), (3, 512, 3, 5), (2, 7, 1, 1), (1, 512, 40, 40)])
def test_l2norm_against_fp64(B, Cn, h, w):
    from instag_amd.face_detect import l2norm_device, l2norm_torch
    g = torch.Generator().manual_seed(B * Cn + h)
    x = torch.relu(torch.randn(B, Cn, h, w, generator=g, dtype=torch.float64))  # behind a ReLU, as in the network
    x[0, :, 0, 0] = 0.0                                                           # an all-zero position: 0 / 1e-10
    wt = torch.rand(Cn, generator=g, dtype=torch.float64) * 10 + 1
    want = l2norm_torch(x, wt)
    scale = float(want.abs().max())
    e32 = float((l2norm_torch(x.float(), wt.float()).double() - want).abs().max()) / scale
    got = l2norm_device(x.float().cuda(), wt.float()).cpu()
    err = float((got.double() - want).abs().max()) / scale
    print(f"l2norm {B} x {Cn} x {h} x {w}: operator {err:.3e} e32 {e32:.3e} bar {H.FACTOR * e32:.3e}")
    RECORD[f"l2norm {B}x{Cn}x{h}x{w}"] = dict(e32=e32, operator=err)
    assert err <= H.FACTOR * e32 and bool((got[0, :, 0, 0] == 0).all())


# ---- the tail alone --------------------------------------------------------------------------------------------------------
CASES = H.tail_cases()


def _check_tail(name, maps, got, expected=None):
    """The operator's (boxes, count, overflow) against the loop statement on the same logits."""
    boxes, count, overflow = (t.cpu() for t in got)
    assert boxes.dtype == torch.float32 and count.dtype == torch.int32 and overflow.dtype == torch.bool
    for b in range(boxes.shape[0]):
        t = H.tail_loops(maps, b)
        n = len(t["det_index"])
        print(f"{name} frame {b}: candidates {len(t['index'])} detections {n} operator count {int(count[b])} "
              f"overflow {bool(overflow[b])} / {t['overflow']}")
        assert int(count[b]) == n and bool(overflow[b]) == t["overflow"]
        k = min(n, H.MAX_FACES)
        assert H.within_one_ulp(boxes[b, :k, :4].numpy(), t["det_boxes"][:k])   # the same candidates in the same order
        assert H.within_one_ulp(boxes[b, :k, 4].numpy(), t["det_score"][:k].astype(np.float64))
        assert bool(torch.isnan(boxes[b, k:]).all())
        if expected is not None:
            assert bool(overflow[b]) == expected["overflow"][b]
            if expected["count"] is not None:
                assert n == expected["count"][b] and t["det_index"].tolist() == expected["index"][b]


@pytest.mark.parametrize("name", list(CASES))
def test_tail_on_the_hand_computed_cases(det, name):
    maps, Hh, Ww, want = CASES[name]
    got = det.post(maps, Hh, Ww)
    _check_tail(name, maps, got, want)
    again = det.post(maps, Hh, Ww)
    assert all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip(got, again))
    if "boxes" in want:
        assert H.within_one_ulp(got[0][0, 0, :4].cpu().numpy(), want["boxes"])
        assert H.within_one_ulp(got[0][0, 0, 4:].cpu().numpy(), [want["score"]])


def test_the_0_05_threshold_through_the_overflow_flag(det):
    """4096 sure candidates and one more position: its score decides the flag (the cases 'cap ...' by name)."""
    for name, over in (("cap at 0.05", False), ("cap below 0.05", False), ("cap above 0.05", True)):
        maps, Hh, Ww, _ = CASES[name]
        assert det.post(maps, Hh, Ww)[2].tolist() == [over], name


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    from instag_amd.face_detect import FaceDetector
    w = H.weights(H.E2E_SHIFT, H.E2E_SEED, H.E2E_GAIN)
    frames = H.seeded_frames(3, H.G20_H, H.G20_W, seed=H.E2E_SEED)
    m64, m32, e32, scale = _reference(w, frames)
    return dict(w=w, det=FaceDetector(w, "cuda", max_batch=2), frames=frames, m64=m64, m32=m32, e32=e32, scale=scale)


def test_end_to_end_detections_are_the_statements(e2e):
    m64, m32, det, frames = e2e["m64"], e2e["m32"], e2e["det"], e2e["frames"]
    # the statement alone: enough candidates, a suppression, two detections in a frame, and nothing at flip risk
    tails = [H.tail_loops(m64, b) for b in range(3)]
    suppressed = [int((H.overlaps(t)[0] > 0.3).sum()) for t in tails]
    print("candidates", [len(t["index"]) for t in tails], "detections", [len(t["det_index"]) for t in tails], "suppressed", suppressed)
    assert all(16 <= len(t["index"]) <= H.MAX_CANDIDATES and not t["overflow"] for t in tails)
    assert max(suppressed) >= 1 and max(len(t["det_index"]) for t in tails) >= 2
    RECORD["end to end"] = {}
    for b in range(3):
        margins = H.flip_margins(m64, m32, b)
        RECORD["end to end"][f"frame {b}"] = {k: dict(margin=v[0], required=v[1]) for k, v in margins.items()}
        for k, (margin, need) in margins.items():
            print(f"frame {b} |{k}|: smallest {margin:.3e} required {need:.3e}")
            assert margin >= need, (b, k, margin, need)
    # the operator: the maps within the bar, then the statement's detections
    got_maps = det.maps(frames)
    _check_maps("end to end 3 x 64 x 96", got_maps, m64, e2e["e32"], e2e["scale"])
    boxes, count, overflow = det.detect(frames)
    via_post = det.post(got_maps, H.G20_H, H.G20_W)
    assert all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip((boxes, count, overflow), via_post))
    _check_tail("end to end, on the operator's maps", [m.cpu() for m in got_maps], (boxes, count, overflow))
    err_conf = max(float((a.double() - w).abs().max()) for a, w in zip(m32[0::2], m64[0::2]))
    err_loc = max(float((a.double() - w).abs().max()) for a, w in zip(m32[1::2], m64[1::2]))
    for b, t in enumerate(tails):
        own = H.tail_loops([m.cpu() for m in got_maps], b)
        assert int(count[b]) == len(t["det_index"]) and not bool(overflow[b])
        assert own["det_index"].tolist() == t["det_index"].tolist() and own["index"].tolist() == t["index"].tolist()
        k = min(len(t["det_index"]), H.MAX_FACES)
        side = (t["det_boxes"][:k, 2:] - t["det_boxes"][:k, :2]).max(axis=1, keepdims=True)
        tol = H.FACTOR * err_loc * 0.2 * np.maximum(side, 512.0) + 1e-4         # an edge moves by at most 0.1 (pw + w) per unit of loc, pw <= 512
        diff = np.abs(boxes[b, :k, :4].cpu().numpy().astype(np.float64) - t["det_boxes"][:k])
        print(f"frame {b}: boxes off by {diff.max():.3e} (tolerance {tol.min():.3e}), scores by "
              f"{np.abs(boxes[b, :k, 4].cpu().numpy().astype(np.float64) - t['det_score'][:k]).max():.3e} (tolerance {H.FACTOR * err_conf / 2:.3e})")
        assert bool((diff <= tol).all())
        assert np.abs(boxes[b, :k, 4].cpu().numpy().astype(np.float64) - t["det_score"][:k]).max() <= H.FACTOR * err_conf / 2 + 1e-7


def test_first_last_and_a_frame_without_a_face(e2e):
    from instag_amd.face_detect import FaceDetector
    det, frames = e2e["det"], e2e["frames"]
    boxes, count, _ = det.detect(frames)
    first, last = det.first(frames), det.last(frames)
    assert first.dtype == torch.float32 and tuple(first.shape) == (3, 4)
    for b in range(3):
        n = min(int(count[b]), H.MAX_FACES)
        assert n >= 1 and torch.equal(first[b], boxes[b, 0, :4]) and torch.equal(last[b], boxes[b, n - 1, :4])
    none = FaceDetector(H.weights(conf_shift=40.0), "cuda")                      # every background logit far above: no face
    one = H.seeded_frames(1, 64, 64, seed=9)
    b0, c0, o0 = none.detect(one)
    assert c0.tolist() == [0] and o0.tolist() == [False] and bool(torch.isnan(b0).all())
    assert bool(torch.isnan(none.first(one)).all()) and bool(torch.isnan(none.last(one)).all())


def test_a_directory(tmp_path, e2e):
    from PIL import Image
    from instag_amd import convnet, track
    from instag_amd.face_detect import detect_identity
    from instag_amd.landmarks import FANWeights, LandmarkNet, landmarks_identity
    os.makedirs(tmp_path / "ori_imgs")
    for i, f in zip((10, 2, 7), e2e["frames"].numpy()):
        Image.fromarray(f).save(tmp_path / "ori_imgs" / f"{i}.jpg", quality=95)
    ids, frames = zip(*[(i, f) for i, f, _ in convnet.frame_batches(str(tmp_path), 3)])
    assert ids[0] == [2, 7, 10]
    want = e2e["det"].first(frames[0])
    got = detect_identity(str(tmp_path), e2e["w"], "cuda", batch=2)
    assert got.is_cuda and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    fan = FANWeights.random(19)
    lms = landmarks_identity(str(tmp_path), fan, "cuda", detector=e2e["det"], batch=2)
    direct = LandmarkNet(fan, "cuda", max_batch=2).landmarks(frames[0], want)
    assert torch.equal(torch.nan_to_num(lms), torch.nan_to_num(direct))
    usable = [i for i, row in zip(ids[0], want.cpu()) if not bool(torch.isnan(row).any())]
    back, back_ids = track.read_landmarks(str(tmp_path / "ori_imgs"))
    assert back_ids == usable and len(usable) >= 1
    assert np.array_equal(back, lms.cpu().numpy()[[ids[0].index(i) for i in usable]])


def test_evaluator_detects_its_own_boxes(e2e):
    """``Evaluator(lmd=(LandmarkNet, FaceDetector))`` on a stub renderer: the boxes are ``last`` of the rendered and of the
    ground-truth frame, a gray ground truth has no face (its largest score under these weights is 0.10) and is counted."""
    from instag_amd import landmarks as L
    from instag_amd.metrics import Evaluator

    class Renderer:
        bg = torch.zeros(3, device="cuda")
        frames_per_replay = 2

        def render_batch(self, frames, scene_backgrounds=None):
            return torch.stack(frames)

    det = e2e["det"]
    net = L.LandmarkNet(L.FANWeights.random(19), "cuda", max_batch=2)
    gt_u8 = H.seeded_frames(3, H.G20_H, H.G20_W, seed=71)
    gt_u8[1] = 128
    as_float = lambda u8: [f.permute(2, 0, 1).float().cuda() / 255 for f in u8]
    frames, gts = as_float(e2e["frames"]), as_float(gt_u8)
    rep = Evaluator(Renderer(), lmd=(net, det)).evaluate(frames, gts)
    as_u8 = lambda ts: torch.stack([(t.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0) for t in ts])
    p8, g8 = as_u8(frames), as_u8(gts)
    assert torch.equal(p8.cpu(), e2e["frames"]) and torch.equal(g8.cpu(), gt_u8)   # u8 -> float -> u8 is the identity
    pb, gb = det.last(p8), det.last(g8)
    assert bool(torch.isnan(gb[1]).all()) and not bool(torch.isnan(pb).any()) and not bool(torch.isnan(gb[[0, 2]]).any())
    want = L.lmd_torch(net.landmarks(p8[[0, 2]], pb[[0, 2]]), net.landmarks(g8[[0, 2]], gb[[0, 2]]))
    print("lmd", rep["lmd"], "skipped", rep["lmd_skipped"], "per frame", want.tolist())
    assert rep["frames"] == 3 and rep["lmd_skipped"] == 1 and abs(rep["lmd"] - float(want.double().mean())) < 1e-6 * max(1.0, rep["lmd"])


# ---- bad shapes ------------------------------------------------------------------------------------------------------------
def test_bad_shapes(weights, det):
    from instag_amd import _lib
    from instag_amd.face_detect import FaceDetector
    with pytest.raises(ValueError, match="H and W"):
        det.detect(torch.zeros(1, 80, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        det.maps(torch.zeros(1, 64, 64, 3))
    with pytest.raises(ValueError, match="max_batch"):
        FaceDetector(weights, "cuda", max_batch=65)
    with pytest.raises(ValueError, match=r"maps\[1\]"):
        maps = H.blank_maps(1, 64, 64)
        det.post(maps[:1] + [maps[1][:, :3]] + maps[2:], 64, 64)
    L = _lib.lib()
    frames = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device="cuda")
    out = (torch.empty(1, 16, 5, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
           torch.empty(1, dtype=torch.uint8, device="cuda"))
    need = L.instag_face_detect_workspace_bytes(1, 64, 64)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    args = lambda B, nbytes: (C.byref(det._struct), _lib.ptr(frames), B, 64, 64, *[_lib.ptr(t) for t in out], _lib.ptr(ws), nbytes, None)
    assert L.instag_face_detect(*args(1, need - 1)) == 3                       # INSTAG_E_SPACE
    assert b"workspace too small" in L.instag_last_error()
    assert L.instag_face_detect(*args(65, need)) == _lib.E_ARG and b"B <= 64" in L.instag_last_error()
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.check_arg(L.instag_face_detect(*args(1, 16)), "face_detect")
