"""GPU tests of the landmark operator (csrc/landmarks.hip) against golden G19 and the fp64 CPU statement: the options
of the shared convolution alone, the heatmaps of all four stacks at three sizes, the landmarks, the crop and the decode
kernels on the crafted host cases, chunking and repeatability bit for bit, bad shapes, and a directory.

Heatmaps: e32 = max|fp32 torch statement on the CPU - fp64| / max|fp64| is measured per stack on each case's own crops,
and the operator must be within 8 x e32 of the fp64 heatmaps of that stack (relative to their largest entry) -- the bar
of test_parsing_gpu.py and test_teeth_gpu.py for the same arithmetic: fp32 MFMA, K-tiled sums (K <= 2304 here),
BatchNorm folded into one scale and shift.  Landmarks: exactly the fp64 statement's, except at flip-risk (face,
landmark) pairs, which the fp64 statement alone decides -- the top-two margin of the pair's heatmap, or a neighbour
difference its shift reads, is below 2 x 8 x e32 x scale; at most 5 % of a case's pairs may be left out, and that share
is asserted.  Every test prints the operator's error beside e32 and the bar before it asserts.  A single convolution is
held to the fp64 ``conv2d`` within 8 x the error of the fp32 ``conv2d`` on the same inputs.  Observed on an MI355X
(profiles/landmarks_parity.json), per stack 0..3: G19 (S = 64) e32 6.6e-7, 6.2e-7, 7.4e-7, 7.9e-7, operator 3.6e-7,
3.2e-7, 3.7e-7, 4.0e-7; B = 3 at S = 128 e32 1.07e-6, 1.09e-6, 1.14e-6, 1.27e-6, operator 4.1e-7, 4.0e-7, 4.6e-7, 4.6e-7;
B = 2 at S = 256 e32 9.7e-7, 1.35e-6, 1.34e-6, 9.9e-7, operator 3.8e-7, 4.6e-7, 4.9e-7, 3.7e-7; left out 0 % of the 68,
204 and 136 pairs, no landmark differed from the fp64 statement's, and the fp32 statement's maxima agreed with fp64's
everywhere; the single convolutions e32 6.7e-8 .. 8.0e-7, operator 5.3e-8 .. 2.0e-7 (at most 1.15 x e32).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import landmarks_helpers as H

pytestmark = pytest.mark.gpu

RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    """INSTAG_LANDMARKS_PARITY=<file>: what the tests of this module observed, as JSON (profiles/landmarks_parity.json)."""
    yield
    path = os.environ.get("INSTAG_LANDMARKS_PARITY")
    if path and RECORD:
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(f"{golden_dir}/g19_landmarks.npz")


@pytest.fixture(scope="module")
def g19_weights():
    return H.weights()


@pytest.fixture(scope="module")
def net(g19_weights):
    from instag_amd.landmarks import LandmarkNet
    return LandmarkNet(g19_weights, "cuda")


# ---- the convolution's options alone -----------------------------------------------------------------------------------
def _conv_case(B, cin, cout, k, Hh, Ww, out_ch, out_off, pre, res, res2, relu, seed):
    from instag_amd import landmarks as L
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w = r(B, cin, Hh, Ww), r(cout, cin, k, k) * (2.0 / (cin * k * k)) ** 0.5
    scale, shift = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5, r(cout) * 0.1
    pre_ = (torch.rand(cin, generator=g, dtype=torch.float64) + 0.5, r(cin) * 0.2) if pre else None
    res_ = r(B, out_ch, Hh, Ww) if res else None
    res2_ = r(B, out_ch, Hh // 2, Ww // 2) if res2 else None
    cut = slice(out_off, out_off + cout)
    f32 = lambda t: None if t is None else t.float()
    cut_ = lambda t: None if t is None else t[:, cut]
    raw64, val64 = L.conv_torch(x, w, scale, shift, pre_, cut_(res_), cut_(res2_), relu)
    raw32, val32 = L.conv_torch(f32(x), f32(w), f32(scale), f32(shift), None if pre_ is None else (f32(pre_[0]), f32(pre_[1])),
                                cut_(f32(res_)), cut_(f32(res2_)), relu)
    mag = float(val64.abs().max())
    e32 = max(float((val32.double() - val64).abs().max()), float((raw32.double() - raw64).abs().max())) / mag
    outs = []
    for tile in (0, 1, 2):
        out = torch.full((B, out_ch, Hh, Ww), -7.0, device="cuda")
        raw = L.conv_slice(x.float().cuda(), w.float(), scale, shift, out, out_off, pre_, res_, res2_, raw=True, relu=relu,
                           tile=tile)
        outs.append((out.cpu(), raw.cpu()))
    out, raw = outs[0]
    for o, rw in outs[1:]:
        assert torch.equal(o, out) and torch.equal(rw, raw)                    # the tile does not enter the bits
    untouched = torch.ones(out_ch, dtype=torch.bool)
    untouched[cut] = False
    assert bool((out[:, untouched] == -7.0).all())                              # nothing outside the slice is written
    err = max(float((out[:, cut].double() - val64).abs().max()), float((raw.double() - raw64).abs().max())) / mag
    return err, e32


@pytest.mark.parametrize("name,B,cin,cout,k,side,out_ch,out_off,res2", [
    ("4x4 cout 128 at 0", 1, 256, 128, 3, 4, 256, 0, True),
    ("4x4 cout 64 at 128", 1, 128, 64, 3, 4, 256, 128, True),
    ("4x4 cout 32 at 96", 1, 32, 32, 3, 4, 256, 96, False),
    ("2x2 cout 64 at 192", 1, 64, 64, 3, 2, 256, 192, True),
    ("1x1 map", 2, 64, 64, 3, 1, 256, 192, False),
    ("K = 68", 2, 68, 256, 1, 16, 256, 0, False),
    ("B = 3 on 8x8", 3, 128, 64, 3, 8, 256, 128, True),
    ("B = 3 on 8x8, cout 68 of 272", 3, 256, 68, 1, 8, 272, 136, False),
    ("64 x 64, the wide tile", 8, 64, 64, 3, 64, 256, 128, True),
])
def test_convolution_options(name, B, cin, cout, k, side, out_ch, out_off, res2):
    """One convolution with the pre-activation, the channel slice, both residuals and the contiguous copy, against
    ``conv2d`` in fp64: every tap an edge tap (4 x 4, 2 x 2, 1 x 1), the three couts of a block, K = 68, a tile that
    spans faces, and the size at which the launcher takes the wide tile."""
    err, e32 = _conv_case(B, cin, cout, k, side, side, out_ch, out_off, pre=k == 3 or cin == 68, res=True, res2=res2,
                          relu=cin == 68, seed=len(name))
    print(f"conv {name}: operator {err:.3e} e32 {e32:.3e} bar {H.FACTOR * e32:.3e}")
    RECORD[f"conv {name}"] = dict(operator=err, e32=e32)
    assert 1e-8 < e32 < 2e-5
    assert err <= H.FACTOR * e32


def test_convolution_refuses():
    from instag_amd import landmarks as L
    x, w, one = torch.zeros(1, 32, 4, 4, device="cuda"), torch.zeros(32, 32, 3, 3), torch.ones(32)
    out = torch.zeros(1, 64, 4, 4, device="cuda")
    with pytest.raises(ValueError, match="slice"):
        L.conv_slice(x, w, one, one, out, out_off=48)
    with pytest.raises(ValueError, match="even"):
        L.conv_slice(x[:, :, :3, :3].contiguous(), w, one, one, out[:, :, :3, :3].contiguous(), res2=torch.zeros(1, 64, 1, 1))
    with pytest.raises(ValueError, match="ks 1 or 3"):
        L.conv_slice(x, torch.zeros(32, 32, 5, 5), one, one, out)


# ---- heatmaps and landmarks ----------------------------------------------------------------------------------------------
def _check_landmarks(name, got, c, boxes):
    from instag_amd import landmarks as L
    want = L.decode_torch(c["want"][:, 3], boxes)
    share = float(c["risk"].double().mean())
    keep = ~c["risk"]
    got = got.cpu()
    wrong = int((got != want).any(dim=2)[keep].sum())
    print(f"{name}: left out {100 * share:.3f} % of {keep.numel()} pairs, landmarks wrong outside them {wrong}, inside "
          f"them {int((got != want).any(dim=2)[c['risk']].sum())}; the fp32 statement's maxima differ from fp64's at "
          f"{int((c['arg32'] != c['arg']).sum())} pairs")
    RECORD[f"landmarks {name}"] = dict(left_out=share, pairs=keep.numel(), wrong=wrong)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    assert share <= H.MAX_LEFT_OUT, share
    assert wrong == 0
    return want


def test_g19(g19, g19_weights, net):
    """B = 1, S = 64: the deepest level of the hourglass is 1 x 1, every tile is an edge tile."""
    crops = torch.from_numpy(g19["crop"])[None]
    c = H.case(g19_weights, crops)
    golden = torch.from_numpy(g19["heatmaps"])[None]
    assert float((c["want"][:, 3] - golden).abs().max()) <= 1e-9 * c["scale"][3]
    H.check_heatmaps("g19", net.heatmaps(crops, all_stacks=True), c, RECORD)
    last = net.heatmaps(crops.cuda())
    assert tuple(last.shape) == (1, 68, 16, 16) and torch.equal(last, net.heatmaps(crops, all_stacks=True)[:, 3])
    box = torch.from_numpy(g19["box"])[None]
    want = _check_landmarks("g19", net.decode(last, box), c, box)
    assert np.array_equal(want[0].numpy(), g19["landmarks"])
    # the whole chain from the golden's frame: the crop kernel gives the golden's crop, so the same heatmaps
    frame = torch.from_numpy(g19["frame"])[None]
    assert torch.equal(net.crop(frame, box, S=64).cpu()[0], crops[0])
    assert torch.equal(net.landmarks(frame, box, S=64), net.decode(last, box))


def test_batch_of_three(net, g19_weights):
    """B = 3, S = 128: a tile spans faces; faces that differ in more than noise."""
    crops = H.seeded_crops(3, 128, seed=3)
    c = H.case(g19_weights, crops)
    H.check_heatmaps("B=3 S=128", net.heatmaps(crops, all_stacks=True), c, RECORD)
    boxes = torch.tensor([[10.0, 20.0, 90.0, 120.0], [-20.0, 0.0, 100.0, 130.0], [30.0, 30.0, 60.0, 70.0]])
    _check_landmarks("B=3 S=128", net.decode(net.heatmaps(crops), boxes), c, boxes)
    differ = (c["arg"][0] != c["arg"][1]) | (c["arg"][0] != c["arg"][2])
    assert int(differ.sum()) >= 3, int(differ.sum())                           # the maxima depend on the face


def test_real_size(g19_weights):
    """B = 2, S = 256: the size the package runs at; 512 x 512 frames through the whole chain."""
    from instag_amd import landmarks as L
    from instag_amd.landmarks import LandmarkNet
    other = H.weights(seed=3)
    net = LandmarkNet(other, "cuda")
    frames = H.seeded_frames(2, 512, 512, seed=7)
    boxes = torch.tensor([[140.0, 120.0, 380.0, 400.0], [300.0, 200.0, 560.0, 470.0]])     # the second leaves the frame
    crops = L.crop_torch(frames, boxes)
    got_crops = net.crop(frames, boxes)
    assert torch.equal(got_crops.cpu(), crops)
    c = H.case(other, crops)
    H.check_heatmaps("B=2 S=256", net.heatmaps(got_crops, all_stacks=True), c, RECORD)
    _check_landmarks("B=2 S=256", net.landmarks(frames, boxes), c, boxes)
    assert int((c["arg"][0] != c["arg"][1]).sum()) >= 3


# ---- the kernels around the network ----------------------------------------------------------------------------------------
def test_crop_kernel_on_the_host_cases(net):
    """Bit-equal to ``crop_torch`` on every crafted box, with and without a frame index, at S = 64 and 256."""
    from instag_amd import landmarks as L
    frames, boxes = H.crop_frames()
    for S_ in (64, 256):
        want = L.crop_torch(frames, boxes, S_)
        got = net.crop(frames, boxes, S_)
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want), S_
    names = list(H.CROP_BOXES)
    for n in ("outside", "reversed", "nan"):
        assert int(got[names.index(n)].sum()) == 0
    index = torch.tensor([3, 3, 0, 9, 1])
    pick = boxes[[0, 3, 4, 5, 6]]
    assert torch.equal(net.crop(frames, pick, 64, frame_index=index).cpu(), L.crop_torch(frames, pick, 64, frame_index=index))
    off = torch.tensor([len(names), -1])                                        # a frame that does not exist: a zero crop
    assert int(net.crop(frames, boxes[:2], 64, frame_index=off).sum()) == 0


def test_decode_kernel_on_the_crafted_heatmaps(net):
    from instag_amd import landmarks as L
    hm, boxes = H.decode_heatmaps()
    want = L.decode_torch(hm, boxes)
    got = net.decode(hm.cuda(), boxes)
    assert got.is_cuda and torch.equal(got.cpu(), want)
    assert got[0, 4].tolist() == [56.0, 32.0] and got[0, 0].tolist() == [28.0, -57.0]
    big = torch.zeros(1, 68, 128, 128)
    big[0, :, 127, 126] = 1.0                                                   # R = 128: the last row, a border, no shift
    big[0, 5, 64, 64] = 1.0                                                     # an earlier equal maximum wins
    box = torch.tensor([[10.0, 0.0, 110.0, 95.0]])
    assert torch.equal(net.decode(big.cuda(), box).cpu(), L.decode_torch(big, box))
    nan = net.decode(hm.cuda(), torch.tensor([[float("nan"), 0, 1, 1], [0, 0, 2.0 ** 21, 1]]))
    assert bool(torch.isnan(nan).all())


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def test_chunking_and_repeatability_bitwise(g19_weights):
    """max_batch + 1 faces at S = 64 in one call: rows 0, max_batch - 1 and max_batch equal single-face calls, a second
    call and another operator give the same bits."""
    from instag_amd.landmarks import LandmarkNet
    net = LandmarkNet(g19_weights, "cuda", max_batch=3)
    mb = net.max_batch
    crops = H.seeded_crops(mb + 1, 64, seed=11).cuda()
    heat = net.heatmaps(crops, all_stacks=True)
    assert tuple(heat.shape) == (mb + 1, 4, 68, 16, 16)
    single = LandmarkNet(g19_weights, "cuda", max_batch=1)
    for i in (0, mb - 1, mb):
        assert torch.equal(net.heatmaps(crops[i:i + 1], all_stacks=True)[0], heat[i]), i
        assert torch.equal(single.heatmaps(crops[i:i + 1])[0], heat[i, 3]), i
    assert torch.equal(single.heatmaps(crops, all_stacks=True), heat)
    assert torch.equal(net.heatmaps(crops, all_stacks=True), heat)
    assert not torch.equal(heat[0], heat[mb]) and float(heat.abs().max()) > 0
    frames = H.seeded_frames(mb + 1, 96, 80, seed=12)
    boxes = torch.tensor([[-10.0, 20.0, 50.0, 90.0]]).repeat(mb + 1, 1)
    boxes[1] = float("nan")
    lms = net.landmarks(frames, boxes, S=64)
    assert bool(torch.isnan(lms[1]).all()) and not bool(torch.isnan(lms[[0, 2, 3]]).any())
    assert torch.equal(lms[[0, 2, 3]], single.landmarks(frames[[0, 2, 3]], boxes[0], S=64))


def test_bad_shapes_raise(net):
    assert 1 <= net.max_batch <= 32
    for shape in ((1, 96, 96, 3), (1, 32, 32, 3), (1, 576, 576, 3)):
        with pytest.raises(ValueError, match="multiple of 64"):
            net.heatmaps(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="square"):
        net.heatmaps(torch.zeros(1, 64, 128, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        net.heatmaps(torch.zeros(1, 64, 64, 3))
    with pytest.raises(ValueError, match="boxes"):
        net.landmarks(torch.zeros(2, 64, 64, 3, dtype=torch.uint8), torch.zeros(3, 4))
    with pytest.raises(ValueError, match="heatmaps"):
        net.decode(torch.zeros(1, 67, 16, 16), torch.zeros(1, 4))
    with pytest.raises(ValueError, match="multiple of 16"):
        net.decode(torch.zeros(1, 68, 8, 8), torch.zeros(1, 4))


def test_landmarks_identity_writes_the_files(tmp_path, g19_weights):
    """Three seeded JPEGs: the files hold what ``.landmarks`` gives for the decoded frames, and a NaN box gets none."""
    from PIL import Image
    from instag_amd import track
    from instag_amd.landmarks import LandmarkNet, landmarks_identity
    os.makedirs(tmp_path / "ori_imgs")
    frames = H.seeded_frames(3, 128, 128, seed=21)
    for i, f in zip((0, 1, 10), frames.numpy()):                                # numeric order: 0, 1, 10
        Image.fromarray(f).save(tmp_path / "ori_imgs" / f"{i}.jpg", quality=95)
    boxes = torch.tensor([[30.0, 20.0, 100.0, 110.0], [float("nan")] * 4, [20.0, 30.0, 90.0, 100.0]])
    got = landmarks_identity(str(tmp_path), g19_weights, "cuda", boxes)
    assert tuple(got.shape) == (3, 68, 2) and bool(torch.isnan(got[1]).all())
    assert sorted(p for p in os.listdir(tmp_path / "ori_imgs") if p.endswith(".lms")) == ["0.lms", "10.lms"]
    lms, ids = track.read_landmarks(str(tmp_path / "ori_imgs"))
    assert ids == [0, 10] and np.array_equal(lms, got[[0, 2]].cpu().numpy())
    decoded = torch.from_numpy(np.stack([np.array(Image.open(tmp_path / "ori_imgs" / f"{i}.jpg").convert("RGB")) for i in (0, 10)]))
    assert torch.equal(LandmarkNet(g19_weights, "cuda").landmarks(decoded, boxes[[0, 2]]), got[[0, 2]])
    assert len(torch.unique(got[0], dim=0)) >= 10
