"""Conditions on the inputs of tests/test_loss_kernels_gpu.py (tests/loss_helpers.py), checked on the CPU: they keep the
device tests from passing vacuously -- the restated SSIM map is losses.ssim, the gradient is alive at the image border
and on the tile seams, the composite's zones and the frozen-pixel sets exist, the noise bars resolve one pixel, the
gradient bars are not floors, and the whole comparison runs once against the CPU fallback of face_loss."""
import pytest
import torch

from instag_amd import losses
from tests import loss_helpers as LH

SHAPES = LH.SHAPES
# the shapes on which the device tests assert on frozen pixels
FROZEN_SHAPES = tuple(s for s in SHAPES if s[0] >= 11)


@pytest.mark.parametrize("kind", LH.KINDS)
def test_ssim_map_is_losses_ssim(kind):
    for C, (H, W) in ((3, (33, 49)), (1, (17, 16)), (4, (5, 7))):
        x, y = LH.pair(kind, C, H, W)
        assert x.dtype == torch.float32 and float(x.min()) >= 0 and float(x.max()) <= 1 and float(y.min()) >= 0 and float(y.max()) <= 1
        for dt in (torch.float32, torch.float64):
            assert torch.equal(LH.ssim_map(x.to(dt), y.to(dt)).mean(), losses.ssim(x.to(dt), y.to(dt)))
    x, y = LH.pair("dark", 3, 33, 49)
    assert float(x.max()) < 0.03 and float(y.max()) < 0.03


@pytest.mark.parametrize("shape", SHAPES, ids=LH.sid)
@pytest.mark.parametrize("kind", ("noise", "smooth"))
def test_gradient_reaches_borders_and_seams(kind, shape):
    """The fp64 SSIM gradient reaches 0.1 of its maximum inside the 5-pixel border ring and on every tile seam: a halo
    or padding error there cannot hide under a vanishing gradient.  A seam is the band of pixels whose window crosses
    it (5 on either side: the pixels a wrong halo reaches).  Against the zero padding a smooth frame's windowed variance
    is large and its gradient falls to a few percent of the maximum in the last two rows, where 17x16, 16x33 and 33x49
    have a seam; there the two lines that touch the seam are held to the bar instead: their gradient is at least 10 bars
    (observed: 158 and more), so a tile of one row or column that is dropped or misplaced cannot pass."""
    H, W = shape
    ref = LH.generic_case(kind, 3, H, W).reference()
    g = ref["grads64"][2]["image"].abs()                                             # upstream on SSIM alone
    _, _, bar = LH.tensor_bar(ref["grads32"][2]["image"], ref["grads64"][2]["image"])
    top = float(g.max())
    assert top > 0
    ring = torch.ones(H, W, dtype=torch.bool)
    if H > 2 * LH.RAD and W > 2 * LH.RAD:
        ring[LH.RAD:H - LH.RAD, LH.RAD:W - LH.RAD] = False
    figures, lines = {"ring": float(g[:, ring].max()) / top}, {}
    for r in range(LH.TS, H, LH.TS):
        figures[f"row seam {r}"] = float(g[:, r - LH.RAD:r + LH.RAD, :].max()) / top
        lines[f"row seam {r}"] = float(g[:, r - 1:r + 1, :].max()) / bar
    for c in range(LH.TS, W, LH.TS):
        figures[f"column seam {c}"] = float(g[:, :, c - LH.RAD:c + LH.RAD].max()) / top
        lines[f"column seam {c}"] = float(g[:, :, c - 1:c + 1].max()) / bar
    print(kind, shape, {k: round(v, 3) for k, v in figures.items()}, "lines at the seam / bar",
          {k: round(v, 1) for k, v in lines.items()})
    assert min(figures.values()) >= 0.1, figures
    assert all(v >= 10.0 for v in lines.values()), lines


@pytest.mark.parametrize("shape", SHAPES, ids=LH.sid)
def test_composite_zones(shape):
    H, W = shape
    z = LH.zones(H, W)
    x, y = LH.pair("composite", 3, H, W)
    bg = LH.background(3)[:, None, None].expand(3, H, W)
    assert int(sum(m.sum() for m in z.values())) == H * W            # disjoint, covering
    assert torch.equal(x[:, z["same"]], bg[:, z["same"]]) and torch.equal(y[:, z["same"]], bg[:, z["same"]])
    assert torch.equal(y[:, z["bleed"]], bg[:, z["bleed"]])
    if z["bleed"].any():
        off = (x - y)[:, z["bleed"]].abs()
        assert 0 < float(off.max()) <= 0.02 + 1e-7
    for t in (x, y):
        assert bool(((t[:, z["strip"]] == 0) | (t[:, z["strip"]] == 1)).all())
    counts = {k: int(m.sum()) for k, m in z.items()}
    print(shape, counts)
    if shape == (1, 1):
        assert counts == {"disc": 1, "bleed": 0, "same": 0, "strip": 0}
    elif shape == (5, 7):
        assert counts["disc"] > 0 and 0 < counts["same"] < 16 and 0 < counts["strip"] < 16
    else:
        assert counts["same"] >= 16 and counts["strip"] >= 16 and counts["disc"] >= 16 and counts["bleed"] > 0
        assert int((x == y)[:, z["strip"]].sum()) > 0 and int((x != y)[:, z["strip"]].sum()) > 0


@pytest.mark.parametrize("shape", FROZEN_SHAPES, ids=LH.sid)
def test_frozen_sets_exist(shape):
    H, W = shape
    face, hair, mouth = LH.masks(H, W)
    assert int(LH.frozen_face(H, W).sum()) > 0 and int(LH.frozen_mouth(H, W).sum()) > 0
    assert int((~LH.frozen_mouth(H, W)).sum()) > 0 and int((face & ~mouth).sum()) > 0
    assert int(LH.masks(H, W, "no_hair")[1].sum()) == 0 and bool(LH.masks(H, W, "all_hair")[1].all())
    # the face mode's composition leaves x == y == background pixels on the composite pair (the sign(0) pixels)
    x, _ = LH.pair("composite", 3, H, W)
    outside = ~(face | hair)
    assert int((x[:, outside] == LH.background(3)[:, None]).all(0).sum()) >= 16


@pytest.mark.parametrize("shape", SHAPES, ids=LH.sid)
def test_noise_bars_resolve_one_pixel(shape):
    """One pixel counted twice or not at all moves a mean by about 1 / (C H W): the noise bars are a tenth of that.
    75x131 is the tightest shape and the reason the shapes stop there: its SSIM bar is 3.34e-6 against 3.39e-6 (2.4e-6
    of it 4 mean|t32 - t64|, the rest the 19 additions of the reduction at 2^-24 each), its L1 bar 2.3e-7."""
    H, W = shape
    for case in (LH.generic_case("noise", 3, H, W), LH.plain_case("noise", H, W)):
        bars = case.reference()["term_bars"]
        print(case.name, {k: f"{v:.2e}" for k, v in bars.items()}, f"0.1/(CHW) {0.1 / (3 * H * W):.2e}")
        assert bars["ssim"] < 0.1 / (3 * H * W) and bars["l1"] < 0.1 / (3 * H * W), (case.name, bars)


def _image_cases(kind, H, W):
    return (LH.generic_case(kind, 3, H, W), LH.plain_case(kind, H, W), LH.face_case(kind, H, W),
            LH.face_case(kind, H, W, attn=False, n_extra=0, hair_mask_iter=True), LH.mouth_case(kind, H, W))


@pytest.mark.parametrize("shape", SHAPES, ids=LH.sid)
@pytest.mark.parametrize("kind", LH.KINDS)
def test_image_gradient_bars_are_not_floors(kind, shape):
    """The bar of d_image comes from the fp32 statement's own error, not from the eps32 floor -- but for the 1x1 shape
    and the runs whose upstream gradient is on the L1 output alone (a gradient of +-1/n, exact in fp32)."""
    H, W = shape
    for case in _image_cases(kind, H, W):
        ref = case.reference()
        for ui, up in enumerate(case.upstreams):
            l1_only = (case.out_names[0] == "l1" and up[1] is None) or (case.out_names[1] == "l1" and up[0] is None)
            e32, floor, _ = LH.tensor_bar(ref["grads32"][ui]["image"], ref["grads64"][ui]["image"])
            if e32 <= floor:
                print(f"floor-dominated: {case.name} up={up} e32 {e32:.3e} floor {floor:.3e}")
                assert shape == (1, 1) or l1_only, (case.name, up, e32, floor)


@pytest.mark.parametrize("shape", SHAPES, ids=LH.sid)
@pytest.mark.parametrize("kind", LH.KINDS)
def test_cpu_fallback_meets_its_own_bar(kind, shape):
    """face_loss on CPU tensors is face_loss_torch: the comparison the device tests make, run against it."""
    H, W = shape
    for case in (LH.face_case(kind, H, W), LH.face_case(kind, H, W, attn=False, n_extra=0, hair_mask_iter=True)):
        ratio = LH.compare(case, "cpu")
        assert ratio <= 1.0 + 1e-12
