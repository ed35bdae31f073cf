"""GPU tests of the fused loss kernels (csrc/ssim.hip): l1_ssim_* behind losses.l1_and_ssim and face_loss_* in the face,
mouth and plain modes behind losses.face_loss / mouth_loss_fused / plain_loss_fused, immediate and deferred, against the
fp64 CPU statement of the same lines -- on noise (the control), on smooth shading, on a composited frame (a head in a
disc on a constant background) and on a dark frame, at the shapes at which a 16x16 tile with a halo of 5 can go wrong
(tests/loss_helpers.SHAPES), with every optional term of the face mode on its own and together, the planted branches
(no hair, hair everywhere, a lips rectangle of one pixel, across tiles, over and past the frame, empty), the exact claims
(frozen pixels, sign(0), channel 2 of d_attn, deferred == immediate, run to run) and the partial-sum buffers behind guards.

Inputs, statements and bars: tests/loss_helpers.py.  A bar comes from the case's own inputs -- the fp32 CPU statement's
error against the fp64 one, times FACTOR = 4, the project's rule -- never from the kernels.  Every comparison prints the
operator's error beside e32 and the bar before it asserts; with INSTAG_RECORD_PARITY=1 the figures are written to
profiles/loss_parity.json.

Observed on an MI355X (profiles/loss_parity.json, 363 cases, 413 tests in 8 s), d_image's operator error over
max(e32, eps32 max|fp64|), under the bar of 4 x:
  noise      0.00 .. 1.74, largest: the mouth mode at 33x49 under (1.5, -0.5) (5.9e-9 against e32 3.4e-9);
  smooth     0.26 .. 1.17, largest: the generic kernel, C = 4, 33x49;
  composite  0.00 .. 2.84, largest: the generic kernel at 1x1 under an upstream on SSIM alone (1.9e-7 against e32
             6.8e-8, bar 2.7e-7: at 0.71 of its bar the closest of all comparisons); beyond 1x1 at most 1.56 (the
             generic kernel, C = 4, 17x16);
  dark       0.32 .. 1.75, largest: the generic kernel at 1x1; beyond 1x1 at most 1.44 (the face mode at 17x16).
(0.00: every pixel frozen, hair everywhere under hair_mask_iter.)  The smooth kinds sit no higher than noise: neither
the window's 10-digit taps -- as floats they are one ulp (1.5e-8) from losses._window's at taps 4 and 6 -- nor the
E[x^2] - mu^2 cancellation costs the kernels more than it costs the fp32 torch statement.  The scalars are at most 0.20
of their bars (the loss of the face mode on the dark 5x7 pair: 9.6e-8 against a bar of 4.9e-7).
"""
import ctypes as C
import json
import os

import pytest
import torch

from instag_amd import losses
from tests import loss_helpers as LH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RECORD = {}
SHAPES = LH.SHAPES
BIT_SHAPES = ((1, 1), (17, 16), (75, 131))
FROZEN_SHAPES = tuple(s for s in SHAPES if s[0] >= 11)          # test_loss_helpers_host.py: the sets are non-empty there
shapes = pytest.mark.parametrize("shape", SHAPES, ids=LH.sid)
kinds = pytest.mark.parametrize("kind", LH.KINDS)


def _summary(record):
    """Per kind of image pair: the range of operator / max(e32, floor) over the d_image comparisons, and the case that
    came closest to its bar."""
    out = {}
    for kind in LH.KINDS:
        rows = [(v["d_image"]["ratio"], name) for name, v in record.items() if f" {kind} " in name and "d_image" in v]
        if rows:
            out[kind] = {"comparisons": len(rows), "min_ratio": min(rows)[0], "max_ratio": max(rows)[0], "closest": max(rows)[1]}
    return out


@pytest.fixture(scope="module", autouse=True)
def record():
    yield _RECORD
    for kind, s in _summary(_RECORD).items():
        print(f"{kind}: d_image operator / max(e32, floor) {s['min_ratio']:.2f} .. {s['max_ratio']:.2f} over "
              f"{s['comparisons']} cases, closest to its bar: {s['closest']}")
    if os.environ.get("INSTAG_RECORD_PARITY") == "1" and _RECORD:
        rnd = lambda v: float(f"{v:.4g}") if isinstance(v, float) else v
        cases = {n: {k: {a: rnd(b) for a, b in f.items()} for k, f in v.items()} for n, v in sorted(_RECORD.items())}
        with open(os.path.join(ROOT, "profiles", "loss_parity.json"), "w") as f:
            head = {"rule": "tensors: operator <= 4 max(e32, eps32 max|fp64|), absolute, over all elements; scalars: "
                            "operator <= 4 max(mean|t32 - t64|, eps32 mean|t64|) + d 2^-24 mean|t64| per term, the loss "
                            "the |w|-weighted sum (tests/loss_helpers.py)",
                    "device": torch.cuda.get_device_name(0), "summary": _summary(_RECORD)}
            f.write(json.dumps(head, indent=1, sort_keys=True)[:-2] + ',\n "cases": {\n')
            f.write(",\n".join(f"  {json.dumps(n)}: {json.dumps(v, sort_keys=True)}" for n, v in cases.items()))
            f.write("\n }\n}\n")


def _compare(case):
    return LH.compare(case, "cuda", _RECORD)


# ---- the generic kernel ---------------------------------------------------------------------------------------------------
@shapes
@kinds
def test_generic_matches_fp64(kind, shape):
    """losses.l1_and_ssim at C = 3: both values and the gradient under (g_l1, g_ssim) = (1, -3), L1 alone, SSIM alone."""
    _compare(LH.generic_case(kind, 3, *shape))


@pytest.mark.parametrize("shape", ((17, 16), (33, 49)), ids=LH.sid)
@pytest.mark.parametrize("C", (1, 4))
@kinds
def test_generic_other_channel_counts(kind, C, shape):
    _compare(LH.generic_case(kind, C, *shape))


# ---- the face mode ----------------------------------------------------------------------------------------------------------
@shapes
@kinds
def test_face_all_terms(kind, shape):
    """alpha, hair attention, lips and extra together, hair_mask_iter off: loss, L1 and d_image / d_alpha / d_attn / d_extra
    under an upstream gradient on the loss alone, on the L1 output alone, and (1.5, -0.5) on both."""
    _compare(LH.face_case(kind, *shape))


@shapes
@kinds
def test_face_hair_to_background_alpha_only(kind, shape):
    _compare(LH.face_case(kind, *shape, attn=False, n_extra=0, hair_mask_iter=True))


@pytest.mark.parametrize("bits", range(32))
def test_face_factorial(bits):
    """Every subset of {alpha, attn, lips, extra, hair_mask_iter} on the 33x49 composite."""
    alpha, attn, lips, extra, hmi = (bool(bits >> i & 1) for i in range(5))
    _compare(LH.face_case("composite", 33, 49, alpha=alpha, attn=attn, lips="default" if lips else None,
                          n_extra=int(extra), hair_mask_iter=hmi))


@pytest.mark.parametrize("n_extra", (1, 64, 65, 200))
def test_face_extra_sizes(n_extra):
    """The extra terms' sum: one element, one full lane-strided round, one more, several rounds."""
    _compare(LH.face_case("composite", 33, 49, n_extra=n_extra))
    _compare(LH.face_case("noise", 17, 16, n_extra=n_extra, attn=False))


@pytest.mark.parametrize("variant,hmi", (("no_hair", False), ("no_hair", True), ("all_hair", False), ("all_hair", True)))
@pytest.mark.parametrize("kind", ("composite", "noise"))
def test_face_hair_extremes(kind, variant, hmi):
    """An empty hair mask (1 / max(count, 1)) and hair over the whole frame."""
    for shape in ((17, 16), (33, 49)):
        _compare(LH.face_case(kind, *shape, hair_mask_iter=hmi, variant=variant))


LIPS = {"one pixel": ((15, 16, 15, 16), ((17, 16), (33, 49))),
        "across tiles": ((15, 17, 15, 33), ((16, 33), (33, 49))),
        "whole frame": (lambda H, W: (0, H, 0, W), ((17, 16), (33, 49))),
        "past the frame": (lambda H, W: (H // 2, H + 3, W // 3, W + 3), ((17, 16), (16, 33), (33, 49))),
        "touching the border": (lambda H, W: (0, 3, W - 2, W), ((17, 16), (33, 49)))}


@pytest.mark.parametrize("which", list(LIPS))
@pytest.mark.parametrize("kind", ("composite", "noise"))
def test_face_lips_rectangles(kind, which):
    rect, where = LIPS[which]
    for H, W in where:
        _compare(LH.face_case(kind, H, W, lips=rect(H, W) if callable(rect) else rect))


# ---- the mouth and plain modes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ("p_xyz", "p_raw", "extra"))
@pytest.mark.parametrize("warm", (False, True))
@shapes
@pytest.mark.parametrize("kind", ("composite", "noise"))
def test_mouth_matches_fp64(kind, shape, warm, way):
    """losses.mouth_loss_fused against train_stages.mouth_loss: loss, L1, d_image, d_alpha and the gradient of the
    alignment term however it arrives."""
    _compare(LH.mouth_case(kind, *shape, warm=warm, way=way))


@shapes
@kinds
def test_plain_matches_fp64(kind, shape):
    _compare(LH.plain_case(kind, *shape))


# ---- exact claims -------------------------------------------------------------------------------------------------------------
def _run(case, up=(1.5, -0.5), deferred=False):
    if deferred:
        with losses.defer_finalize():
            outs, grads = case.run("cuda", up)
    else:
        outs, grads = case.run("cuda", up)
    torch.cuda.synchronize()
    return [o.clone() for o in outs], grads


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1].keys() == b[1].keys() and all(
        torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("shape", FROZEN_SHAPES, ids=LH.sid)
@pytest.mark.parametrize("kind", ("composite", "noise"))
def test_frozen_pixels_get_exactly_zero(kind, shape):
    """Pixels the background overwrote take no gradient: hair under hair_mask_iter, lips != mouth in the mouth mode."""
    H, W = shape
    for case, frozen in ((LH.face_case(kind, H, W, hair_mask_iter=True), LH.frozen_face(H, W)),
                         (LH.mouth_case(kind, H, W), LH.frozen_mouth(H, W))):
        for deferred in (False, True):
            g = _run(case, deferred=deferred)[1]["image"].cpu()
            assert int(frozen.sum()) > 0 and int((g[:, frozen] != 0).sum()) == 0, case.name
            assert int((g[:, ~frozen] != 0).sum()) > 0, case.name


@pytest.mark.parametrize("shape", FROZEN_SHAPES, ids=LH.sid)
def test_equal_pixels_get_no_l1_gradient(shape):
    """sign(0) = 0: with the SSIM weight at 0 the gradient is exactly 0 where the composed images are equal, and exactly
    +-(g_loss + g_l1) / (3 H W) -- one rounding of the quotient apart -- elsewhere."""
    H, W = shape
    n = 3 * H * W
    x, y = LH.pair("composite", 3, H, W)
    face, hair, mouth = LH.masks(H, W)
    bg3 = LH.background(3)[:, None, None].expand(3, H, W)
    yg = torch.where(((face | hair) & ~mouth)[None], y, bg3)
    eq = x == yg
    assert int(eq.sum()) >= 16 and int((~eq).sum()) > 0
    g = _run(LH.face_case("composite", H, W, lam=0.0), up=(1.0, None))[1]["image"].cpu()
    assert int((g[eq] != 0).sum()) == 0
    want = torch.sign(x - yg).double() / n
    assert float((g.double() - want).abs().max()) <= 2 * LH.EPS32 / n
    # the generic kernel, upstream on L1 alone
    eq = x == y
    assert int(eq.sum()) >= 16
    g = _run(LH.generic_case("composite", 3, H, W), up=(1.0, None))[1]["image"].cpu()
    assert int((g[eq] != 0).sum()) == 0 and int((g[~eq] == 0).sum()) == 0
    # the plain mode
    g = _run(LH.plain_case("composite", H, W, lam=0.0), up=(1.0, None))[1]["image"].cpu()
    assert int((g[eq] != 0).sum()) == 0 and int((g[~eq] == 0).sum()) == 0


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=LH.sid)
def test_attention_channel_two_is_zero(shape):
    for hmi in (False, True):
        for up in LH.FACE_UPSTREAMS:
            g = _run(LH.face_case("composite", *shape, hair_mask_iter=hmi), up=up)[1]["attn"]
            assert int((g[2] != 0).sum()) == 0
            if up[0] is not None:
                assert int((g[1] != 0).sum()) > 0


@pytest.mark.parametrize("rect", ((5, 5, 3, 9), (9, 4, 3, 9), (4, 9, 7, 7), (40, 45, 3, 9), (4, 9, 60, 70)))
def test_empty_lips_rectangle(rect):
    """out[4] is "0 when empty": with an empty lips rectangle -- no rows, rows reversed, no columns, wholly below or right
    of the frame -- the loss is the loss without the lips term bit for bit and the lips part of d_attn is 0.  (The torch
    statement gives NaN there: this is pinned to the kernel's own comment.)"""
    for deferred in (False, True):
        with_rect = _run(LH.face_case("composite", 33, 49, lips=rect), deferred=deferred)
        without = _run(LH.face_case("composite", 33, 49, lips=None), deferred=deferred)
        assert all(bool(torch.isfinite(o)) for o in with_rect[0])
        assert _same_bits(with_rect, without), (rect, deferred)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=LH.sid)
@pytest.mark.parametrize("mode", ("face", "face hair", "mouth", "mouth cold", "mouth extra", "plain"))
def test_deferred_is_immediate_bit_for_bit(mode, shape):
    """The scalar stage inside the backward launch: the same bits for both values (once backward has run) and every
    gradient, under each upstream; and two immediate runs give the same bits."""
    H, W = shape
    for kind in ("composite", "noise"):
        case = {"face": lambda: LH.face_case(kind, H, W, n_extra=65),
                "face hair": lambda: LH.face_case(kind, H, W, hair_mask_iter=True),
                "mouth": lambda: LH.mouth_case(kind, H, W, way="p_raw"),
                "mouth cold": lambda: LH.mouth_case(kind, H, W, warm=False),
                "mouth extra": lambda: LH.mouth_case(kind, H, W, way="extra"),
                "plain": lambda: LH.plain_case(kind, H, W)}[mode]()
        for up in case.upstreams:
            first, again, late = _run(case, up), _run(case, up), _run(case, up, deferred=True)
            assert _same_bits(first, again), (case.name, up)
            assert _same_bits(first, late), (case.name, up)


def test_generic_runs_are_reproducible():
    for shape in BIT_SHAPES:
        case = LH.generic_case("smooth", 3, *shape)
        assert _same_bits(_run(case, (1.0, -3.0)), _run(case, (1.0, -3.0)))


# ---- the buffers, through the C entries -------------------------------------------------------------------------------------------
GUARD = 4096
SENTINEL = -777.25


class Guarded:
    """``n`` floats between two guards of 4096, everything pre-filled with a sentinel."""

    def __init__(self, n):
        self.all = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.all[GUARD:GUARD + n]

    def guards_untouched(self):
        return bool((self.all[:GUARD] == SENTINEL).all()) and bool((self.all[GUARD + self.t.numel():] == SENTINEL).all())

    def unwritten(self):
        return int((self.t == SENTINEL).sum())


def _check(bufs, written):
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.guards_untouched(), name
        if name in written:
            assert b.unwritten() == 0, (name, b.unwritten())


@pytest.mark.parametrize("shape", ((1, 1), (17, 16), (33, 49)), ids=LH.sid)
@pytest.mark.parametrize("deferred", (False, True))
def test_face_buffers(shape, deferred):
    """maps, partials and out behind guards: the launches write every slot the layout assigns -- all 12 tiles partial sums
    whichever terms are on -- and nothing outside; the gradients are those of the wrapper."""
    from instag_amd import _lib
    from instag_amd._lib import check, ptr
    L = _lib.lib()
    H, W = shape
    case = LH.face_case("composite", H, W, n_extra=65)
    leaves, consts = case.args("cuda", torch.float32)
    a = {k: v.detach() for k, v in {**leaves, **consts}.items()}
    u8 = lambda m: m.to(torch.uint8).contiguous()
    face, hair, mouth = u8(a["face"]), u8(a["hair"]), u8(a["mouth"])
    lips = torch.tensor(LH.default_lips(H, W), dtype=torch.int32, device="cuda")
    flags = losses.FLAG_ALPHA | losses.FLAG_HAIR_ATTN | losses.FLAG_LIPS
    cfg = _lib.FaceLossCfg(H, W, flags, 0.2, 1e-3, 1e-4, 5e-3, 1e-2)
    nparts = L.instag_face_loss_num_partials(H, W)
    assert nparts == 12 * LH.tiles(H, W)
    b = {"maps": Guarded(9 * H * W), "partials": Guarded(nparts), "out": Guarded(5), "d_image": Guarded(3 * H * W),
         "d_alpha": Guarded(H * W), "d_attn": Guarded(3 * H * W)}
    g_loss = torch.tensor([1.5], device="cuda")
    g_l1 = torch.tensor([-0.5], device="cuda")
    stream = _lib.current_stream()
    n_extra = a["extra"].numel()
    if deferred:
        check(L.instag_face_loss_forward_deferred(C.byref(cfg), ptr(a["image"]), ptr(a["gt"]), ptr(face), ptr(hair),
                                                  ptr(mouth), ptr(a["bg"]), ptr(a["alpha"]), ptr(a["attn"]), ptr(lips),
                                                  ptr(a["extra"]), n_extra, ptr(b["maps"].t), ptr(b["partials"].t), stream))
        _check(b, ("maps", "partials"))
        assert b["out"].unwritten() == 5
        check(L.instag_face_loss_backward_deferred(C.byref(cfg), ptr(a["image"]), ptr(a["gt"]), ptr(face), ptr(hair),
                                                   ptr(mouth), ptr(a["bg"]), ptr(lips), ptr(b["maps"].t),
                                                   ptr(b["partials"].t), ptr(a["extra"]), n_extra, ptr(b["out"].t),
                                                   ptr(g_loss), ptr(g_l1), ptr(b["d_image"].t), ptr(b["d_alpha"].t),
                                                   ptr(b["d_attn"].t), stream))
    else:
        check(L.instag_face_loss_forward(C.byref(cfg), ptr(a["image"]), ptr(a["gt"]), ptr(face), ptr(hair), ptr(mouth),
                                         ptr(a["bg"]), ptr(a["alpha"]), ptr(a["attn"]), ptr(lips), ptr(a["extra"]), n_extra,
                                         ptr(b["maps"].t), ptr(b["partials"].t), ptr(b["out"].t), stream))
        _check(b, ("maps", "partials", "out"))
        check(L.instag_face_loss_backward(C.byref(cfg), ptr(a["image"]), ptr(a["gt"]), ptr(face), ptr(hair), ptr(mouth),
                                          ptr(a["bg"]), ptr(lips), ptr(b["maps"].t), ptr(b["out"].t), ptr(g_loss), ptr(g_l1),
                                          ptr(b["d_image"].t), ptr(b["d_alpha"].t), ptr(b["d_attn"].t), stream))
    _check(b, tuple(b))
    outs, grads = _run(case, (1.5, -0.5), deferred=deferred)
    assert torch.equal(b["out"].t[0], outs[0]) and torch.equal(b["out"].t[1], outs[1])
    assert torch.equal(b["d_image"].t.view(3, H, W), grads["image"])
    assert torch.equal(b["d_alpha"].t.view(1, H, W), grads["alpha"])
    assert torch.equal(b["d_attn"].t.view(3, H, W), grads["attn"])


@pytest.mark.parametrize("shape", ((1, 1), (17, 16), (33, 49)), ids=LH.sid)
@pytest.mark.parametrize("channels", (3, 4))
def test_generic_buffers(channels, shape):
    """maps and the two partial-sum arrays of the generic kernel behind guards: C tiles slots each, all written."""
    from instag_amd import _lib
    from instag_amd._lib import check, ptr
    L = _lib.lib()
    H, W = shape
    case = LH.generic_case("composite", channels, H, W)
    leaves, consts = case.args("cuda", torch.float32)
    x, y = leaves["image"].detach(), consts["gt"]
    nb = L.instag_l1_ssim_num_partials(channels, H, W)
    assert nb == channels * LH.tiles(H, W)
    b = {"maps": Guarded(3 * channels * H * W), "part_ssim": Guarded(nb), "part_l1": Guarded(nb),
         "d_image": Guarded(channels * H * W)}
    stream = _lib.current_stream()
    check(L.instag_l1_ssim_forward(ptr(x), ptr(y), channels, H, W, ptr(b["maps"].t), ptr(b["part_ssim"].t),
                                   ptr(b["part_l1"].t), stream))
    _check(b, ("maps", "part_ssim", "part_l1"))
    g_l1, g_ssim = torch.tensor([1.0], device="cuda"), torch.tensor([-3.0], device="cuda")
    check(L.instag_l1_ssim_backward(ptr(x), ptr(y), ptr(b["maps"].t), ptr(g_ssim), ptr(g_l1), channels, H, W,
                                    ptr(b["d_image"].t), stream))
    _check(b, tuple(b))
    outs, grads = _run(case, (1.0, -3.0))
    sums = torch.stack([b["part_ssim"].t, b["part_l1"].t]).sum(dim=1) / float(channels * H * W)     # as the wrapper does
    assert torch.equal(sums[1], outs[0]) and torch.equal(sums[0], outs[1])
    assert torch.equal(b["d_image"].t.view(channels, H, W), grads["image"])
