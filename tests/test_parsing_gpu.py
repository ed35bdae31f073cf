"""GPU tests of the face parser (csrc/parsing.hip) against golden G14 and the fp64 CPU statement: the three frame
sizes at which the tiling differs, the final stage alone, chunking and determinism bit for bit, and the chain into
gt_and_torso.

Logits: e32 = max|fp32 torch statement on the CPU - fp64| / max|fp64| is measured on each case's own frames, and the
operator must be within 8 x e32 of the fp64 logits at 1/8 resolution (relative to their largest entry) -- the bar of
test_ave_encoder_gpu.py for the same arithmetic: fp32 MFMA, K-tiled sums (K <= 4608 here), BatchNorm folded into one
scale and shift.  Labels and colours: exactly the fp64 statement's, except at flip-risk pixels, which the fp64 statement
alone decides -- the top-two margin of its full-size logits is below 2 x 8 x e32 x scale; at most 1 % of a case's pixels
may be left out, and that share is asserted.  Every test prints the operator's error beside e32 and the bar before it
asserts.  Observed on an MI355X (profiles/parsing_parity.json): G14 e32 1.11e-6, operator 6.9e-7, left out 0.033 %;
B = 3 at 96 x 64 e32 1.66e-6, operator 5.5e-7, left out 0.016 %; 512 x 512 e32 3.39e-6, operator 1.06e-6, left out
0.048 %; no label differed from the fp64 statement's in any case, inside the left-out pixels or outside them.
"""
import numpy as np
import pytest
import torch

from tests import parsing_helpers as H
from tests import segnet_helpers as S

pytestmark = pytest.mark.gpu

MAX_LEFT_OUT = 0.01


def _case(weights, frames):
    return S.case(H.reference_fp64, weights, frames)


_check_logits = S.check_logits


def _check_labels(name, labels, colours, c):
    from instag_amd import parsing as P
    share = float(c["risk"].double().mean())
    keep = ~c["risk"]
    labels = labels.cpu()
    wrong = int((labels != c["labels"])[keep].sum())
    print(f"{name}: left out {100 * share:.4f} % of {keep.numel()} pixels, labels wrong outside them {wrong}, "
          f"wrong inside them {int((labels != c['labels'])[c['risk']].sum())}, distinct {len(torch.unique(c['labels']))}")
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == tuple(c["labels"].shape)
    assert share <= MAX_LEFT_OUT, share
    assert wrong == 0
    if colours is not None:
        want = P.colour_map_torch(c["labels"])
        colours = colours.cpu()
        assert colours.dtype == torch.uint8 and tuple(colours.shape) == tuple(want.shape)
        assert torch.equal(colours[keep], want[keep])
        assert torch.equal(colours, P.colour_map_torch(labels))              # the operator's colours are its labels'


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(f"{golden_dir}/g14_parsing.npz")


@pytest.fixture(scope="module")
def g14_weights():
    return H.weights()


@pytest.fixture(scope="module")
def other_weights():
    return H.weights(seed=3)


def test_g14(g14, g14_weights):
    """B = 1, 64 x 96: feat32 is 2 x 3, every tile is an edge tile, the pools run over 6, 24 and 96 elements."""
    from instag_amd.parsing import FaceParser
    frames = torch.from_numpy(g14["frame"])[None]
    c = _case(g14_weights, frames)
    golden = torch.from_numpy(g14["logits8"])[None]
    assert float((c["want"] - golden).abs().max()) <= 1e-9 * c["scale"]
    assert np.array_equal(c["labels"][0].numpy(), g14["labels"])
    parser = FaceParser(g14_weights, "cuda")
    _check_logits("g14", parser.logits(frames), c)
    _check_labels("g14", parser.labels(frames), parser.parse(frames.cuda()), c)


def test_batch_of_three_transposed(other_weights):
    """B = 3, 96 x 64, other weights: the batch-joint m tiling (a tile spans frames) and the other aspect."""
    from instag_amd.parsing import FaceParser
    frames = H.seeded_frames(3, 96, 64, seed=3)
    c = _case(other_weights, frames)
    parser = FaceParser(other_weights, "cuda")
    _check_logits("B=3 96x64", parser.logits(frames), c)
    _check_labels("B=3 96x64", parser.labels(frames), parser.parse(frames), c)
    assert len(torch.unique(c["labels"])) >= 5


def test_real_size(g14_weights):
    """B = 1, 512 x 512: the size InsTaG parses at; the large tiles, several workgroups per layer."""
    from instag_amd.parsing import FaceParser
    frames = H.seeded_frames(1, 512, 512, seed=7)
    c = _case(g14_weights, frames)
    parser = FaceParser(g14_weights, "cuda")
    _check_logits("512x512", parser.logits(frames), c)
    _check_labels("512x512", parser.labels(frames), None, c)


def test_final_stage_alone():
    """Crafted logits at 1/8 of 64 x 96, colours at 50 x 70: every class wins somewhere (every colour branch), and two
    identical dominant planes give the first of them everywhere."""
    from instag_amd import parsing as P
    g = torch.Generator().manual_seed(5)
    h8, w8, Hh, Ww = 8, 12, 64, 96
    cells = torch.arange(h8 * w8).view(h8, w8)
    logits = (torch.rand(1, 19, h8, w8, generator=g) * 16).round() / 8                       # [0, 2] in eighths
    winner = (cells * 7 + cells // w8) % 19
    logits[0].scatter_(0, winner[None], 8.0 + (torch.rand(1, h8, w8, generator=g) * 16).round() / 8)
    full = P.upsample_torch(logits.double(), Hh, Ww)
    want = P.first_argmax(full)
    assert len(torch.unique(want)) == 19
    risk = H.top_two_margin(full) < 1e-5 * float(logits.abs().max())   # fp32 interpolation: a few ulp of the scale
    share = float(risk.double().mean())
    colours, labels = P.colour_map(logits.cuda(), Hh, Ww, out_size=(50, 70), want_labels=True)
    print(f"final stage: left out {100 * share:.4f} %, wrong {int((labels.cpu() != want)[~risk].sum())}")
    assert share <= MAX_LEFT_OUT
    assert torch.equal(labels.cpu()[~risk], want[~risk])
    assert len(torch.unique(labels)) == 19
    assert tuple(colours.shape) == (1, 50, 70, 3) and colours.dtype == torch.uint8
    assert torch.equal(colours.cpu(), P.colour_map_torch(labels.cpu(), 50, 70))
    assert {tuple(v) for v in colours.cpu().reshape(-1, 3).tolist()} == {tuple(v) for v in P.COLOURS.tolist()}
    # colours alone, and at the labels' own size
    assert torch.equal(P.colour_map(logits.cuda(), Hh, Ww, out_size=(50, 70)), colours)
    assert torch.equal(P.colour_map(logits.cuda(), Hh, Ww).cpu(), P.colour_map_torch(labels.cpu()))

    tie = (torch.rand(1, 19, h8, w8, generator=g) * 16).round() / 8
    tie[0, 3] = 6.0 + (torch.rand(h8, w8, generator=g) * 16).round() / 8
    tie[0, 7] = tie[0, 3]
    colours, labels = P.colour_map(tie.cuda(), Hh, Ww, out_size=(50, 70), want_labels=True)
    assert bool((labels == 3).all())
    assert bool((colours.cpu() == torch.tensor([0, 0, 255], dtype=torch.uint8)).all())


def test_chunking_bitwise(g14_weights):
    """max_batch + 1 frames at 64 x 64 in one call: rows 0, max_batch - 1 and max_batch equal single-frame calls."""
    from instag_amd.parsing import FaceParser
    parser = FaceParser(g14_weights, "cuda", max_batch=3)
    mb = parser.max_batch
    frames = H.seeded_frames(mb + 1, 64, 64, seed=11).cuda()
    logits, labels, colours = parser.logits(frames), parser.labels(frames), parser.parse(frames)
    assert tuple(logits.shape) == (mb + 1, 19, 8, 8) and tuple(colours.shape) == (mb + 1, 64, 64, 3)
    single = FaceParser(g14_weights, "cuda", max_batch=1)
    for i in (0, mb - 1, mb):
        assert torch.equal(parser.logits(frames[i:i + 1])[0], logits[i]), i
        assert torch.equal(single.logits(frames[i:i + 1])[0], logits[i]), i
        assert torch.equal(parser.labels(frames[i:i + 1])[0], labels[i]), i
        assert torch.equal(parser.parse(frames[i:i + 1])[0], colours[i]), i
    assert not torch.equal(logits[0], logits[mb])
    pick = [0, mb - 1, mb]
    c = _case(g14_weights, frames[pick].cpu())
    _check_logits("chunked", logits[pick], c)


def test_a_smaller_call_keeps_the_workspace(g14_weights):
    """Three 64 x 64 frames in chunks of two (the chunk tail), then one: the second call needs fewer bytes, so the
    workspace stays where it is; both results are a fresh operator's bit for bit."""
    from instag_amd.parsing import FaceParser
    frames = H.seeded_frames(3, 64, 64, seed=12).cuda()
    parser = FaceParser(g14_weights, "cuda", max_batch=2)
    first = parser.logits(frames).clone()
    where, size = parser._ws.data_ptr(), parser._ws.numel()
    second = parser.logits(frames[:1])
    assert parser._ws.data_ptr() == where and parser._ws.numel() == size
    assert tuple(first.shape) == (3, 19, 8, 8) and float(second.abs().max()) > 0
    assert torch.equal(first, FaceParser(g14_weights, "cuda", max_batch=2).logits(frames))
    assert torch.equal(second, FaceParser(g14_weights, "cuda", max_batch=2).logits(frames[:1]))


def test_two_calls_same_bits(g14, g14_weights):
    from instag_amd.parsing import FaceParser
    frames = torch.from_numpy(g14["frame"])[None].cuda()
    parser = FaceParser(g14_weights, "cuda")
    first = parser.logits(frames).clone()
    colours = parser.parse(frames).clone()
    assert float(first.abs().max()) > 0
    assert torch.equal(first, parser.logits(frames)) and torch.equal(colours, parser.parse(frames))
    other = FaceParser(g14_weights, "cuda")
    assert torch.equal(first, other.logits(frames)) and torch.equal(colours, other.parse(frames))


def test_argument_errors(g14_weights):
    from instag_amd.parsing import FaceParser
    parser = FaceParser(g14_weights, "cuda")
    for shape in ((1, 64, 80, 3), (1, 32, 64, 3)):
        with pytest.raises(ValueError, match="multiples of 32"):
            parser.parse(torch.zeros(shape, dtype=torch.uint8))


def test_parse_feeds_gt_and_torso(g14_weights):
    """parse's output goes into gt_and_torso on the device; against parse_torch's output: gt (pointwise in the parsing
    map) is equal wherever the two maps agree, gt and torso are equal for every frame whose maps agree everywhere."""
    from instag_amd import prepare
    from instag_amd.parsing import FaceParser, parse_torch
    frames = H.seeded_frames(3, 64, 64, seed=21)
    bc = H.seeded_frames(1, 64, 64, seed=22)[0]
    par_h = FaceParser(g14_weights, "cuda").parse(frames.cuda())
    par_t = parse_torch(g14_weights, frames)
    assert par_h.is_cuda and par_h.dtype == par_t.dtype == torch.uint8 and tuple(par_h.shape) == tuple(par_t.shape)
    agree = (par_h.cpu() == par_t).all(dim=-1)
    print(f"parsing maps agree on {100 * float(agree.double().mean()):.3f} % of the pixels")
    assert float(agree.double().mean()) >= 1.0 - MAX_LEFT_OUT
    gt_h, torso_h = prepare.gt_and_torso(frames.cuda(), par_h, bc.cuda())
    gt_t, torso_t = prepare.gt_and_torso(frames.cuda(), par_t.cuda(), bc.cuda())
    assert gt_h.is_cuda and gt_h.dtype == torch.uint8 and tuple(gt_h.shape) == (3, 64, 64, 3)
    assert torso_h.dtype == torch.uint8 and tuple(torso_h.shape) == (3, 64, 64, 4)
    assert torch.equal(gt_h.cpu()[agree], gt_t.cpu()[agree])
    for f in range(3):
        if bool(agree[f].all()):
            assert torch.equal(gt_h[f], gt_t[f]) and torch.equal(torso_h[f], torso_t[f])
