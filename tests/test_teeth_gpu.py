"""GPU tests of the teeth segmenter (csrc/teeth.hip) against golden G15 and the fp64 CPU statement: the three frame
sizes at which the tiling differs, the final stage alone, chunking and determinism bit for bit, and the chain into the
frame store.

Logits: e32 = max|fp32 torch statement on the CPU - fp64| / max|fp64| is measured on each case's own frames, and the
operator must be within 8 x e32 of the fp64 logits at 1/4 resolution (relative to their largest entry) -- the bar of
test_parsing_gpu.py for the same arithmetic: fp32 MFMA, K-tiled sums (K <= 4608 here), BatchNorm folded into one scale
and shift.  Labels and mask: exactly the fp64 statement's, except at flip-risk pixels, which the fp64 statement alone
decides -- the top-two margin of its full-size logits is below 2 x 8 x e32 x scale; at most 1 % of a case's pixels may
be left out, and that share is asserted.  Every test prints the operator's error beside e32 and the bar before it
asserts.  Observed on an MI355X (profiles/teeth_parity.json): G15 e32 2.31e-6, operator 8.6e-7, left out
0 %; B = 3 at 96 x 64 e32 2.70e-6, operator 8.0e-7, left out 0.011 %; 512 x 512 e32 4.16e-6, operator 1.15e-6, left out
0.027 %; the chunked frames e32 3.07e-6, operator 8.1e-7; no label differed from the fp64 statement's in any case,
inside the left-out pixels or outside them, and the two masks fed to the frame store agreed on every pixel.
"""
import numpy as np
import pytest
import torch

from tests import teeth_helpers as H
from tests import segnet_helpers as S

pytestmark = pytest.mark.gpu

MAX_LEFT_OUT = 0.01


def _case(weights, frames):
    return S.case(H.reference_fp64, weights, frames)


_check_logits = S.check_logits


def _check_labels(name, labels, mask, c):
    share = float(c["risk"].double().mean())
    keep = ~c["risk"]
    labels, mask = labels.cpu(), mask.cpu()
    wrong = int((labels != c["labels"])[keep].sum())
    print(f"{name}: left out {100 * share:.4f} % of {keep.numel()} pixels, labels wrong outside them {wrong}, "
          f"wrong inside them {int((labels != c['labels'])[c['risk']].sum())}, distinct {len(torch.unique(c['labels']))}, "
          f"teeth {100 * float((c['labels'] == 7).double().mean()):.3f} %")
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == tuple(c["labels"].shape)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(c["labels"].shape)
    assert share <= MAX_LEFT_OUT, share
    assert wrong == 0
    assert torch.equal(mask[keep], (c["labels"] == 7).to(torch.uint8)[keep])
    assert torch.equal(mask, (labels == 7).to(torch.uint8))                  # the operator's mask is its labels'


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(f"{golden_dir}/g15_teeth.npz")


@pytest.fixture(scope="module")
def g15_weights():
    return H.weights()


@pytest.fixture(scope="module")
def other_weights():
    return H.weights(seed=3)


def test_g15(g15, g15_weights):
    """B = 1, 64 x 96: the stride-32 map is 2 x 3, every tile is an edge tile."""
    from instag_amd.teeth import TeethSegmenter
    frames = torch.from_numpy(g15["frame"])[None]
    c = _case(g15_weights, frames)
    golden = torch.from_numpy(g15["logits4"])[None]
    assert float((c["want"] - golden).abs().max()) <= 1e-9 * c["scale"]
    assert np.array_equal(c["labels"][0].numpy(), g15["labels"])
    seg = TeethSegmenter(g15_weights, "cuda")
    _check_logits("g15", seg.logits(frames), c)
    _check_labels("g15", seg.labels(frames), seg.mask(frames.cuda()), c)


def test_batch_of_three_transposed(other_weights):
    """B = 3, 96 x 64, other weights: the batch-joint m tiling (a tile spans frames) and the other aspect."""
    from instag_amd.teeth import TeethSegmenter
    frames = H.seeded_frames(3, 96, 64, seed=3)
    c = _case(other_weights, frames)
    seg = TeethSegmenter(other_weights, "cuda")
    _check_logits("B=3 96x64", seg.logits(frames), c)
    _check_labels("B=3 96x64", seg.labels(frames), seg.mask(frames), c)
    assert len(torch.unique(c["labels"])) >= 5


def test_real_size(g15_weights):
    """B = 1, 512 x 512: the size InsTaG runs at; the large tiles, many workgroups per layer."""
    from instag_amd.teeth import TeethSegmenter
    frames = H.seeded_frames(1, 512, 512, seed=7)
    c = _case(g15_weights, frames)
    seg = TeethSegmenter(g15_weights, "cuda")
    _check_logits("512x512", seg.logits(frames), c)
    _check_labels("512x512", seg.labels(frames), seg.mask(frames), c)


def test_final_stage_alone():
    """Crafted logits [1,8,16,24] for 64 x 96: every class wins somewhere, the mask is labels == 7, and two identical
    dominant planes give the first of them everywhere."""
    from instag_amd import teeth as T
    g = torch.Generator().manual_seed(5)
    h4, w4, Hh, Ww = 16, 24, 64, 96
    cells = torch.arange(h4 * w4).view(h4, w4)
    logits = (torch.rand(1, 8, h4, w4, generator=g) * 16).round() / 8                        # [0, 2] in eighths
    winner = (cells * 3 + cells // w4) % 8
    logits[0].scatter_(0, winner[None], 8.0 + (torch.rand(1, h4, w4, generator=g) * 16).round() / 8)
    full = T.upsample_torch(logits.double(), Hh, Ww)
    want = T.first_argmax(full)
    assert len(torch.unique(want)) == 8
    risk = H.top_two_margin(full) < 1e-5 * float(logits.abs().max())   # fp32 interpolation: a few ulp of the scale
    share = float(risk.double().mean())
    labels, mask = T.teeth_labels(logits.cuda(), Hh, Ww, want_mask=True)
    print(f"final stage: left out {100 * share:.4f} %, wrong {int((labels.cpu() != want)[~risk].sum())}")
    assert labels.dtype == mask.dtype == torch.uint8 and tuple(labels.shape) == tuple(mask.shape) == (1, Hh, Ww)
    assert share <= MAX_LEFT_OUT
    assert torch.equal(labels.cpu()[~risk], want[~risk])
    assert len(torch.unique(labels)) == 8
    assert torch.equal(mask, (labels == 7).to(torch.uint8)) and 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(T.teeth_labels(logits.cuda(), Hh, Ww), labels)                        # labels alone

    tie = (torch.rand(1, 8, h4, w4, generator=g) * 16).round() / 8
    tie[0, 3] = 6.0 + (torch.rand(h4, w4, generator=g) * 16).round() / 8
    tie[0, 7] = tie[0, 3]
    labels, mask = T.teeth_labels(tie.cuda(), Hh, Ww, want_mask=True)
    assert bool((labels == 3).all()) and int(mask.sum()) == 0
    with pytest.raises(ValueError, match="logits"):
        T.teeth_labels(torch.zeros(1, 7, h4, w4, device="cuda"), Hh, Ww)


def test_chunking_bitwise(g15_weights):
    """max_batch + 1 frames at 64 x 64 in one call: rows 0, max_batch - 1 and max_batch equal single-frame calls."""
    from instag_amd.teeth import TeethSegmenter
    seg = TeethSegmenter(g15_weights, "cuda", max_batch=3)
    mb = seg.max_batch
    frames = H.seeded_frames(mb + 1, 64, 64, seed=11).cuda()
    logits, labels, mask = seg.logits(frames), seg.labels(frames), seg.mask(frames)
    assert tuple(logits.shape) == (mb + 1, 8, 16, 16) and tuple(mask.shape) == (mb + 1, 64, 64)
    single = TeethSegmenter(g15_weights, "cuda", max_batch=1)
    for i in (0, mb - 1, mb):
        assert torch.equal(seg.logits(frames[i:i + 1])[0], logits[i]), i
        assert torch.equal(single.logits(frames[i:i + 1])[0], logits[i]), i
        assert torch.equal(seg.labels(frames[i:i + 1])[0], labels[i]), i
        assert torch.equal(seg.mask(frames[i:i + 1])[0], mask[i]), i
    assert torch.equal(single.logits(frames), logits)
    assert not torch.equal(logits[0], logits[mb])
    pick = [0, mb - 1, mb]
    c = _case(g15_weights, frames[pick].cpu())
    _check_logits("chunked", logits[pick], c)


def test_two_calls_same_bits(g15, g15_weights):
    from instag_amd.teeth import TeethSegmenter
    frames = torch.from_numpy(g15["frame"])[None].cuda()
    seg = TeethSegmenter(g15_weights, "cuda")
    first = seg.logits(frames).clone()
    mask = seg.mask(frames).clone()
    assert float(first.abs().max()) > 0
    assert torch.equal(first, seg.logits(frames)) and torch.equal(mask, seg.mask(frames))
    other = TeethSegmenter(g15_weights, "cuda")
    assert torch.equal(first, other.logits(frames)) and torch.equal(mask, other.mask(frames))


def test_argument_errors(g15_weights):
    from instag_amd.teeth import TeethSegmenter
    seg = TeethSegmenter(g15_weights, "cuda")
    assert 1 <= seg.max_batch <= 8
    for shape in ((1, 64, 80, 3), (1, 32, 64, 3)):
        with pytest.raises(ValueError, match="multiples of 32"):
            seg.mask(torch.zeros(shape, dtype=torch.uint8))


def test_mask_feeds_the_frame_store(g15_weights):
    """mask's output goes into FrameStore.append / instag_frame_ingest on the device, beside teeth_torch's mask: the
    ingested planes and counts are equal for every frame whose two masks agree everywhere."""
    from instag_amd import frame_store as FS
    from instag_amd.teeth import TeethSegmenter, teeth_torch
    from tests import frame_store_helpers as FH
    frames = H.seeded_frames(3, 64, 64, seed=21)
    raw = FH.raw_frames(3, 64, 64, seed=9)
    m_h = TeethSegmenter(g15_weights, "cuda").mask(frames.cuda())
    m_t = teeth_torch(g15_weights, frames)
    assert m_h.is_cuda and m_h.dtype == m_t.dtype == torch.uint8 and tuple(m_h.shape) == tuple(m_t.shape) == (3, 64, 64)
    agree = m_h.cpu() == m_t
    print(f"teeth masks agree on {100 * float(agree.double().mean()):.3f} % of the pixels, "
          f"teeth {100 * float(m_t.double().mean()):.3f} %")
    assert float(agree.double().mean()) >= 1.0 - MAX_LEFT_OUT
    assert int(m_t.sum()) > 0

    def ingest(teeth):
        store = FS.FrameStore("cuda")
        store.append(raw["gt"], raw["torso"], raw["bc"], raw["parsing"], teeth, FH.cameras(3, 64, 64), torch.zeros(3, 6),
                     torch.zeros(3, 4, dtype=torch.int32), [0, 0, 0])
        return [p.cpu() for p in store.planes()], store.counts

    planes_h, counts_h = ingest(m_h)                                       # the device tensor as it is
    planes_t, counts_t = ingest(m_t.cuda())
    want = FS.ingest_torch(*(torch.from_numpy(raw[k]) for k in ("gt", "torso", "bc", "parsing")), m_h.cpu())
    for g, w in zip(planes_h, want):
        assert torch.equal(g, w)
    assert torch.equal(counts_h, want[3])
    whole = [f for f in range(3) if bool(agree[f].all())]
    for f in whole:
        for a, b in zip(planes_h, planes_t):
            assert torch.equal(a[f], b[f])
        assert torch.equal(counts_h[f], counts_t[f])
