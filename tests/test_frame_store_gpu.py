"""GPU: csrc/frames.hip against the plain-torch statements of instag_amd.frame_store.  Every comparison is for exact
equality: every output is a copy, an integer, or a single correctly rounded operation."""
import random

import numpy as np
import pytest
import torch

from instag_amd import frame_store as FS
from tests import frame_store_helpers as H

pytestmark = pytest.mark.gpu
T = 12
AUDIO_INDICES = (0, 1, 3, 4, T - 4, T - 3, T - 1, T)     # T: the last window the reference accepts


def test_ingest_composite_all_triples():
    """The 256^3 (torso, alpha, bc) triples as one [1,4096,4096] frame."""
    torso, bc = H.triples()
    zeros3 = np.zeros((1, 4096, 4096, 3), dtype=np.uint8)
    store = FS.FrameStore("cuda")
    store.append(zeros3, torso[None], bc, zeros3, zeros3[..., 0], H.cameras(1, 4096, 4096), torch.zeros(1, 6),
                 torch.zeros(1, 4, dtype=torch.int32), [0])
    got = store.planes()[1][0].cpu()
    z1 = torch.zeros(1, 256, 4096, dtype=torch.uint8)
    z3 = z1[..., None].expand(1, 256, 4096, 3)
    bad = 0
    for r in range(0, 4096, 256):                 # (the statement in slabs: its fp64 temporaries stay small)
        rows = slice(r, r + 256)
        _, want, _, _ = FS.ingest_torch(z3, torch.from_numpy(torso[rows])[None], torch.from_numpy(bc[rows]), z3, z1)
        bad += int((got[rows] != want[0]).sum())
    assert bad == 0, f"{bad} of 3 * 256^3 composite bytes differ"
    assert store.counts.tolist() == [[0, 4096 * 4096, 0]]        # parsing all black = hair


@pytest.mark.parametrize("shape", H.SHAPES)
def test_ingest_masks_and_counts(shape):
    raw = H.raw_frames(3, *shape, seed=7)
    store = FS.FrameStore("cuda")
    store.append(raw["gt"], raw["torso"], raw["bc"], raw["parsing"], raw["teeth"], H.cameras(3, *shape),
                 torch.zeros(3, 6), torch.zeros(3, 4, dtype=torch.int32), [0, 0, 0])
    want = FS.ingest_torch(*(torch.from_numpy(raw[k]) for k in ("gt", "torso", "bc", "parsing", "teeth")))
    for name, g, w in zip(("rgb", "bg", "mask"), store.planes(), want):
        assert torch.equal(g.cpu(), w), name
    assert torch.equal(store.counts, want[3]) and int(want[3][1, 2]) == 0 and int(want[3][:, 2].sum()) > 0
    # nothing but the planes is written: the padding behind each plane of each frame is still zero
    HW = shape[0] * shape[1]
    buf = store.chunks[0].buf.cpu().view(3, -1)
    P3 = FS._pad256(HW * 3)
    assert not buf[:, HW * 3:P3].any() and not buf[:, P3 + HW * 3:2 * P3].any() and not buf[:, 2 * P3 + HW:].any()


@pytest.mark.parametrize("layout", ["face", "fuse", "face+priors"])
@pytest.mark.parametrize("shape", H.SHAPES)
def test_unpack_writes_the_tensors_and_nothing_else(shape, layout):
    """Every frame of an 8-frame store (two batches; the last frame included), one audio index each, both table shapes,
    into a packed frame pre-filled with 0xA5 == the CPU store's statement, byte for byte, padding included."""
    priors, background = layout == "face+priors", layout == "fuse"
    F = len(AUDIO_INDICES)
    for C, L in ((29, 16), (1, 512)):
        audio = H.audio_table(T, C, L, 3)
        dev_store, _ = H.build_store("cuda", F, *shape, 11, AUDIO_INDICES, audio, priors=priors, split=3)
        cpu_store, _ = H.build_store("cpu", F, *shape, 11, AUDIO_INDICES, audio, priors=priors, split=3)
        static = dev_store.empty_frame(background, priors)
        ref = cpu_store.empty_frame(background, priors)
        assert static._layout == ref._layout and len(static._layout) == 10 + background + 2 * priors
        offs, total = FS._offsets(ref._layout)
        inside = torch.zeros(total, dtype=torch.bool)
        for (k, s, d), o in zip(ref._layout, offs):
            inside[o:o + FS._nbytes(s, d)] = True
        assert int((~inside).sum()) > 0
        for i in (F - 1,) + tuple(range(F - 1)):
            static._buf.fill_(0xA5)
            ref._buf.fill_(0xA5)
            dev_store.unpack_into(static, i)
            cpu_store.unpack_into(ref, i)
            got = static._buf.cpu()
            want = cpu_store.unpack_torch(i, background=background, priors=priors)
            for k in want:
                t = getattr(static, k) if k in type(static).TENSORS else static.talking_dict[k]
                assert t.dtype == want[k].dtype and torch.equal(t.cpu(), want[k]), (k, i, C)
            assert bool((got[~inside] == 0xA5).all()), (i, C)
            assert torch.equal(got, ref._buf), (i, C)


def _params(tr):
    return [p.detach().clone() for p in tr._all_params()]


def test_trainer_steps_from_the_store_match_materialised_frames():
    """Three sampled steps eager, then three replayed, fed with store.ref(i) == the same steps fed with make_frame of
    the torch statement: bit-identical loss and parameters."""
    from instag_amd import diff_gauss
    from instag_amd.scene_synth import toy_cameras
    from instag_amd.train import build_trainer, make_frame
    dev = torch.device("cuda")
    F, size = 4, 64
    store = H.synthetic_store(dev, F, size)
    cpu_store = H.synthetic_store("cpu", F, size)
    cams = [c.to(dev) for c in toy_cameras(size, F)]
    frames = []
    for i in range(F):
        s = cpu_store.unpack_torch(i, background=False)
        frames.append(make_frame(cams[i], dict({k: v.to(dev) for k, v in s.items()}, gt_image=s["original_image"].to(dev))))
        assert frames[i]._layout == store.layout()
    runs = {}
    try:
        for mode in ("stored", "materialised"):
            feed = (lambda i: store.ref(i, background=False)) if mode == "stored" else (lambda i: frames[i])
            tr = build_trainer(2000, dev, seed=3)
            rng = random.Random(0)
            losses = [tr.step(feed(rng.randrange(F)))["loss"].clone() for _ in range(3)]
            eager = _params(tr)
            tr.enable_graph(feed(0), warmup_steps=1)
            for _ in range(3):
                losses.append(tr.step(feed(rng.randrange(F)))["loss"].clone())
                assert tr._graph is not None
            runs[mode] = (losses, eager, _params(tr))
            diff_gauss.set_capacity_plan(None)
    finally:
        diff_gauss.set_capacity_plan(None)
    (la, ea, ga), (lb, eb, gb) = runs["stored"], runs["materialised"]
    assert all(torch.isfinite(x) for x in la)
    for k, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), (k, float(x), float(y))
    assert all(torch.equal(x, y) for x, y in zip(ea, eb)) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert not all(torch.equal(x, y) for x, y in zip(ea, ga))                 # the replayed steps trained on


def test_fuse_renderer_on_a_stored_frame():
    from types import SimpleNamespace
    from instag_amd import diff_gauss
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.infer import FuseRenderer
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    dev = torch.device("cuda")
    torch.manual_seed(21)
    face_args = SimpleNamespace(audio_extractor="deepspeech", type="face")
    mouth_args = SimpleNamespace(audio_extractor="deepspeech", type="mouth")
    pc = GaussianModel(1, PersonalizedMotionNetwork(args=face_args).to(dev)).create_random(2000, dev, seed=1)
    pcm = GaussianModel(1, PersonalizedMotionNetwork(args=mouth_args).to(dev)).create_random(600, dev, seed=2)
    net, netm = MotionNetwork(args=face_args).to(dev), MouthMotionNetwork(args=mouth_args).to(dev)
    store = H.synthetic_store(dev, 3, 64)
    frames = [store.frame(i) for i in range(3)]
    r = FuseRenderer(pc, net, pcm, netm, torch.zeros(3, device=dev))
    try:
        for graph in (False, True):
            if graph:
                r.enable_graph(store.ref(0))
            for i in (2, 0, 1):
                sb = frames[i].talking_dict["background"]
                want = r.render(frames[i], sb).clone()
                got = r.render(store.ref(i), sb).clone()
                assert torch.equal(got, want), (graph, i)
            assert not torch.equal(r.render(store.ref(0), sb), want)
    finally:
        r.close()
        diff_gauss.set_capacity_plan(None)
