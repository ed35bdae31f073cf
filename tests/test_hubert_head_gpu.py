"""GPU tests of the per-frame branch of a 'hubert' head: the instag_frame_code_wide_* operator against the fp64 CPU
modules and golden G18, its dead taps, misaligned tensors, determinism / arrival word / two-stream behaviour, the face,
mouth, fuse and pretrain-face steps and the fuse renderer on 'hubert' frames (eager, captured, and against the torch
branch), and a FrameStore that carries a [T, 1024, 2] table.

INSTAG_HUBERT_HEAD_PARITY_OUT=<file> writes every figure the parity tests print to that JSON file."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import hubert_head_helpers as H
from tests.test_ave_gpu import NoEncoder, _Opt, _audio_names, _audio_state, _single_workgroup

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 2e-5, 5e-5          # of test_glue_gpu.py::test_frame_codes_match_torch_modules
CONV_W = tuple(f"audio_net.encoder_conv.{i}.weight" for i in (0, 2, 4, 6))
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _record_figures():
    yield
    out = os.environ.get("INSTAG_HUBERT_HEAD_PARITY_OUT")
    if out and _FIGURES:
        with open(out, "w") as f:
            json.dump(_FIGURES, f, indent=1, sort_keys=True)


def _figure(a, b, name, floor=True):
    err = float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())
    peak = float(b.detach().abs().max())
    scale = max(1.0, peak) if floor else peak
    print(f"{name}: err {err:.3e} scale {scale:.3e} rel {err / scale:.3e}")
    _FIGURES[name] = dict(err=err, scale=scale, rel=err / scale)
    return err, scale


def _codes(net, a, e):
    if hasattr(net, "encode_frame"):
        return net.encode_frame(a, e)
    return net.encode_audio(a), None           # MouthMotionNetwork


def _reference_and_device(tag, dim_in=1024):
    """The fp64 CPU network (weights x 2, torch.manual_seed(3)) and its fp32 copy on the device."""
    from instag_amd.motion_net import AudioNet
    torch.manual_seed(3)
    ref, _ = H.build_network(tag, encoder_cls=NoEncoder)
    if dim_in != 1024:
        ref.audio_net = AudioNet(dim_in, 32)
    ref = ref.double()
    with torch.no_grad():
        for p in ref.parameters():             # biases and weights large enough to exercise both LeakyReLU sides
            p.mul_(2.0)
    return ref, copy.deepcopy(ref).float().cuda()


def _inputs(has_e, dim_in=1024):
    g = torch.Generator().manual_seed(7)
    a = torch.randn(8, dim_in, 2, generator=g)
    e = torch.rand(6, generator=g) if has_e else None
    return a, e, torch.randn(1, 32, generator=g), torch.randn(6, generator=g), g


def _scalar(enc_a, enc_e, wa, we):
    s = (enc_a * wa).sum()
    return s if enc_e is None else s + (enc_e * we).sum()


_REFERENCE = {}


def _reference_run(tag, dim_in=1024):
    """(reference network after backward, device copy before any call, inputs, reference outputs): computed once per
    (tag, dim_in), never modified."""
    key = (tag, dim_in)
    if key not in _REFERENCE:
        has_e = next(n[3] for n in H.NETWORKS if n[0] == tag)
        ref, dev = _reference_and_device(tag, dim_in)
        a, e, wa, we, g = _inputs(has_e, dim_in)
        enc_a_r, enc_e_r = _codes(ref, a.double(), None if e is None else e.double())
        _scalar(enc_a_r, enc_e_r, wa.double(), we.double()).backward()
        with torch.no_grad():                       # both sides of the four LeakyReLUs behind the convolutions occur
            x = a.double()
            for i in (0, 2, 4, 6):
                z = ref.audio_net.encoder_conv[i](x)
                pos, neg = float((z > 0).double().mean()), float((z < 0).double().mean())
                print(f"{tag} D={dim_in} encoder_conv.{i}: {pos:.2f} above zero, {neg:.2f} below")
                assert pos > 0.05 and neg > 0.05
                x = torch.nn.functional.leaky_relu(z, 0.02)
        _REFERENCE[key] = (ref, dev, (a, e, wa, we), (enc_a_r.detach(), None if enc_e_r is None else enc_e_r.detach()))
    ref, dev, inputs, outs = _REFERENCE[key]
    return ref, copy.deepcopy(dev), inputs, outs


def _compare(tag, form, dev, ref, inputs, outs, label):
    from instag_amd import audio as A
    a, e, wa, we = inputs
    has_e = e is not None
    ac, ec = a.cuda(), None if e is None else e.cuda()
    assert A.supported(dev, ac, ec)
    enc_a_h, enc_e_h = _codes(dev, ac, ec)
    _scalar(enc_a_h, enc_e_h, wa.cuda(), we.cuda()).backward()
    checks = [(_figure(enc_a_h, outs[0], f"{label}.enc_a"), FWD_TOL)]
    if has_e:
        checks.append((_figure(enc_e_h, outs[1], f"{label}.enc_e"), FWD_TOL))
    names = _audio_names(ref)
    assert len(names) == (26 if has_e else 24)
    pr, ph = dict(ref.named_parameters()), dict(dev.named_parameters())
    for n in names:
        assert ph[n].grad is not None, n
        checks.append((_figure(ph[n].grad, pr[n].grad, f"{label}.d_{n}"), GRAD_TOL))
        if n in CONV_W:                             # ... and against the tensor's own largest entry, unfloored
            checks.append((_figure(ph[n].grad, pr[n].grad, f"{label}.own.d_{n}", floor=False), GRAD_TOL))
    for (err, scale), tol in checks:                # every figure is printed before the first assertion
        assert err <= tol * scale, (label, err, scale, tol)
    return dev


@pytest.mark.parametrize("form", ["arrivals", "one-workgroup"])
@pytest.mark.parametrize("tag", [n[0] for n in H.NETWORKS])
def test_hubert_head_frame_codes_match_torch_modules(tag, form, monkeypatch, golden_dir):
    """The wide AudioNet + AudioAttNet + expression MLP as HIP kernels vs the nn.Module chain (fp64, CPU): enc_a,
    enc_e and every parameter gradient, in the split form (an arrival word) and the single-workgroup form; then the
    closed-form weights and the window of golden G18 against the reference's recorded enc_a."""
    from instag_amd import audio as A
    if form == "one-workgroup":
        _single_workgroup(monkeypatch)
    ref, dev, inputs, outs = _reference_run(tag)
    _compare(tag, form, dev, ref, inputs, outs, f"{tag}.{form}")
    table = dev.__dict__.get("_frame_code_arrivals", {})
    device = torch.device("cuda", torch.cuda.current_device())
    if form == "arrivals":
        assert int(table[device][0].abs().sum()) == 0 and len(table[device][1]) == 1
    else:
        assert all(len(slots) == 0 for _, slots in table.values())

    g18 = np.load(f"{golden_dir}/g18_hubert_head.npz")
    net, salt = H.build_network(tag, encoder_cls=NoEncoder)
    net = H.load_closed_form(net, salt).cuda()
    a18 = torch.from_numpy(g18["a"].astype(np.float32)).cuda()
    e18 = torch.rand(6).cuda() if inputs[1] is not None else None
    assert A.supported(net, a18, e18)
    with torch.no_grad():
        got = _codes(net, a18, e18)[0]
    err, scale = _figure(got, torch.from_numpy(g18[f"{tag}.enc_a"]), f"{tag}.{form}.g18.enc_a")
    assert err <= FWD_TOL * scale


@pytest.mark.parametrize("form", ["arrivals", "one-workgroup"])
@pytest.mark.parametrize("dim_in", [256, 768])
def test_hubert_head_frame_codes_at_one_and_three_chunks(dim_in, form, monkeypatch):
    """dim_in = 256 and 768 (one and three chunks of 4 channels x 64 lanes) on the universal field with
    AudioNet(dim_in, 32) in audio_net's place."""
    if form == "one-workgroup":
        _single_workgroup(monkeypatch)
    ref, dev, inputs, outs = _reference_run("umf", dim_in)
    assert tuple(dev.audio_net.encoder_conv[0].weight.shape) == (128, dim_in, 3)
    _compare("umf", form, dev, ref, inputs, outs, f"umf.D{dim_in}.{form}")


def test_hubert_head_dead_taps_are_written_as_zeros():
    """Every gradient element is written: freed NaN-filled blocks of the gradients' sizes sit in the allocator's cache
    when backward allocates with empty_like.  The taps that only meet padding get exactly 0.0, as torch gives."""
    ref, dev, inputs, outs = _reference_run("umf")
    a, e, wa, we = inputs
    enc_a, enc_e = _codes(dev, a.cuda(), e.cuda())
    loss = _scalar(enc_a, enc_e, wa.cuda(), we.cuda())
    names = _audio_names(dev)
    params = dict(dev.named_parameters())
    for _ in range(2):
        junk = [torch.full_like(params[n], float("nan")) for n in names]
        torch.cuda.synchronize()
        del junk
    loss.backward()
    for n in names:
        assert bool(torch.isfinite(params[n].grad).all()), n
    g1 = params[CONV_W[0]].grad
    assert int(torch.count_nonzero(g1[:, :, 0])) == 0
    assert int(torch.count_nonzero(g1[:, :, 1])) > g1[:, :, 1].numel() // 2
    assert int(torch.count_nonzero(g1[:, :, 2])) > g1[:, :, 2].numel() // 2
    for n in CONV_W[1:]:
        gw = params[n].grad
        assert int(torch.count_nonzero(gw[:, :, 0])) == 0 and int(torch.count_nonzero(gw[:, :, 2])) == 0, n
        assert int(torch.count_nonzero(gw[:, :, 1])) > gw[:, :, 1].numel() // 2, n


def test_hubert_head_misaligned_conv1_weight(monkeypatch):
    """encoder_conv.0.weight at a 4-byte offset inside a larger storage, and its gradient too: the 4-byte access paths
    of both passes, same bounds."""
    ref, dev, inputs, outs = _reference_run("pmf_face")
    w = dev.audio_net.encoder_conv[0].weight
    store = torch.zeros(w.numel() + 8, device="cuda")
    base = 1 if store.data_ptr() % 16 == 0 else 0
    while (store.data_ptr() + 4 * base) % 16 == 0:
        base += 1
    with torch.no_grad():
        store[base:base + w.numel()].copy_(w.detach().reshape(-1))
    dev.audio_net.encoder_conv[0].weight = torch.nn.Parameter(store[base:base + w.numel()].view_as(w))
    assert dev.audio_net.encoder_conv[0].weight.data_ptr() % 16 != 0
    assert dev.audio_net.encoder_conv[0].weight.is_contiguous()
    # ... and its gradient likewise: backward's empty_like of that one shape hands out a misaligned view
    real, seen = torch.empty_like, []

    def empty_like(t, *args, **kw):
        if tuple(t.shape) != tuple(w.shape):
            return real(t, *args, **kw)
        big = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
        off = next(o for o in range(1, 5) if (big.data_ptr() + 4 * o) % 16 != 0)
        seen.append(big[off:off + t.numel()].view_as(t))
        return seen[-1]

    monkeypatch.setattr(torch, "empty_like", empty_like)
    _compare("pmf_face", "arrivals", dev, ref, inputs, outs, "pmf_face.misaligned")
    assert len(seen) == 1 and seen[0].data_ptr() % 16 != 0


def _run_twice(net, a, e, wa):
    outs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        enc_a, enc_e = net.encode_frame(a, e)
        ((enc_a * wa).sum() + enc_e.sum()).backward()
        outs.append([enc_a.detach().clone(), enc_e.detach().clone()]
                    + [p.grad.detach().clone() for n, p in net.named_parameters() if n in _audio_names(net)])
    return outs


def test_hubert_head_frame_codes_deterministic_and_arrival_word_zero():
    """Two forward + backward runs give the same bits in every output and gradient; the arrival word reads zero after
    each call."""
    torch.manual_seed(5)
    net = H.build_network("umf", encoder_cls=NoEncoder)[0].cuda()
    a, e, wa = torch.randn(8, 1024, 2).cuda(), torch.rand(6).cuda(), torch.randn(1, 32).cuda()
    first, second = _run_twice(net, a, e, wa)
    assert len(first) == 28
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    words, slots = net.__dict__["_frame_code_arrivals"][a.device]
    assert len(slots) == 1 and int(words.abs().sum()) == 0
    assert all(float(t.abs().max()) > 0 for t in first)


def test_hubert_head_frame_codes_overlap_on_two_streams():
    """Two networks' forwards on two streams with two arrival words: each equals its stand-alone result bit for bit."""
    from instag_amd import _lib
    torch.manual_seed(6)
    dev = torch.device("cuda")
    nets = [H.build_network(t, encoder_cls=NoEncoder)[0].cuda() for t in ("umf", "pmf_face")]
    a, e = torch.randn(8, 1024, 2).cuda(), torch.rand(6).cuda()
    with torch.no_grad():
        alone = [n.encode_frame(a, e) for n in nets]
        torch.cuda.synchronize()
        streams = [_lib.side_stream(dev, ("hubert_head_test", i)) for i in range(2)]
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        both = [[], []]
        for _ in range(8):                            # interleaved launches: the two branches overlap on the device
            for i, (n, s) in enumerate(zip(nets, streams)):
                with torch.cuda.stream(s):
                    both[i].append(n.encode_frame(a, e))
        torch.cuda.synchronize()
    for i, n in enumerate(nets):
        for enc_a, enc_e in both[i]:
            assert torch.equal(enc_a, alone[i][0]) and torch.equal(enc_e, alone[i][1])
        words, slots = n.__dict__["_frame_code_arrivals"][a.device]
        assert len(slots) == 2 and int(words.abs().sum()) == 0     # the default stream's word and the side stream's
    assert not torch.equal(alone[0][0], alone[1][0])


# ---- trainers and the renderer on 'hubert' frames --------------------------------------------------------------------
# the smallest scene of test_stages_gpu.py: 96 x 96 images, 2000 face / 900 mouth Gaussians


def _frames(n, dev, **kw):
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    from instag_amd.train import make_frame
    cams = toy_cameras(96)
    frames = [make_frame(cams[i].to(dev), synthetic_frame(96, i, dev, audio_extractor="hubert", **kw)) for i in range(n)]
    assert tuple(frames[0].talking_dict["auds"].shape) == (8, 1024, 2)
    return frames


def _nets(dev, seed, n_face=2000, n_mouth=900):
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    torch.manual_seed(seed)
    fa, ma = H.hubert_args("face"), H.hubert_args("mouth")
    pc_face = GaussianModel(1, PersonalizedMotionNetwork(args=fa).to(dev)).create_random(n_face, dev, seed=1)
    face_net = MotionNetwork(args=fa).to(dev)
    pc = GaussianModel(1, PersonalizedMotionNetwork(args=ma).to(dev)).create_random(n_mouth, dev, seed=2)
    net = MouthMotionNetwork(args=ma).to(dev)
    return pc_face, face_net, pc, net


def _trainer(kind, dev, seed=7):
    from instag_amd.train import build_trainer
    from instag_amd.train_stages import FuseTrainer, MouthTrainer
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    if kind == "face":
        return build_trainer(2000, dev, seed=seed, densify=False, audio_extractor="hubert")
    pc_face, face_net, pc_mouth, mouth_net = _nets(dev, seed)
    if kind == "mouth":
        return MouthTrainer(pc_mouth, mouth_net, pc_face, face_net, bg, opt=_Opt, densify=False, seed=3, warm_step=0,
                            bg_iter=1000)
    return FuseTrainer(pc_face, face_net, pc_mouth, mouth_net, bg, opt=_Opt)


@pytest.mark.parametrize("kind", ["face", "mouth", "fuse"])
def test_hubert_head_trainers_graph_matches_eager(kind):
    """The face, mouth and fuse steps on 'hubert' frames: a few eager steps == the same steps replayed from a hipGraph
    (the tolerance of test_ave_trainers_graph_matches_eager); the audio net's parameters move where the stage trains
    the field (the fuse stage freezes both fields)."""
    from instag_amd import audio as A, diff_gauss
    dev = torch.device("cuda")
    frames = _frames(3, dev, background=True)

    def run(graph):
        tr = _trainer(kind, dev)
        td = frames[0].talking_dict
        assert A.supported(tr.motion_net, td["auds"], td["au_exp"] if getattr(tr.motion_net, "exp_eye", False) else None)
        before = _audio_state(tr)
        try:
            if graph:
                tr.enable_graph(frames[0], warmup_steps=2)          # 4 real steps on frame 0
                assert tr.iteration == 4 and tr._graph is not None
            else:
                for _ in range(4):
                    tr.step(frames[0])
            losses = [float(tr.step(frames[i % 3])["loss"]) for i in range(3)]
            if graph:
                assert tr._graph is not None
        finally:
            diff_gauss.set_capacity_plan(None)
        moved = not torch.equal(before, _audio_state(tr))
        vec = torch.cat([tr.g._p["f_dc"].detach().reshape(-1), tr.g._p["opacity"].detach().reshape(-1),
                         tr.g._p["xyz"].detach().reshape(-1), _audio_state(tr)])
        return losses, vec, moved

    le, ve, moved_e = run(False)
    lg, vg, moved_g = run(True)
    assert moved_e == moved_g == (kind != "fuse")
    for a_, b_ in zip(le, lg):
        assert abs(a_ - b_) <= 1e-4 * max(1.0, abs(a_)), (kind, le, lg)
    assert float((ve - vg).abs().max()) <= 2e-4, kind


def _operator_then_torch(one, monkeypatch):
    """one() with the HIP operator answering, then with audio.supported patched to False."""
    from instag_amd import audio as A
    calls = []
    real = A.frame_codes
    monkeypatch.setattr(A, "frame_codes", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with_operator = one()
    assert calls                                           # the HIP operator answered
    monkeypatch.setattr(A, "supported", lambda *a, **k: False)
    n_calls = len(calls)
    with_torch = one()
    assert len(calls) == n_calls                           # ... and the torch modules the second time
    return with_operator, with_torch


def _audio_grads(net):
    names = [n for n in _audio_names(net) if not n.startswith("exp_encode_net")]
    return {n: p.grad.detach().clone() for n, p in net.named_parameters() if n in names and p.grad is not None}


def _same_step(kind, with_operator, with_torch, n_grads):
    (loss_h, grads_h), (loss_t, grads_t) = with_operator, with_torch
    assert abs(loss_h - loss_t) <= 2e-6 * max(1.0, abs(loss_t)), (loss_h, loss_t)
    assert set(grads_h) == set(grads_t) and len(grads_h) == n_grads
    for n in grads_t:
        scale = float(grads_t[n].abs().max())
        err = float((grads_h[n] - grads_t[n]).abs().max())
        print(f"{kind} {n}: err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-4 * scale + 1e-9, (n, err, scale)


@pytest.mark.parametrize("kind", ["face", "mouth", "fuse"])
def test_hubert_head_step_matches_torch_branch(kind, monkeypatch):
    """One step's loss and audio-net gradients with the HIP operator == the same step with audio.supported patched to
    False (the torch modules answer); the bounds of test_ave_step_matches_torch_branch."""
    from instag_amd.train_stages import mouth_phase
    dev = torch.device("cuda")
    frame = _frames(1, dev, background=True)[0]

    def one():
        tr = _trainer(kind, dev, seed=9)
        if kind == "face":
            _, loss, _ = tr._forward_backward(frame)
        elif kind == "mouth":
            _, loss, _ = tr.forward(frame, mouth_phase(4, _Opt, 3, 10), k=12)
            loss.backward()
        else:
            _, loss, _ = tr.forward(frame)
            loss.backward()
        torch.cuda.synchronize()
        return float(loss), _audio_grads(tr.motion_net)

    _same_step(kind, *_operator_then_torch(one, monkeypatch), n_grads=0 if kind == "fuse" else 24)


def test_hubert_head_pretrain_face_step_matches_torch_branch(monkeypatch):
    """One pretrain-face step (two identities, the phase with every term) with the operator == with the torch branch."""
    from instag_amd.pretrain import build_pretrainer, pretrain_phase
    from tests.test_pretrain_gpu import PreOpt
    dev = torch.device("cuda")
    frame = _frames(1, dev)[0]
    phase = pretrain_phase(3001, 3, PreOpt)
    assert phase.motion and phase.warm

    def one():
        tr = build_pretrainer(2, 2000, dev, seed=2, opt=PreOpt, audio_extractor="hubert")
        _, loss, _ = tr._forward_backward(1, frame, phase)
        torch.cuda.synchronize()
        return float(loss.detach()), _audio_grads(tr.motion_net)

    _same_step("pretrain", *_operator_then_torch(one, monkeypatch), n_grads=24)


def test_hubert_head_fuse_inference_matches_torch_branch(monkeypatch):
    """FuseRenderer on one 'hubert' frame, eager and from a hipGraph, == the render with the torch modules answering
    the per-frame branch (2e-6, the bound of test_fuse_inference_matches_plain_torch)."""
    from instag_amd import audio as A, diff_gauss
    from instag_amd.infer import FuseRenderer
    dev = torch.device("cuda")
    pc, net, pcm, netm = _nets(dev, 21, n_face=3000, n_mouth=800)
    with torch.no_grad():
        for mod in (net.sigma_net, netm.sigma_net, pc.neural_motion_grid.sigma_net, pc.neural_motion_grid.align_net,
                    pcm.neural_motion_grid.sigma_net, pcm.neural_motion_grid.align_net):
            mod.net[-1].weight.mul_(30.0)
    frames = _frames(2, dev)
    bg = torch.zeros(3, device=dev)
    scene_bg = torch.rand(3, 96, 96, device=dev)
    r = FuseRenderer(pc, net, pcm, netm, bg, personalized=True)
    try:
        with monkeypatch.context() as m:
            m.setattr(A, "supported", lambda *a, **k: False)
            want = [r.render(f, scene_bg).clone() for f in frames]
        assert float((want[0] - want[1]).abs().max()) > 1e-2               # the audio window shapes the image
        assert A.supported(net, frames[0].talking_dict["auds"], frames[0].talking_dict["au_exp"])
        eager = r.render(frames[0], scene_bg).clone()
        r.enable_graph(frames[1])
        graphed = r.render(frames[0], scene_bg).clone()
        assert not r.check_overflow()
    finally:
        r.close()
        diff_gauss.set_capacity_plan(None)
    assert float((eager - want[0]).abs().max()) <= 2e-6
    assert float((graphed - want[0]).abs().max()) <= 2e-6


def test_hubert_head_frame_store_carries_the_table():
    """A FrameStore with an [11, 1024, 2] table: store.ref(i) carries the window audio_window cuts, at the table's
    start, inside it and one past its end; a face trainer's operator takes it."""
    from instag_amd import audio as A
    from instag_amd.frame_store import audio_window
    from instag_amd.train import build_trainer
    from tests import frame_store_helpers as FH
    dev = torch.device("cuda")
    table = FH.audio_table(11, 1024, 2, 3)
    indices = (0, 5, 11)
    store, _ = FH.build_store(dev, len(indices), 16, 16, 11, indices, table)
    tr = build_trainer(500, dev, seed=1, audio_extractor="hubert")
    for i, index in enumerate(indices):
        auds = store.ref(i).talking_dict["auds"]
        want = audio_window(table, index)
        assert tuple(auds.shape) == (8, 1024, 2) and torch.equal(auds.cpu(), want)
        assert A.supported(tr.motion_net, auds, store.ref(i).talking_dict["au_exp"])
    assert int(torch.count_nonzero(audio_window(table, 11)[4:])) == 0 and int(torch.count_nonzero(audio_window(table, 0)[:4])) == 0
