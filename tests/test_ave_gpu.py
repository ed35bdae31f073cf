"""GPU tests of the 'ave' audio extractor: the instag_frame_code_ave_* operator against the fp64 CPU modules and
golden G8, its determinism / arrival word / two-stream behaviour, and the face, mouth and fuse trainers and the fuse
renderer on 'ave' frames (eager, captured, and against the torch branch)."""
import copy

import numpy as np
import pytest
import torch

from tests import ave_helpers as H

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 2e-5, 5e-5          # of test_glue_gpu.py::test_frame_codes_match_torch_modules


class NoEncoder(torch.nn.Module):          # the tri-plane encoders play no part in the per-frame branch
    def __init__(self, **kw):
        super().__init__()
        self.output_dim = 12


def _close(a, b, name, tol):
    err = float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())
    scale = max(1.0, float(b.detach().abs().max()))
    print(f"{name}: err {err:.3e} scale {scale:.3e} rel {err / scale:.3e}")
    assert err <= tol * scale, f"{name}: err {err} scale {scale}"


def _single_workgroup(monkeypatch):
    """frame_codes() with no arrival word to hand out: the single-workgroup forward."""
    from instag_amd import audio as A
    monkeypatch.setattr(A, "_ARRIVAL_SLOTS", 0)


def _audio_names(net):
    return [n for n, _ in net.named_parameters() if n.startswith(("audio_net", "audio_att_net", "exp_encode_net"))]


@pytest.mark.parametrize("form", ["arrivals", "one-workgroup"])
@pytest.mark.parametrize("tag", [n[0] for n in H.NETWORKS])
def test_ave_frame_codes_match_torch_modules(tag, form, monkeypatch, golden_dir):
    """AudioNet_ave + AudioAttNet + expression MLP as HIP kernels vs the nn.Module chain (fp64, CPU): enc_a, enc_e and
    every parameter gradient, in the split form (an arrival word) and the single-workgroup form; then the closed-form
    weights and the window of golden G8 against the reference's recorded enc_a."""
    from instag_amd import audio as A
    if form == "one-workgroup":
        _single_workgroup(monkeypatch)
    has_e = next(n[3] for n in H.NETWORKS if n[0] == tag)
    torch.manual_seed(3)
    ref, salt = H.build_network(tag, encoder_cls=NoEncoder)
    ref = ref.double()
    with torch.no_grad():
        for p in ref.parameters():             # biases and weights large enough to exercise both LeakyReLU sides
            p.mul_(2.0)
    dev = copy.deepcopy(ref).float().cuda()
    g = torch.Generator().manual_seed(7)
    a = torch.randn(8, 1, 512, generator=g)
    e = torch.rand(6, generator=g) if has_e else None
    wa, we = torch.randn(1, 32, generator=g), torch.randn(6, generator=g)

    def codes(net, a_, e_):
        if hasattr(net, "encode_frame"):
            return net.encode_frame(a_, e_)
        return net.encode_audio(a_), None           # MouthMotionNetwork

    def scalar(enc_a, enc_e, wa_, we_):
        s = (enc_a * wa_).sum()
        return s + (enc_e * we_).sum() if has_e else s

    enc_a_r, enc_e_r = codes(ref, a.double(), None if e is None else e.double())
    scalar(enc_a_r, enc_e_r, wa.double(), we.double()).backward()
    with torch.no_grad():
        z1 = ref.audio_net.encoder_fc1[0](a.double())
        z2 = ref.audio_net.encoder_fc1[2](torch.nn.functional.leaky_relu(z1, 0.02))
    for t in (z1, z2):                         # both sides of both LeakyReLUs occur
        assert float((t > 0).double().mean()) > 0.05 and float((t < 0).double().mean()) > 0.05
    assert A.supported(dev, a.cuda(), None if e is None else e.cuda())
    enc_a_h, enc_e_h = codes(dev, a.cuda(), None if e is None else e.cuda())
    scalar(enc_a_h, enc_e_h, wa.cuda(), we.cuda()).backward()
    _close(enc_a_h, enc_a_r, "enc_a", FWD_TOL)
    if has_e:
        _close(enc_e_h, enc_e_r, "enc_e", FWD_TOL)
    names = _audio_names(ref)
    assert len(names) == (20 if has_e else 18)
    pr, ph = dict(ref.named_parameters()), dict(dev.named_parameters())
    for n in names:
        assert ph[n].grad is not None, n
        _close(ph[n].grad, pr[n].grad, "d_" + n, GRAD_TOL)
    table = dev.__dict__.get("_frame_code_arrivals", {})
    if form == "arrivals":
        assert int(table[a.cuda().device][0].abs().sum()) == 0 and len(table[a.cuda().device][1]) == 1
    else:
        assert all(len(slots) == 0 for _, slots in table.values())

    # golden G8: the reference's fp64 enc_a on the closed-form weights
    g8 = np.load(f"{golden_dir}/g8_ave_nets.npz")
    net, salt = H.build_network(tag, encoder_cls=NoEncoder)
    net = H.load_closed_form(net, salt).cuda()
    a8 = torch.from_numpy(g8["a"].astype(np.float32)).cuda()
    e8 = torch.rand(6, generator=g).cuda() if has_e else None
    assert A.supported(net, a8, e8)
    with torch.no_grad():
        got = codes(net, a8, e8)[0]
    _close(got, torch.from_numpy(g8[f"{tag}.enc_a"]), "g8.enc_a", FWD_TOL)


def _run_twice(net, a, e, wa):
    outs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        enc_a, enc_e = net.encode_frame(a, e)
        ((enc_a * wa).sum() + enc_e.sum()).backward()
        outs.append([enc_a.detach().clone(), enc_e.detach().clone()]
                    + [p.grad.detach().clone() for n, p in net.named_parameters() if n in _audio_names(net)])
    return outs


def test_ave_frame_codes_deterministic_and_arrival_word_zero():
    """Two forward + backward runs give the same bits in every output and gradient; the arrival word reads zero after
    each call."""
    torch.manual_seed(5)
    net = H.build_network("umf", encoder_cls=NoEncoder)[0].cuda()
    a, e, wa = torch.randn(8, 1, 512).cuda(), torch.rand(6).cuda(), torch.randn(1, 32).cuda()
    first, second = _run_twice(net, a, e, wa)
    assert len(first) == 22
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    words, slots = net.__dict__["_frame_code_arrivals"][a.device]
    assert len(slots) == 1 and int(words.abs().sum()) == 0
    assert all(float(t.abs().max()) > 0 for t in first)


def test_ave_frame_codes_overlap_on_two_streams():
    """Two networks' forwards on two streams with two arrival words: each equals its stand-alone result bit for bit."""
    from instag_amd import _lib
    torch.manual_seed(6)
    dev = torch.device("cuda")
    nets = [H.build_network(t, encoder_cls=NoEncoder)[0].cuda() for t in ("umf", "pmf_face")]
    a, e = torch.randn(8, 1, 512).cuda(), torch.rand(6).cuda()
    with torch.no_grad():
        alone = [n.encode_frame(a, e) for n in nets]
        torch.cuda.synchronize()
        streams = [_lib.side_stream(dev, ("ave_test", i)) for i in range(2)]
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


# ---- trainers and the renderer on 'ave' frames -----------------------------------------------------------------------
# the smallest scene of test_stages_gpu.py: 96 x 96 images, 2000 face / 900 mouth Gaussians


def _frames(n, dev, **kw):
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    from instag_amd.train import make_frame
    cams = toy_cameras(96)
    frames = [make_frame(cams[i].to(dev), synthetic_frame(96, i, dev, audio_extractor="ave", **kw)) for i in range(n)]
    assert tuple(frames[0].talking_dict["auds"].shape) == (8, 1, 512)
    return frames


def _nets(dev, seed, n_face=2000, n_mouth=900):
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    torch.manual_seed(seed)
    fa, ma = H.ave_args("face"), H.ave_args("mouth")
    pc_face = GaussianModel(1, PersonalizedMotionNetwork(args=fa).to(dev)).create_random(n_face, dev, seed=1)
    face_net = MotionNetwork(args=fa).to(dev)
    pc = GaussianModel(1, PersonalizedMotionNetwork(args=ma).to(dev)).create_random(n_mouth, dev, seed=2)
    net = MouthMotionNetwork(args=ma).to(dev)
    return pc_face, face_net, pc, net


class _Opt:
    iterations = 100000
    position_lr_init = 0.00016
    position_lr_final = 0.0000016
    position_lr_delay_mult = 0.01
    position_lr_max_steps = 45000
    feature_lr = 0.0025
    opacity_lr = 0.05
    scaling_lr = 0.003
    rotation_lr = 0.001
    percent_dense = 0.005
    lambda_dssim = 0.2
    densification_interval = 3
    opacity_reset_interval = 6
    densify_from_iter = 2
    densify_until_iter = 11
    densify_grad_threshold = 0.00002


def _trainer(kind, dev, seed=7):
    from instag_amd.train import build_trainer
    from instag_amd.train_stages import FuseTrainer, MouthTrainer
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    if kind == "face":
        return build_trainer(2000, dev, seed=seed, densify=False, audio_extractor="ave")
    pc_face, face_net, pc_mouth, mouth_net = _nets(dev, seed)
    if kind == "mouth":
        return MouthTrainer(pc_mouth, mouth_net, pc_face, face_net, bg, opt=_Opt, densify=False, seed=3, warm_step=0,
                            bg_iter=1000)
    return FuseTrainer(pc_face, face_net, pc_mouth, mouth_net, bg, opt=_Opt)


def _audio_state(tr):
    return torch.cat([p.detach().reshape(-1).clone() for p in tr.motion_net.audio_net.parameters()])


@pytest.mark.parametrize("kind", ["face", "mouth", "fuse"])
def test_ave_trainers_graph_matches_eager(kind):
    """The face, mouth and fuse steps on 'ave' frames: a few eager steps == the same steps replayed from a hipGraph
    (the tolerance of test_stage_trainers_graph_matches_eager); the audio net's parameters move where the stage trains
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


@pytest.mark.parametrize("kind", ["face", "mouth", "fuse"])
def test_ave_step_matches_torch_branch(kind, monkeypatch):
    """One step's loss and audio-net gradients with the HIP operator == the same step with audio.supported patched to
    False (the torch modules answer).  Gradient bound: the one test_face_phase_step_matches_torch_loss_statement uses
    for two fp32 evaluations of the same step that differ in summation order (2e-4 of the tensor's largest entry)."""
    from instag_amd import audio as A
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
        names = [n for n in _audio_names(tr.motion_net) if not n.startswith("exp_encode_net")]
        grads = {n: p.grad.detach().clone() for n, p in tr.motion_net.named_parameters()
                 if n in names and p.grad is not None}
        return float(loss), grads

    calls = []
    real = A.frame_codes
    monkeypatch.setattr(A, "frame_codes", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    loss_h, grads_h = one()
    assert calls                                           # the HIP operator answered
    monkeypatch.setattr(A, "supported", lambda *a, **k: False)
    n_calls = len(calls)
    loss_t, grads_t = one()
    assert len(calls) == n_calls                           # ... and the torch modules the second time
    assert abs(loss_h - loss_t) <= 2e-6 * max(1.0, abs(loss_t)), (loss_h, loss_t)
    assert set(grads_h) == set(grads_t)
    assert (len(grads_h) == 18) == (kind != "fuse") and (kind != "fuse" or not grads_h)
    for n in grads_t:
        scale = float(grads_t[n].abs().max())
        err = float((grads_h[n] - grads_t[n]).abs().max())
        print(f"{kind} {n}: err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-4 * scale + 1e-9, (n, err, scale)


def test_ave_fuse_inference_matches_torch_branch(monkeypatch):
    """FuseRenderer on one 'ave' frame, eager and from a hipGraph, == the render with the torch modules answering the
    per-frame branch (2e-6, the bound of test_fuse_inference_matches_plain_torch)."""
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
