"""CPU: host logic of the mouth UMF pretraining stage (instag_amd/pretrain.py, pretrain_mouth.py:34-358): the rescaled
schedule and its phases, the learning-rate lambda, the contrast-partner sampler, the lips-centring helper, the
checkpoint formats with the hand-off into MouthTrainer, the optimizer's weight decay, and the guards of the new
keywords."""
import os
import random
from types import SimpleNamespace

import pytest
import torch

from tests.test_pretrain_host import Opt

FACE = SimpleNamespace(audio_extractor="deepspeech", type="face")
MOUTH = SimpleNamespace(audio_extractor="deepspeech", type="mouth")


@pytest.mark.parametrize("K", [1, 3])
def test_schedule_and_phase_boundaries(K):
    from instag_amd.pretrain import pretrain_mouth_phase, pretrain_schedule
    s = pretrain_schedule(K, Opt, "mouth")
    assert (s.iterations, s.warm_step, s.densify_until, s.mouth_select_iter) == (
        30000 * K, 3000 * K, 29000 * K, 20000 * K)
    assert s.lpips_start > s.iterations                     # no LPIPS
    assert pretrain_schedule(K, Opt).warm_step == 1000 * K  # the face schedule is what it was
    w = s.warm_step
    ph = pretrain_mouth_phase(w - 1, K, Opt)
    assert (ph.motion, ph.warm, ph.hair_mask_iter) == (False, False, False)
    ph = pretrain_mouth_phase(w, K, Opt)                    # personalised mouth render, no warm terms
    assert (ph.motion, ph.warm, ph.hair_mask_iter) == (True, False, False)
    ph = pretrain_mouth_phase(w + 1, K, Opt)
    assert (ph.motion, ph.warm, ph.hair_mask_iter) == (True, True, False)
    assert pretrain_mouth_phase(1, K, Opt) == pretrain_mouth_phase(w - 1, K, Opt)
    assert pretrain_mouth_phase(s.iterations, K, Opt) == pretrain_mouth_phase(w + 1, K, Opt)


@pytest.mark.parametrize("K", [1, 3])
def test_motion_lr_lambda_on_the_mouth_schedule(K):
    from instag_amd.pretrain import motion_lr_lambda
    msi, iters = 20000 * K, 30000 * K
    for i in (0, 1, 2999 * K, msi - 1, msi, msi + 1, iters - 1, iters):
        want = 0.5 ** (i / msi) if i < msi else 0.1 ** (i / iters)
        assert motion_lr_lambda(i, K, Opt, "mouth") == want
    assert motion_lr_lambda(msi - 1, K, Opt, "mouth") > 0.5 > 0.1 ** (msi / iters) == motion_lr_lambda(msi, K, Opt, "mouth")


def test_partner_sampler():
    from instag_amd.pretrain import PartnerSampler
    for K in (2, 3, 5):
        a, b = PartnerSampler(K, seed=4), PartnerSampler(K, seed=4)
        seq = [i % K for i in range(200)]
        got = [a(i) for i in seq]
        assert got == [b(i) for i in seq]
        assert all(j != i and 0 <= j < K for i, j in zip(seq, got))
        assert got != [PartnerSampler(K, seed=5)(i) for i in seq] or K == 2
        if K > 2:
            assert len(set(got)) == K
    # the reference's draw: randint(0, K - 1), redrawn while it equals the trained identity
    rng, s = random.Random(9), PartnerSampler(4, seed=9)
    for i in (0, 3, 1, 1, 2):
        j = rng.randint(0, 3)
        while j == i:
            j = rng.randint(0, 3)
        assert s(i) == j
    one = PartnerSampler(1, seed=0)
    assert [one(0) for _ in range(5)] == [None] * 5


def test_centre_on_lips():
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.pretrain import centre_on_lips
    g = GaussianModel(1).create_random(50, "cpu", seed=1)
    before = g.get_xyz.detach().clone()
    param = g._xyz
    assert centre_on_lips(g) is g and g._xyz is param and g._xyz.requires_grad
    want = before / 2
    want[:, 1] -= 0.05
    assert torch.equal(g.get_xyz.detach(), want)


def _trainer(K=2, n=48):
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    from instag_amd.pretrain import PretrainMouthTrainer
    ids = [GaussianModel(1, PersonalizedMotionNetwork(args=MOUTH)).create_random(n, "cpu", seed=k) for k in range(K)]
    faces = [GaussianModel(1, PersonalizedMotionNetwork(args=FACE)).create_random(n, "cpu", seed=9 + k) for k in range(K)]
    return PretrainMouthTrainer(ids, MouthMotionNetwork(args=MOUTH), faces, MotionNetwork(args=FACE),
                                torch.tensor([0.0, 1.0, 0.0]), opt=Opt, names=["a", "b"][:K])


def test_checkpoint_layouts_and_handoff(tmp_path):
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    from instag_amd.pretrain import load_pretrained_motion
    from instag_amd.train_stages import MouthTrainer
    tr = _trainer()
    assert tr.sched.warm_step == 6000 and tr.ids[0].neural_motion_grid.out_dim == 7
    assert tr.ids[0].neural_motion_grid.hidden_dim == 16
    tr.iteration = 11
    with torch.no_grad():
        for s in tr.ema.shadow_params:
            s.add_(0.25)
    root = str(tmp_path)
    tr.save_checkpoints(root)
    assert sorted(os.listdir(root)) == ["a", "b", "chkpnt_ema_mouth_latest.pth", "chkpnt_mouth_latest.pth"]
    sd, osd, it = torch.load(os.path.join(root, "chkpnt_mouth_latest.pth"), weights_only=False)
    assert it == 11 and set(osd) == {"state", "param_groups"}
    for k, v in tr.motion_net.state_dict().items():
        assert torch.equal(sd[k], v)
    ema_path = os.path.join(root, "chkpnt_ema_mouth_latest.pth")
    ckpt = torch.load(ema_path, weights_only=False)
    assert len(ckpt) == 3 and ckpt[2] == 11
    esd = ckpt[0]
    for (n, p), s in zip(tr.motion_net.named_parameters(), tr.ema.shadow_params):
        assert torch.equal(esd[n], s), n                   # the EMA file holds the shadows ...
        assert torch.equal(p.detach(), sd[n])              # ... and the parameters hold their own values again
        assert not torch.equal(esd[n], sd[n])
    for name, g in zip(tr.names, tr.ids):
        assert sorted(os.listdir(os.path.join(root, name))) == ["chkpnt_mouth_11.pth", "chkpnt_mouth_latest.pth"]
        for f in ("chkpnt_mouth_11.pth", "chkpnt_mouth_latest.pth"):
            cap, usd, uosd, uit = torch.load(os.path.join(root, name, f), weights_only=False)
            assert uit == 11 and len(cap) == 15 and set(usd) == set(sd) and set(uosd) == {"state", "param_groups"}
            assert torch.equal(cap[1].detach(), g.get_xyz.detach())
    # train_mouth.py:67: the mouth adaptation starts from the EMA file
    pc = GaussianModel(1, PersonalizedMotionNetwork(args=MOUTH)).create_random(40, "cpu", seed=3)
    pc_face = GaussianModel(1, PersonalizedMotionNetwork(args=FACE)).create_random(40, "cpu", seed=4)
    mt = MouthTrainer(pc, MouthMotionNetwork(args=MOUTH), pc_face, MotionNetwork(args=FACE),
                      torch.tensor([0.0, 1.0, 0.0]), opt=Opt)
    load_pretrained_motion(mt.motion_net, ema_path)
    for (n, p), s in zip(mt.motion_net.named_parameters(), tr.ema.shadow_params):
        assert torch.equal(p.detach(), s), n


def test_face_stage_files_load(tmp_path):
    """The mouth stage's inputs are the files PretrainFaceTrainer.save_checkpoints writes (pretrain_mouth.py:80-98)."""
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, PersonalizedMotionNetwork
    from instag_amd.pretrain import load_face_stage
    from tests.test_pretrain_host import _trainer as face_trainer
    ft = face_trainer()
    ft.iteration = 5
    with torch.no_grad():
        for s in ft.ema.shadow_params:
            s.add_(0.5)
    ft.save_checkpoints(str(tmp_path))
    faces, umf = load_face_stage(str(tmp_path), ft.names, MotionNetwork(args=FACE),
                                 lambda: GaussianModel(1, PersonalizedMotionNetwork(args=FACE)))
    for f, g in zip(faces, ft.ids):
        assert torch.equal(f.get_xyz.detach(), g.get_xyz.detach()) and f.optimizer is None
        for a, b in zip(f.neural_motion_grid.parameters(), g.neural_motion_grid.parameters()):
            assert torch.equal(a.detach(), b.detach())
    for p, s in zip(umf.parameters(), ft.ema.shadow_params):
        assert torch.equal(p.detach(), s)


def test_effective_weight_decay_matches_torch_adamw():
    """pretrain_mouth.py:89 passes no weight decay: torch's default 0.01 reaches the groups that carry none of their own
    (the three encoders); the network's other groups carry wd = 0, the audio attention net 1e-4."""
    from instag_amd.motion_net import MouthMotionNetwork
    from instag_amd.optim import make_motion_optimizer
    from instag_amd.pretrain import MotionEMA
    net = MouthMotionNetwork(args=MOUTH)
    ref = torch.optim.AdamW(net.get_params(5e-3, 5e-4), betas=(0.9, 0.99), eps=1e-8)
    want = [(g["weight_decay"], g["lr"], tuple(g["betas"]), g["eps"]) for g in ref.param_groups]
    assert [w[0] for w in want] == [0, 0.01, 0.01, 0.01, 0, 0, 0.0001, 0]
    for on_gpu in (False, True):       # (the fused optimizer's constructor touches no device)
        o = make_motion_optimizer(net, on_gpu, ema=MotionEMA(net.parameters()))
        got = [(g["weight_decay"], g["lr"], tuple(g["betas"]), g["eps"]) for g in o.param_groups]
        assert got == want, on_gpu
        for a, b in zip(o.param_groups, ref.param_groups):
            assert [id(p) for p in a["params"]] == [id(p) for p in b["params"]]
        if on_gpu:
            assert all(g["decoupled"] for g in o.param_groups)
    assert [g["weight_decay"] for g in _trainer(1).motion_optimizer.param_groups] == [w[0] for w in want]


def test_new_keywords_raise_in_unsupported_combinations():
    from instag_amd.losses import mouth_loss_fused
    from instag_amd.renderer import render_motion_mouth_con
    pc = SimpleNamespace(get_xyz=torch.zeros(4, 3))
    head = torch.zeros(4, 7)
    for kw in (dict(pretrain_reg=True, personalized=True, align=False),                       # not on the device
               dict(pretrain_reg=False, personalized=True, align=False),
               dict(pretrain_other=head, pretrain_reg=True, personalized=True, align=False),
               dict(pretrain_reg=True, personalized=False, align=False),
               dict(pretrain_reg=True, personalized=True, align=True),
               dict(pretrain_other=head, personalized=True, align=False)):
        with pytest.raises(RuntimeError, match="pretrain_other"):
            render_motion_mouth_con(None, pc, None, None, None, **kw)
    img = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="extra replaces"):
        mouth_loss_fused(img, None, img, None, torch.zeros(4), None, p_raw=torch.zeros(4, 6), extra=torch.zeros(2))
    with pytest.raises(ValueError, match="extra replaces"):
        mouth_loss_fused(img, None, img, None, torch.zeros(4), None, p_xyz=torch.zeros(4, 3), extra=torch.zeros(2))


def test_step_needs_the_gpu():
    with pytest.raises(RuntimeError, match="PretrainMouthTrainer.step runs on the GPU"):
        _trainer(1).step(0, None)
