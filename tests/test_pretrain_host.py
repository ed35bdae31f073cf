"""CPU: host logic of the UMF pretraining stage (instag_amd/pretrain.py, pretrain_face.py:34-522): the rescaled
schedule, the motion learning-rate lambda, the EMA (torch_ema 0.3 semantics), the checkpoint formats and the
identity sampler."""
import os
from types import SimpleNamespace

import pytest
import torch


class Opt:
    iterations = 30000
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
    densification_interval = 100
    opacity_reset_interval = 3000
    densify_from_iter = 500
    densify_until_iter = 29000
    densify_grad_threshold = 0.0005


@pytest.mark.parametrize("K", [1, 3])
def test_phase_boundaries(K):
    from instag_amd.pretrain import pretrain_phase, pretrain_schedule
    s = pretrain_schedule(K, Opt)
    assert (s.iterations, s.warm_step, s.densify_until, s.mouth_select_iter, s.lpips_start) == (
        30000 * K, 1000 * K, 29000 * K, 20000 * K, 99999999 * K)
    w = s.warm_step
    ph = pretrain_phase(w - 1, K, Opt)
    assert not ph.motion and not ph.warm and not ph.hair_mask_iter
    ph = pretrain_phase(w, K, Opt)                     # motion render, no warm terms
    assert ph.motion and not ph.warm and not ph.hair_mask_iter
    for it in range(w + 1, w + 30):
        ph = pretrain_phase(it, K, Opt)
        assert ph.motion and ph.warm
        assert ph.hair_mask_iter == (it % 7 != 0)
    assert not pretrain_phase(7 * 1000 * K, K, Opt).hair_mask_iter
    assert pretrain_phase(s.iterations, K, Opt).hair_mask_iter == (s.iterations % 7 != 0)


@pytest.mark.parametrize("K", [1, 3])
def test_motion_lr_lambda_closed_form(K):
    from instag_amd.pretrain import motion_lr_lambda
    msi, iters = 20000 * K, 30000 * K
    for i in (0, 1, 999, msi - 1, msi, msi + 1, iters - 1, iters):
        want = 0.5 ** (i / msi) if i < msi else 0.1 ** (i / iters)
        assert motion_lr_lambda(i, K, Opt) == want
    # reference LambdaLR: step `it` runs with lambda(it - 1)
    net = torch.nn.Linear(2, 2)
    o = torch.optim.AdamW(net.parameters(), lr=5e-3)
    sch = torch.optim.lr_scheduler.LambdaLR(o, lambda i: motion_lr_lambda(i, K, Opt))
    for it in range(1, 5):
        assert o.param_groups[0]["lr"] == 5e-3 * motion_lr_lambda(it - 1, K, Opt)
        o.step()
        sch.step()


def test_ema_matches_transcription():
    from instag_amd.pretrain import MotionEMA
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(7, 3)), torch.nn.Parameter(torch.randn(5))]
    ema = MotionEMA(ps, decay=0.995)
    shadow = [p.detach().clone() for p in ps]
    decays = []
    for n in range(1, 1900):          # (the decay reaches its cap at n = 1791)
        with torch.no_grad():
            for p in ps:
                p.add_(torch.randn_like(p) * 0.1)
        ema.update()
        d = min(0.995, (1 + n) / (10 + n))
        decays.append(d)
        for s, p in zip(shadow, ps):
            s.sub_((1.0 - d) * (s - p.detach()))
        assert ema.num_updates == n
    assert decays[0] == 2 / 11 and decays[-1] == 0.995
    for a, b in zip(ema.shadow_params, shadow):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)
    before = [p.detach().clone() for p in ps]
    with ema.average_parameters():
        for p, s in zip(ps, shadow):
            assert torch.allclose(p, s, rtol=1e-6, atol=1e-7)
    for p, b in zip(ps, before):
        assert torch.equal(p.detach(), b)


def _trainer(K=2, n=64):
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, PersonalizedMotionNetwork
    from instag_amd.pretrain import PretrainFaceTrainer
    args = SimpleNamespace(audio_extractor="deepspeech", type="face")
    ids = []
    for k in range(K):
        g = GaussianModel(1, neural_motion_grid=PersonalizedMotionNetwork(args=args))
        g.create_random(n, "cpu", seed=k)
        ids.append(g)
    umf = MotionNetwork(args=args)
    return PretrainFaceTrainer(ids, umf, torch.tensor([0.0, 1.0, 0.0]), opt=Opt, names=["a", "b"][:K])


def test_checkpoint_layouts(tmp_path):
    from instag_amd.motion_net import MotionNetwork
    from instag_amd.pretrain import load_pretrained_motion
    tr = _trainer()
    tr.iteration = 7
    with torch.no_grad():
        for s in tr.ema.shadow_params:
            s.add_(0.25)
    root = str(tmp_path)
    tr.save_checkpoints(root)
    sd, osd, it = torch.load(os.path.join(root, "chkpnt_face_latest.pth"), weights_only=False)
    assert it == 7 and set(osd) == {"state", "param_groups"}
    for k, v in tr.motion_net.state_dict().items():
        assert torch.equal(sd[k], v)
    esd, _, eit = torch.load(os.path.join(root, "chkpnt_ema_face_latest.pth"), weights_only=False)
    assert eit == 7
    names = [n for n, _ in tr.motion_net.named_parameters()]
    for n, s in zip(names, tr.ema.shadow_params):
        assert torch.equal(esd[n], s), n
    fresh = MotionNetwork(args=SimpleNamespace(audio_extractor="deepspeech", type="face"))
    fresh.load_state_dict(esd, strict=True)
    load_pretrained_motion(fresh, os.path.join(root, "chkpnt_ema_face_latest.pth"))
    for (n, p), s in zip(fresh.named_parameters(), tr.ema.shadow_params):
        assert torch.equal(p.detach(), s), n
    # the parameters hold their own values again after the EMA file was written
    for n, p in tr.motion_net.named_parameters():
        assert torch.equal(p.detach(), sd[n])
    for name, g in zip(tr.names, tr.ids):
        for f in ("chkpnt_face_7.pth", "chkpnt_face_latest.pth"):
            cap, usd, uosd, uit = torch.load(os.path.join(root, name, f), weights_only=False)
            assert uit == 7 and len(cap) == 15 and set(usd) == set(sd)
            assert torch.equal(cap[1].detach(), g.get_xyz.detach())


def test_share_audio_net_raises():
    from instag_amd.pretrain import PretrainFaceTrainer
    with pytest.raises(NotImplementedError, match="share_audio_net"):
        PretrainFaceTrainer([], None, None, share_audio_net=True)


def test_identity_sampler_is_seeded_randint():
    import random
    from instag_amd.pretrain import IdentitySampler
    a, b = IdentitySampler(5, seed=3), random.Random(3)
    assert [a() for _ in range(50)] == [b.randint(0, 4) for _ in range(50)]
