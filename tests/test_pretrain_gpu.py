"""GPU tests of the UMF pretraining stage (instag_amd/pretrain.py, pretrain_face.py:34-522): the pretraining deform
operator and the fused AdamW + EMA launch against plain torch, the whole step against a plain-torch transcription of the
reference's lines, and the hand-off of the EMA checkpoint to the face adaptation."""
import os

import pytest
import torch

from tests.test_stages_gpu import _frames, _plain_render_motion

pytestmark = pytest.mark.gpu


class PreOpt:
    """OptimizationParams of the reference's pretraining (30k iterations per identity)."""
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


def _deform_inputs(N, n_others, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    hp = r(N, 11) * 0.5
    hp[:, :3] += torch.sign(hp[:, :3]) * 0.3                    # displacements away from 0
    others = []
    for _ in range(n_others):
        sign = torch.where(torch.rand(N, 1, generator=g) < 0.5, -1.0, 1.0)
        h = r(N, 11)
        h[:, :3] = sign * (hp[:, :3] + 0.1 * r(N, 3))           # c_j of both signs, |c_j| well away from 0
        others.append(h)
    base = [r(N, 3) * 0.1, r(N, 3) * 0.5 - 4.0, r(N, 4), r(N, 1), r(N, 11) * 0.5, hp]
    return base, others


def _plain_deform(xyz, scaling, rotation, opacity, hu, hp, others):
    """gaussian_renderer/__init__.py:200-235 (personalized, not align) and the per-Gaussian loss lines of
    pretrain_face.py, with the reference's in-place updates and in-place contrast zeroing."""
    m = {"d_xyz": hu[..., :3] * 1e-2, "d_rot": hu[..., 3:7], "d_opa": hu[..., 7:8], "d_scale": hu[..., 8:11]}
    p = {"d_xyz": hp[..., :3] * 1e-2, "d_rot": hp[..., 3:7], "d_opa": hp[..., 7:8], "d_scale": hp[..., 8:11]}
    d_xyz, d_scale, d_rot = m["d_xyz"] + p["d_xyz"], m["d_scale"] + p["d_scale"], m["d_rot"] + p["d_rot"]
    m["d_xyz"], m["d_scale"], m["d_rot"] = d_xyz, d_scale, d_rot
    means = xyz + d_xyz
    scales = torch.nn.functional.softplus(scaling + d_scale)
    rots = torch.nn.functional.normalize(rotation + d_rot)
    opac = torch.sigmoid(opacity)
    reg = 0.0
    for d in (m, p):
        for k in ("d_xyz", "d_rot", "d_opa", "d_scale"):
            reg = reg + 1e-5 * d[k].abs().mean()
    for h in others:
        c = (h[..., :3] * 1e-2 * p["d_xyz"]).sum(-1)
        c[c < 0] = 0
        reg = reg + c.mean()
    return means, scales, rots, opac, reg


@pytest.mark.parametrize("n_others", [0, 1, 4])
def test_pretrain_deform_matches_plain_torch(n_others):
    from instag_amd.glue import pretrain_deform
    dev = torch.device("cuda")
    N = 3000
    base, others = _deform_inputs(N, n_others, seed=11 + n_others)
    base = [t.to(dev) for t in base]
    others = [t.to(dev) for t in others]
    g = torch.Generator().manual_seed(5)
    w = [torch.randn(N, k, generator=g).to(dev) for k in (3, 3, 4, 1)]

    def run(fn, part):
        leaves = [t.clone().requires_grad_(True) for t in base]
        outs = fn(*leaves, others)
        if part == "geometry":
            loss = sum((o * wi).sum() for o, wi in zip(outs[:4], w))
        else:
            loss = outs[4].sum() * 1e4          # (the regulariser and contrast terms alone, scaled up)
        loss.backward()
        return [o.detach() for o in outs[:4]], float(outs[4].detach().sum()), [t.grad for t in leaves]

    for part in ("geometry", "reg"):
        got, got_reg, got_g = run(lambda *a: pretrain_deform(*a[:6], others=a[6]), part)
        want, want_reg, want_g = run(_plain_deform, part)
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) <= 1e-6
        assert abs(got_reg - want_reg) <= 2e-6 * abs(want_reg), (got_reg, want_reg)
        names = ("xyz", "scaling", "rotation", "opacity", "h_u", "h_p")
        for name, a, b in zip(names, got_g, want_g):
            if b is None:
                assert a is None or float(a.abs().max()) == 0.0, (part, name)
                continue
            scale = float(b.abs().max())
            assert float((a - b).abs().max()) <= 2e-4 * scale + 1e-12, (part, name)
    if n_others:
        # the contrast term is non-trivial: both signs of c_j occur, and the term changes h_p's gradient
        c = ((others[0][:, :3] * 1e-2) * (base[5][:, :3] * 1e-2)).sum(-1)
        assert bool((c > 0).any()) and bool((c < 0).any())
        alone = run(lambda *a: pretrain_deform(*a[:6], others=[]), "reg")[2][5]
        with_contrast = got_g[5]                     # (the "reg" part's gradients: the loop's last pass)
        diff = float((with_contrast[:, :3] - alone[:, :3]).abs().max())
        assert diff > 0.1 * float(with_contrast[:, :3].abs().max())
        assert torch.equal(with_contrast[:, 3:], alone[:, 3:])


def test_fused_adamw_ema_matches_torch():
    from instag_amd.optim import MultiTensorAdamEMA
    from instag_amd.pretrain import MotionEMA
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(5000, generator=g), torch.randn(300, 7, generator=g), torch.randn(9000, generator=g)]
    ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    qs = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    ema = MotionEMA(ps, decay=0.995)
    shadow = [q.detach().clone() for q in qs]
    groups = lambda v: [{"params": [v[0], v[2]], "lr": 5e-3}, {"params": [v[1]], "lr": 2.5e-3, "weight_decay": 0.0}]
    opt = MultiTensorAdamEMA(groups(ps), ema, lr=5e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01, decoupled=True)
    ref = torch.optim.AdamW(groups(qs), lr=5e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    # five steps from the start, then three past the decay's cap (n >= 1791: d = 0.995)
    for n in list(range(1, 6)) + [1801, 1802, 1803]:
        if n == 1801:
            ema.counter[0] = 1800
        grads = [torch.randn(5000, generator=g).to(dev), torch.randn(300, 7, generator=g).to(dev)]
        for v in (ps, qs):
            v[0].grad, v[1].grad, v[2].grad = grads[0].clone(), grads[1].clone(), None     # v[2]: no gradient
        opt.step()
        ref.step()
        d = min(0.995, (1 + n) / (10 + n))
        with torch.no_grad():
            for s, q in zip(shadow, qs):
                tmp = s - q
                tmp.mul_(1.0 - d)
                s.sub_(tmp)
        opt.zero_grad()
        ref.zero_grad()
    torch.cuda.synchronize()
    for a, b in zip(ps, qs):
        assert float((a.detach() - b.detach()).abs().max()) <= 1e-6 * float(b.detach().abs().max())
    assert torch.equal(ps[2].detach(), qs[2].detach())             # not stepped
    for a, b in zip(ema.shadow_params, shadow):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    assert not torch.equal(ema.shadow_params[0], init[0].to(dev))
    assert ema.counter.tolist() == [1803, 0]
    assert float(opt.state[ps[0]]["step"]) == 8.0


def _grads_of(tr, idx, umf=True):
    g = tr.ids[idx]
    out = {k: p.grad.detach().clone() for k, p in g._p.items() if p.grad is not None}
    for name, net in (("umf", tr.motion_net if umf else None), ("pmf", g.neural_motion_grid)):
        if net is None:
            continue
        for n_, p_ in net.named_parameters():
            if p_.grad is not None:
                out[f"{name}.{n_}"] = p_.grad.detach().clone()
    return out


def _zero(tr):
    tr.motion_net.zero_grad(set_to_none=True)
    for g in tr.ids:
        for p in g._p.values():
            p.grad = None
        g.neural_motion_grid.zero_grad(set_to_none=True)


def _plain_pretrain_loss(tr, idx, frame, phase):
    """pretrain_face.py's step lines with plain torch ops: separate rasterizer passes, a second forward of the current
    PMF for the contrast, the in-place contrast zeroing, boolean-mask indexing."""
    from instag_amd.losses import face_loss_torch
    from instag_amd.renderer import render
    g, bg, td = tr.ids[idx], tr.bg, frame.talking_dict
    face, hair, mouth = td["face_mask"], td["hair_mask"], td["mouth_mask"]
    if not phase.motion:
        pkg = render(frame, g, None, bg)
        return face_loss_torch(pkg["render"], frame.original_image, face, hair, mouth, bg)
    pkg = _plain_render_motion(frame, g, tr.motion_net, bg, personalized=True, align=False)
    loss, l1 = face_loss_torch(pkg["render"], frame.original_image, face, hair, mouth, bg,
                               hair_mask_iter=phase.hair_mask_iter)
    if phase.warm:
        m, pm = pkg["motion"], pkg["p_motion"]
        for k in ("d_xyz", "d_rot", "d_opa", "d_scale"):
            loss = loss + 1e-5 * m[k].abs().mean()
        alpha, head = pkg["alpha"], face | hair
        loss = loss + 1e-3 * (((1 - alpha) * head).mean() + (alpha * ~head).mean())
        for k in ("d_xyz", "d_rot", "d_opa", "d_scale"):
            loss = loss + 1e-5 * pm[k].abs().mean()
        aud, exp = td["auds"], td["au_exp"]
        p2 = g.neural_motion_grid(g.get_xyz, aud, exp)
        contrast = 0
        for j, other in enumerate(tr.ids):
            if j == idx:
                continue
            with torch.no_grad():
                tmp = other.neural_motion_grid(g.get_xyz, aud, exp)
            ci = (tmp["d_xyz"] * p2["d_xyz"]).sum(-1)
            ci[ci < 0] = 0
            contrast = contrast + ci.mean()
        loss = loss + contrast
        r0, r1, c0, c1 = [int(v) for v in td["lips_rect"].tolist()]
        loss = loss + 5e-3 * pkg["attn"][1, r0:r1, c0:c1].mean()
        loss = loss + 5e-3 * pkg["p_attn"][1, r0:r1, c0:c1].mean()
        if not phase.hair_mask_iter:
            loss = loss + 1e-4 * pkg["attn"][1][hair].mean()
            loss = loss + 1e-4 * pkg["attn"][0][hair].mean()
    return loss, l1


@pytest.mark.parametrize("it", [2999, 3000, 3001, 3003], ids=["static", "warm_step", "hair", "no-hair"])
def test_pretrain_step_matches_torch_transcription(it):
    from instag_amd.deferred import deferred_grads
    from instag_amd.pretrain import build_pretrainer, pretrain_phase
    dev = torch.device("cuda")
    frame = _frames(96, 1, dev)[0]
    tr = build_pretrainer(3, 2500, dev, seed=2, opt=PreOpt)
    phase = pretrain_phase(it, 3, PreOpt)
    assert (phase.motion, phase.warm, phase.hair_mask_iter) == {
        2999: (False, False, False), 3000: (True, False, False), 3001: (True, True, True),
        3003: (True, True, False)}[it]
    idx = 1
    pkg, loss, l1 = tr._forward_backward(idx, frame, phase)
    loss, l1 = float(loss.detach()), float(l1.detach())
    # (a live autograd graph of this pass would keep the parameters' gradient accumulators, bound to the side streams of
    # its per-frame branches, into the backward of the plain pass below)
    del pkg
    got = _grads_of(tr, idx)
    for j in (0, 2):                    # the other identities never receive gradients
        assert not _grads_of(tr, j, umf=False), j
    _zero(tr)
    want, want_l1 = _plain_pretrain_loss(tr, idx, frame, phase)
    with deferred_grads(dev):
        want.backward()
    ref = _grads_of(tr, idx)
    want, want_l1 = float(want.detach()), float(want_l1.detach())
    assert abs(loss - want) <= 2e-6 * max(1.0, abs(want)), (loss, want)
    assert abs(l1 - want_l1) <= 2e-6
    assert set(got) == set(ref), set(got) ^ set(ref)
    assert any(k.startswith("umf.") for k in ref) == phase.motion
    for k in ref:
        scale = float(ref[k].abs().max())
        err = float((got[k] - ref[k]).abs().max())
        assert err <= 2e-4 * scale + 1e-9, (k, err, scale)


def test_pretrain_to_adaptation_handoff(tmp_path):
    """A few pretraining steps (warm phase, one density event), then the EMA checkpoint: it holds the shadows, loads
    into a FaceTrainer's UMF (train_face.py:66-68), and that trainer steps."""
    from instag_amd.pretrain import IdentitySampler, build_pretrainer, load_pretrained_motion
    from instag_amd.train import build_trainer
    dev = torch.device("cuda")
    frames = _frames(96, 2, dev)
    Opt = type("Opt", (PreOpt,), {"densify_from_iter": 1, "densification_interval": 2})
    tr = build_pretrainer(2, 2000, dev, seed=5, opt=Opt, densify=True)
    tr.iteration = 2000                                  # warm_step = 2000: the next steps carry every term
    pick = IdentitySampler(2, seed=1)
    init = [s.clone() for s in tr.ema.shadow_params]
    for i in range(4):                                   # 2002 and 2004: density control of the picked identity
        out = tr.step(pick(), frames[i % 2])
        assert torch.isfinite(out["loss"])
    torch.cuda.synchronize()
    assert tr.ema.counter.tolist() == [4, 0]
    assert any(not torch.equal(a, b) for a, b in zip(tr.ema.shadow_params, init))
    root = str(tmp_path)
    tr.save_checkpoints(root)
    path = os.path.join(root, "chkpnt_ema_face_latest.pth")
    esd, _, it = torch.load(path, weights_only=False)
    assert it == 2004
    for (n, _), s in zip(tr.motion_net.named_parameters(), tr.ema.shadow_params):
        assert torch.equal(esd[n], s), n
    ft = build_trainer(2000, dev, seed=6)
    load_pretrained_motion(ft.motion_net, path)
    for (n, p), s in zip(ft.motion_net.named_parameters(), tr.ema.shadow_params):
        assert torch.equal(p.detach(), s), n
    out = ft.step(frames[0])
    assert torch.isfinite(out["loss"])


def test_pretrain_graph_matches_eager():
    """Graph mode == eager launches over a fixed identity sequence (K = 2) that crosses warm_step (static render, the
    motion render without warm terms, then hair and non-hair iterations) and one density-control event: losses, both
    identities' parameters, the UMF, its EMA shadows and counter.  A capture consumes no iteration, and the identity
    whose parameter set changed is captured again."""
    from instag_amd import diff_gauss
    from instag_amd.pretrain import build_pretrainer
    dev = torch.device("cuda")
    frames = _frames(96, 3, dev)
    # density control at 2004 only (it > 2003 and it % 4 == 0) within iterations 1997..2007; warm_step = 2000
    Opt = type("Opt", (PreOpt,), {"densify_from_iter": 2003, "densification_interval": 4})
    seq = [0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0]

    def run(graph):
        tr = build_pretrainer(2, 2000, dev, seed=7, opt=Opt, densify=True)
        tr.iteration = 1996
        if graph:
            tr.enable_graph()
        losses = []
        try:
            for i, idx in enumerate(seq):
                losses.append(float(tr.step(idx, frames[i % 3])["loss"]))
        finally:
            diff_gauss.set_capacity_plan(None)
        torch.cuda.synchronize()
        vec = [torch.cat([p.detach().reshape(-1) for p in g._p.values()]) for g in tr.ids]
        vec += [torch.cat([p.detach().reshape(-1) for p in g.neural_motion_grid.parameters()]) for g in tr.ids]
        vec += [torch.cat([p.detach().reshape(-1) for p in tr.motion_net.parameters()]),
                torch.cat([s.reshape(-1) for s in tr.ema.shadow_params])]
        return losses, vec, tr

    le, ve, te = run(False)
    lg, vg, tg = run(True)
    assert tg.iteration == te.iteration == 2007
    # (static, id 0) and (static, id 1) are captured once each and replayed; id 0's steps after the event are captured again
    assert 5 <= tg.captures < len(seq) - 1, tg.captures
    assert te.ema.counter.tolist() == tg.ema.counter.tolist() == [len(seq), 0]
    assert [g.num_points for g in te.ids] == [g.num_points for g in tg.ids]
    for a_, b_ in zip(le, lg):
        assert abs(a_ - b_) <= 1e-4 * max(1.0, abs(a_)), (le, lg)
    for k, (a_, b_) in enumerate(zip(ve, vg)):
        assert float((a_ - b_).abs().max()) <= 2e-4, k
