"""GPU tests of the mouth UMF pretraining stage (instag_amd/pretrain.py, pretrain_mouth.py:34-358): the mouth pretraining
deform operator against an fp64 plain-torch statement, one whole step against a plain-torch transcription of the
reference's lines, graph mode against eager launches, determinism, and the hand-off of the EMA checkpoint to the mouth
adaptation.  Bounds: the ones tests/test_pretrain_gpu.py applies to the face counterparts."""
import math
import os

import pytest
import torch

from tests.test_pretrain_gpu import PreOpt
from tests.test_stages_gpu import _frames

pytestmark = pytest.mark.gpu

XYZ_SCALE = (1e-2 / 5, 1e-2, 1e-2 / 5)


# ---- 1. the operator ----------------------------------------------------------------------------------------------------
def _deform_inputs(N, seed, opposite=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    h, hs = r(N, 7) * 0.5, r(N, 1)
    h[:, :3] += torch.sign(h[:, :3]) * 0.3                       # displacements away from 0
    hp = r(N, 7) * 0.5
    hp[:, :3] += torch.sign(hp[:, :3]) * 0.3
    if opposite:
        # the PMF's displacement is several times the gated mouth displacement and of the opposite sign in every
        # component: |d_xyz + p.d_xyz| and its gradient differ in sign from the uncombined |d_xyz|
        gated = (h[:, :3] * torch.tensor(XYZ_SCALE)) * torch.sigmoid(hs) * 2
        hp[:, :3] = -4.0 * gated / 1e-2
    sign = torch.where(torch.rand(N, 1, generator=g) < 0.5, -1.0, 1.0)
    hq = r(N, 7)
    hq[:, :3] = sign * (hp[:, :3] + 0.1 * r(N, 3))               # contrast products of both signs, away from 0
    base = [r(N, 3) * 0.1, r(N, 3) * 0.5 - 4.0, r(N, 4), r(N, 1), h, hs, hp]
    return base, hq


def _plain_mouth_deform(xyz, scaling, rotation, opacity, h, hs, hp, hq, combined=True):
    """gaussian_renderer/__init__.py:377-406 (personalized, not align) and pretrain_mouth.py:231-276 per Gaussian, in the
    dtype of the inputs, with the reference's in-place ``d_xyz += p_motion_preds['d_xyz']`` and in-place contrast
    zeroing.  -> means3D, scales, rotations, opacity, [the five sums].  ``combined=False``: the first regulariser on the
    mouth field's own displacement, which is what an out-of-place addition would leave in the dictionary."""
    scale = torch.tensor(XYZ_SCALE, dtype=xyz.dtype, device=xyz.device)
    own = (h[..., :3] * scale) * torch.sigmoid(hs) * 2
    m = {"d_xyz": own * 1.0, "d_rot": h[..., 3:]}
    p = {"d_xyz": hp[..., :3] * 1e-2, "d_rot": hp[..., 3:]}
    d_xyz = m["d_xyz"]
    d_xyz += p["d_xyz"]
    means = xyz + d_xyz
    scales = torch.nn.functional.softplus(scaling)
    rots = torch.nn.functional.normalize(rotation)
    opac = torch.sigmoid(opacity)
    sums = [1e-5 * (m["d_xyz"] if combined else own).abs().mean(), 1e-5 * m["d_rot"].abs().mean(),
            1e-5 * p["d_xyz"].abs().mean(), 1e-5 * p["d_rot"].abs().mean()]
    if hq is not None:
        c = ((hq[..., :3] * 1e-2) * p["d_xyz"]).sum(-1)
        c[c < 0] = 0
        sums.append(c.mean())
    else:
        sums.append(means.new_zeros(()))
    return means, scales, rots, opac, sums


NAMES = ("xyz", "scaling", "rotation", "opacity", "h", "hs", "h_p")


def _run_operator(base, hq, part, w):
    from instag_amd.glue import pretrain_mouth_deform
    leaves = [t.clone().requires_grad_(True) for t in base]
    outs = pretrain_mouth_deform(*leaves, h_q=hq)
    loss = sum((o * wi).sum() for o, wi in zip(outs[:4], w)) if part == "geometry" else outs[4].sum() * 1e4
    loss.backward()
    return [o.detach() for o in outs[:4]], float(outs[4].detach().double().sum()), [t.grad for t in leaves]


def _run_plain64(base, hq, part, w, combined=True):
    leaves = [t.double().clone().requires_grad_(True) for t in base]
    outs = _plain_mouth_deform(*leaves, None if hq is None else hq.double(), combined=combined)
    loss = sum((o * wi.double()).sum() for o, wi in zip(outs[:4], w)) if part == "geometry" else sum(outs[4]) * 1e4
    loss.backward()
    return [o.detach() for o in outs[:4]], [float(s) for s in outs[4]], [t.grad for t in leaves]


@pytest.mark.parametrize("case", ["no-partner", "partner", "opposite"])
def test_mouth_deform_matches_fp64_statement(case):
    from instag_amd.glue import pretrain_mouth_deform
    dev = torch.device("cuda")
    N = 3000
    base, hq = _deform_inputs(N, seed=21 + len(case), opposite=case == "opposite")
    base = [t.to(dev) for t in base]
    hq = None if case == "no-partner" else hq.to(dev)
    g = torch.Generator().manual_seed(5)
    w = [torch.randn(N, k, generator=g).to(dev) for k in (3, 3, 4, 1)]
    for part in ("geometry", "reg"):
        got, got_reg, got_g = _run_operator(base, hq, part, w)
        want, want_sums, want_g = _run_plain64(base, hq, part, w)
        want_reg = sum(want_sums)
        print(case, part, "outputs", [float((a.double() - b).abs().max()) for a, b in zip(got, want)],
              "reg", got_reg, want_reg)
        for a, b in zip(got, want):
            assert float((a.double() - b).abs().max()) <= 1e-6
        assert abs(got_reg - want_reg) <= 2e-6 * abs(want_reg), (got_reg, want_reg)
        for name, a, b in zip(NAMES, got_g, want_g):
            if b is None:
                assert a is None or float(a.abs().max()) == 0.0, (part, name)
                continue
            scale = float(b.abs().max())
            err = float((a.double() - b).abs().max())
            print(case, part, name, err, scale)
            assert err <= 2e-4 * scale + 1e-12, (part, name, err, scale)
    # each of the five sums on its own: the operator without the partner drops exactly the contrast
    if hq is not None:
        leaves = [t.clone() for t in base]
        alone = float(pretrain_mouth_deform(*leaves, h_q=None)[4].double().sum())
        assert abs(alone - sum(want_sums[:4])) <= 2e-6 * sum(want_sums[:4])
        assert want_sums[4] > 0
        c = ((hq[:, :3] * 1e-2) * (base[6][:, :3] * 1e-2)).sum(-1)
        assert bool((c > 0).any()) and bool((c < 0).any())
        no_con = _run_operator(base, None, "reg", w)[2]
        assert torch.equal(no_con[4], got_g[4]) and torch.equal(no_con[5], got_g[5])       # h, hs: no contrast gradient
        assert torch.equal(no_con[6][:, 3:], got_g[6][:, 3:]) and not torch.equal(no_con[6][:, :3], got_g[6][:, :3])
    if case == "opposite":
        # in-place semantics (gaussian_renderer/__init__.py:387): the regulariser sees own + PMF displacement.  Here that
        # is -3 x the mouth field's own displacement: the sum is 3 x the uncombined one and the gradient into the mouth
        # field's head has the opposite sign
        _, sums_u, g_u = _run_plain64(base, hq, "reg", w, combined=False)
        assert abs(want_sums[0] - 3 * sums_u[0]) <= 1e-5 * want_sums[0]     # (h_p is rounded to fp32)
        got_sum0 = alone - sum(want_sums[1:4])               # (without the far larger contrast sum)
        assert abs(got_sum0 - want_sums[0]) <= 0.01 * want_sums[0] < abs(got_sum0 - sums_u[0])
        gh, gh_u = got_g[4][:, :3].double(), g_u[4][:, :3]
        assert float((gh + gh_u).abs().max()) <= 2e-4 * float(gh_u.abs().max())            # == -uncombined
        assert float((gh - gh_u).abs().max()) > float(gh_u.abs().max())
        # and the PMF's head takes the first regulariser's gradient too: d/dh_p = (sgn(combined) + sgn(p)) w 1e-2
        assert float((got_g[6][:, :3].double() - want_g[6][:, :3]).abs().max()) <= 2e-4 * float(want_g[6].abs().max())


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
def test_mouth_deform_is_deterministic():
    dev = torch.device("cuda")
    N = 20001                                    # (not a multiple of the workgroup size)
    base, hq = _deform_inputs(N, seed=3)
    base, hq = [t.to(dev) for t in base], hq.to(dev)
    g = torch.Generator().manual_seed(6)
    w = [torch.randn(N, k, generator=g).to(dev) for k in (3, 3, 4, 1)]

    def both(part):
        from instag_amd.glue import pretrain_mouth_deform
        leaves = [t.clone().requires_grad_(True) for t in base]
        outs = pretrain_mouth_deform(*leaves, h_q=hq)
        (sum((o * wi).sum() for o, wi in zip(outs[:4], w)) + outs[4].sum() * 1e4).backward()
        return [o.detach() for o in outs] + [t.grad for t in leaves]

    a, b = both("x"), both("x")
    assert len(a) == 12
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    from instag_amd import _lib
    assert a[4].numel() == _lib.lib().instag_pretrain_mouth_deform_num_partials(N) == (N + 255) // 256


# ---- 2. one whole step ---------------------------------------------------------------------------------------------------
def _plain_mouth_render(frame, pc, motion_net, pc_face, motion_net_face, bg, k=10):
    """gaussian_renderer/__init__.py:302-435 with personalized=True, align=False, inference=False: plain torch ops, the
    reference's in-place addition, top-k for the jaw feature."""
    from instag_amd.diff_gauss import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(
        image_height=frame.image_height, image_width=frame.image_width, tanfovx=math.tan(frame.FoVx * 0.5),
        tanfovy=math.tan(frame.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=frame.world_view_transform,
        projmatrix=frame.full_proj_transform, sh_degree=pc.active_sh_degree, campos=frame.camera_center,
        prefiltered=False, debug=False)
    aud = frame.talking_dict["auds"]
    p = pc.neural_motion_grid(pc.get_xyz, aud)
    exp = torch.zeros_like(frame.talking_dict["au_exp"])
    face = motion_net_face(pc_face.get_xyz, aud, exp)
    with torch.no_grad():
        dy = face["d_xyz"][..., 1]
        mx, mn = dy.topk(k, 0, True, True)[0], dy.topk(k, 0, False, True)[0]
        move = torch.stack([mx[-1], mn[-1], mx[-1] - mn[-1]]).reshape(1, 3) * 1e2
    m = dict(motion_net(pc.get_xyz, aud, move.detach()).items())
    d_xyz = m["d_xyz"]
    d_xyz += p["d_xyz"]
    m2 = torch.zeros_like(pc.get_xyz, requires_grad=True)
    opacity = pc.get_opacity
    img, depth, normal, alpha, radii, extra = GaussianRasterizer(s)(
        means3D=pc.get_xyz + d_xyz, means2D=m2, shs=pc.get_features, opacities=opacity, scales=pc.get_scaling,
        rotations=pc.rotation_activation(pc._rotation), extra_attrs=torch.ones_like(opacity))
    return dict(render=img, alpha=alpha, radii=radii, viewspace_points=m2, motion=m, p_motion=p)


def _plain_mouth_step(tr, idx, frame, it, partner):
    """pretrain_mouth.py:113-358 for one iteration on trainer ``tr`` (an untouched twin of the trainer under test) with
    plain torch operators and torch.optim optimizers.  -> (loss, Ll1, the gradients the optimizers stepped with)"""
    from instag_amd.deferred import deferred_grads
    from instag_amd.losses import l1_loss, ssim
    from instag_amd.pretrain import motion_lr_lambda
    from instag_amd.renderer import render
    K, opt, g, bg, td = tr.K, tr.opt, tr.ids[idx], tr.bg, frame.talking_dict
    warm_step = 3000 * K
    g.update_learning_rate(it)
    if it < warm_step:
        pkg = render(frame, g, None, bg)
    else:
        pkg = _plain_mouth_render(frame, g, tr.motion_net, tr.faces[idx], tr.motion_net_face, bg)
    image, alpha = pkg["render"], pkg["alpha"]
    mouth = td["mouth_mask"]
    r0, r1, c0, c1 = [int(v) for v in td["lips_rect"].tolist()]
    lips = torch.zeros_like(mouth)
    lips[r0:r1, c0:c1] = True
    gt_green = frame.original_image * mouth + bg[:, None, None] * ~mouth
    image = image.clone()
    image[:, (lips ^ mouth)] = bg[:, None]
    Ll1 = l1_loss(image, gt_green)
    loss = Ll1 + opt.lambda_dssim * (1.0 - ssim(image, gt_green))
    if it > warm_step:
        m, pm = pkg["motion"], pkg["p_motion"]
        loss = loss + 1e-5 * m["d_xyz"].abs().mean()
        loss = loss + 1e-5 * m["d_rot"].abs().mean()
        loss = loss + 1e-3 * (((1 - alpha) * lips).mean() + (alpha * ~lips).mean())
        loss = loss + 1e-5 * pm["d_xyz"].abs().mean()
        loss = loss + 1e-5 * pm["d_rot"].abs().mean()
        if partner is not None:
            aud = td["auds"]
            p2 = g.neural_motion_grid(g.get_xyz, aud)
            with torch.no_grad():
                tmp = tr.ids[partner].neural_motion_grid(g.get_xyz, aud)
            c = (tmp["d_xyz"] * p2["d_xyz"]).sum(-1)
            c[c < 0] = 0
            loss = loss + c.mean()
    with deferred_grads(tr.device):
        loss.backward()
    with torch.no_grad():
        vis = pkg["radii"] > 0
        g.max_radii2D[vis] = torch.max(g.max_radii2D[vis], pkg["radii"][vis].to(g.max_radii2D.dtype))
        g.add_densification_stats(pkg["viewspace_points"].grad, vis)
    # :89-90, gaussian_model.training_setup: fresh torch optimizers (the twin has not stepped), LambdaLR at it - 1
    mo = torch.optim.AdamW(tr.motion_net.get_params(5e-3, 5e-4), betas=(0.9, 0.99), eps=1e-8)
    for grp in mo.param_groups:
        grp["lr"] = grp["lr"] * motion_lr_lambda(it - 1, K, opt, "mouth")
    go = torch.optim.Adam([{"params": grp["params"], "lr": float(grp["lr"])} for grp in g.optimizer.param_groups],
                          lr=0.0, eps=1e-15)
    info = {}
    for o in (mo, go):
        for grp in o.param_groups:
            for p in grp["params"]:
                info[id(p)] = (grp["lr"], grp["eps"], None if p.grad is None else p.grad.detach().clone())
    mo.step()
    go.step()
    shadows = [s.clone() for s in tr.ema.shadow_params]
    d = min(0.995, (1 + 1) / (10 + 1))                       # torch_ema: first update
    with torch.no_grad():
        for s, p in zip(shadows, tr.motion_net.parameters()):
            s.sub_((1.0 - d) * (s - p))
    return float(loss.detach()), float(Ll1.detach()), info, shadows


def _first_step_bound(p_ref, lr, eps, g_ref):
    """How far a parameter may be from the transcription's after the FIRST Adam step when its gradient is within the
    face counterpart's bound e = 2e-4 max|g_ref| + 1e-9: the step is lr u(g), u(g) = g / (|g| + eps) (zero moments, bias
    corrections cancel); u' <= 1 / (|g| + eps), so |u(g) - u(g_ref)| <= e / (max(|g_ref| - e, 0) + eps), and never more
    than 2.  Plus 4 ulp of the parameter for its own rounding."""
    e = 2e-4 * float(g_ref.abs().max()) + 1e-9
    du = (e / ((g_ref.abs() - e).clamp_min(0.0) + eps)).clamp_max(2.0)
    return lr * du + 4 * torch.finfo(torch.float32).eps * p_ref.abs()


@pytest.mark.parametrize("offset", [-1, 0, 2], ids=["static", "warm_step", "warm"])
def test_mouth_pretrain_step_matches_torch_transcription(offset):
    from instag_amd.pretrain import build_mouth_pretrainer, pretrain_mouth_phase
    dev = torch.device("cuda")
    K, idx = 3, 1
    frame = _frames(96, 1, dev)[0]
    it = 3000 * K + offset
    phase = pretrain_mouth_phase(it, K, PreOpt)
    assert (phase.motion, phase.warm) == {-1: (False, False), 0: (True, False), 2: (True, True)}[offset]
    tr = build_mouth_pretrainer(K, 900, 1500, dev, seed=2, opt=PreOpt)
    twin = build_mouth_pretrainer(K, 900, 1500, dev, seed=2, opt=PreOpt)
    for a, b in zip(tr.motion_net.parameters(), twin.motion_net.parameters()):
        assert torch.equal(a, b)
    tr.iteration = it - 1
    out = tr.step(idx, frame)
    partner = out.get("drawn")
    assert (partner is not None) == phase.warm and partner != idx
    torch.cuda.synchronize()
    want, want_l1, info, shadows = _plain_mouth_step(twin, idx, frame, it, partner)
    loss, l1 = float(out["loss"]), float(out["l1"])
    print(offset, "loss", loss, want, "l1", l1, want_l1)
    assert abs(loss - want) <= 2e-6 * max(1.0, abs(want)), (loss, want)
    assert abs(l1 - want_l1) <= 2e-6
    g, h = tr.ids[idx], twin.ids[idx]
    pairs = [(f"g.{k}", g._p[k], h._p[k]) for k in g._p]
    pairs += [(f"pmf.{n}", a, b) for (n, a), (_, b) in zip(g.neural_motion_grid.named_parameters(),
                                                          h.neural_motion_grid.named_parameters())]
    umf = [(f"umf.{n}", a, b) for (n, a), (_, b) in zip(tr.motion_net.named_parameters(),
                                                      twin.motion_net.named_parameters())]
    moved = 0
    for name, a, b in pairs + umf:
        lr, eps, g_ref = info[id(b)]
        if g_ref is None:
            # no gradient: neither optimizer touches the tensor (torch skips it, decay included)
            assert float((a - b).abs().max()) <= 4 * torch.finfo(torch.float32).eps * float(b.abs().max()), name
            continue
        moved += 1
        bound = _first_step_bound(b.detach(), lr, eps, g_ref)
        err = (a.detach() - b.detach()).abs()
        print(offset, name, float(err.max()), float(bound.max()), float((bound < 2 * lr).float().mean()))
        assert bool((err <= bound).all()), (name, float((err - bound).max()))
    assert moved >= (6 if not phase.motion else 20)
    d = 1.0 - 2.0 / 11.0
    for (name, a, b), s, s_ref in zip(umf, tr.ema.shadow_params, shadows):
        lr, eps, g_ref = info[id(b)]
        bound = 4 * torch.finfo(torch.float32).eps * s_ref.abs() if g_ref is None else \
            d * _first_step_bound(b.detach(), lr, eps, g_ref) + 4 * torch.finfo(torch.float32).eps * s_ref.abs()
        assert bool(((s - s_ref).abs() <= bound).all()), ("ema", name)
    assert tr.ema.counter.tolist() == [1, 0]
    # the other identities and the frozen face side did not move
    for j in (0, 2):
        for a, b in zip(list(tr.ids[j]._p.values()) + list(tr.ids[j].neural_motion_grid.parameters()),
                        list(twin.ids[j]._p.values()) + list(twin.ids[j].neural_motion_grid.parameters())):
            assert torch.equal(a, b)
    for a, b in zip(tr.motion_net_face.parameters(), twin.motion_net_face.parameters()):
        assert torch.equal(a, b) and a.grad is None
    # statistics (while it < densify_until)
    for a, b in ((g.denom, h.denom), (g.max_radii2D, h.max_radii2D)):
        assert torch.equal(a, b)
    acc, acc_ref = g.xyz_gradient_accum, h.xyz_gradient_accum
    assert float(acc_ref.max()) > 0
    assert float((acc - acc_ref).abs().max()) <= 2e-4 * float(acc_ref.abs().max()) + 1e-9


# ---- 3. graph mode against eager launches ---------------------------------------------------------------------------------
def _state(tr):
    out = []
    for g in tr.ids:
        out += [p.detach() for p in g._p.values()] + [p.detach() for p in g.neural_motion_grid.parameters()]
        out += [g.xyz_gradient_accum, g.denom, g.max_radii2D]
        for st in g.optimizer.state.values():
            out += [st[k] for k in ("exp_avg", "exp_avg_sq", "step") if torch.is_tensor(st.get(k))]
    out += [p.detach() for p in tr.motion_net.parameters()] + list(tr.ema.shadow_params) + [tr.ema.counter]
    for st in tr.motion_optimizer.state.values():
        out += [st[k] for k in ("exp_avg", "exp_avg_sq", "step") if torch.is_tensor(st.get(k))]
    return out


def test_mouth_pretrain_graph_matches_eager():
    """Graph mode == eager launches, bit for bit, over ten steps at K = 3 that change identity and partner, cross
    warm_step (static render, motion render without warm terms, warm iterations) and one density-control event (9004):
    parameters, moments, EMA and statistics.  One capture per distinct key; the identity whose parameter set changed is
    captured again.  (The mouth field's table gradient is summed in 64-bit fixed point and in fixed order, csrc/grid.hip
    triplane_level_backward_kernel, so nothing in the step depends on the order of atomic additions.)"""
    from instag_amd import diff_gauss
    from instag_amd.pretrain import build_mouth_pretrainer
    dev = torch.device("cuda")
    frames = _frames(96, 3, dev)
    Opt = type("Opt", (PreOpt,), {"densify_from_iter": 9003, "densification_interval": 4})
    seq = [0, 1, 2, 0, 1, 2, 1, 0, 0, 1]          # (9004 = identity 0's density event; it returns at 9005)

    def run(graph):
        tr = build_mouth_pretrainer(3, 900, 1500, dev, seed=7, opt=Opt, densify=True)
        tr.iteration = 8996
        if graph:
            tr.enable_graph()
        keys, gen, losses = set(), [0, 0, 0], []
        try:
            for i, idx in enumerate(seq):
                out = tr.step(idx, frames[i % 3])
                losses.append(float(out["loss"]))
                if tr._density_due(tr.iteration):
                    gen[idx] += 1
                else:
                    keys.add((idx, out["phase"], out.get("drawn"), gen[idx]))
        finally:
            diff_gauss.set_capacity_plan(None)
        torch.cuda.synchronize()
        return tr, keys, losses

    te, ke, le = run(False)
    tg, kg, lg = run(True)
    assert te.iteration == tg.iteration == 9006 and ke == kg
    assert sum(1 for i in range(8997, 9007) if te._density_due(i)) == 1
    assert len({k[2] for k in kg}) >= 3 and len({k[1] for k in kg}) == 3          # partners (and None), three phases
    assert tg.captures == len(kg), (tg.captures, len(kg))
    assert any(k[0] == 0 and k[3] == 1 for k in kg)                               # identity 0, captured again
    assert [g.num_points for g in te.ids] == [g.num_points for g in tg.ids]
    assert te.ema.counter.tolist() == tg.ema.counter.tolist() == [len(seq), 0]
    se, sg = _state(te), _state(tg)
    assert len(se) == len(sg)
    worst = max(float((a.float() - b.float()).abs().max()) for a, b in zip(se, sg))
    print("graph vs eager: losses", le, lg, "largest state difference", worst,
          "tensors that differ", sum(1 for a, b in zip(se, sg) if not torch.equal(a, b)), "of", len(se))
    for a, b in zip(se, sg):
        assert torch.equal(a, b)


# ---- 5. hand-off -----------------------------------------------------------------------------------------------------------
def test_mouth_pretrain_to_adaptation_handoff(tmp_path):
    """A few pretraining steps (warm phase, one density event), then the EMA checkpoint: it holds the shadows, loads into
    a MouthTrainer's field (train_mouth.py:67), and that trainer steps."""
    from instag_amd.pretrain import IdentitySampler, build_mouth_pretrainer, load_pretrained_motion
    from instag_amd.train_stages import MouthTrainer
    from tests.test_stages_gpu import _mouth_setup
    dev = torch.device("cuda")
    frames = _frames(96, 2, dev)
    Opt = type("Opt", (PreOpt,), {"densify_from_iter": 1, "densification_interval": 2})
    tr = build_mouth_pretrainer(2, 900, 1500, dev, seed=5, opt=Opt, densify=True)
    tr.iteration = 6000                                  # warm_step = 6000: the next steps carry every term
    pick = IdentitySampler(2, seed=1)
    init = [s.clone() for s in tr.ema.shadow_params]
    for i in range(4):                                   # 6002 and 6004: density control of the picked identity
        out = tr.step(pick(), frames[i % 2])
        assert torch.isfinite(out["loss"]) and out["drawn"] == 1 - out["identity"]
    torch.cuda.synchronize()
    assert tr.ema.counter.tolist() == [4, 0]
    assert any(not torch.equal(a, b) for a, b in zip(tr.ema.shadow_params, init))
    root = str(tmp_path)
    tr.save_checkpoints(root)
    path = os.path.join(root, "chkpnt_ema_mouth_latest.pth")
    esd, _, it = torch.load(path, weights_only=False)
    assert it == 6004
    for (n, _), s in zip(tr.motion_net.named_parameters(), tr.ema.shadow_params):
        assert torch.equal(esd[n], s), n
    pc_face, face_net, pc, net = _mouth_setup(dev)
    mt = MouthTrainer(pc, net, pc_face, face_net, tr.bg, opt=PreOpt, densify=False, seed=0)
    load_pretrained_motion(mt.motion_net, path)
    for (n, p), s in zip(mt.motion_net.named_parameters(), tr.ema.shadow_params):
        assert torch.equal(p.detach(), s), n
    out = mt.step(frames[0])
    assert torch.isfinite(out["loss"])


def test_composed_path_agrees_with_the_operator():
    """The measurement switch of scripts/bench_pretrain_mouth.py (fused_deform=False: today's torch-composed personalised
    branch plus torch loss terms) computes the same loss as the operator."""
    from instag_amd.pretrain import build_mouth_pretrainer, pretrain_mouth_phase
    dev = torch.device("cuda")
    frame = _frames(96, 1, dev)[0]
    vals = []
    for fused in (True, False):
        tr = build_mouth_pretrainer(2, 900, 1500, dev, seed=4, opt=PreOpt, fused_deform=fused)
        pkg, loss, l1 = tr.forward_loss(0, frame, pretrain_mouth_phase(6002, 2, PreOpt), 1)
        vals.append((float(loss), float(l1)))
        del pkg
    assert abs(vals[0][0] - vals[1][0]) <= 2e-6 * max(1.0, abs(vals[1][0])) and abs(vals[0][1] - vals[1][1]) <= 2e-6
