"""Train steps of the two stages that follow the face branch: the mouth branch and the face+mouth fuse stage.

Counterparts of /root/reference/train_mouth.py:106-293 and /root/reference/train_fuse_con.py:75-245 restricted to
the hot path (render -> loss -> backward -> statistics / density control -> optimizers).  Same kernels as the face
branch behind other callers: ``render_motion_mouth_con`` / ``render_motion`` of
instag_amd/renderer.py, the fused L1+SSIM operator, the single-launch Adam.  Frame selection by AU25, logging and
checkpoint cadence are the reference's data pipeline / control plane and stay out.  The fuse stage's LPIPS patch term
(train_fuse_con.py:186-193) is opt-in: ``FuseTrainer(..., lpips=LPIPSWeights)``; the mouth branch's exists only under
``mode_long``, which the trainers do not carry.
"""
from __future__ import annotations

import random
from dataclasses import dataclass
from typing import Optional

import torch

from . import graphs
from .deferred import backward
from .gaussian_model import GaussianModel, OptimizationParams, green_mask
from .losses import l1_and_ssim
from .optim import StepOptimizers, lambda_lr, make_motion_optimizer
from .train import Frame, densify_and_prune_at, motion_lr_factor

GEOMETRY = ("xyz", "opacity", "scaling", "rotation")


def _lips_mask(like: torch.Tensor, lips_rect) -> torch.Tensor:
    """lips_mask[xmin:xmax, ymin:ymax] = True (train_mouth.py:168-170: the rect indexes rows first).  A tensor
    rect stays on its device (comparisons against row / column indices: no host round trip, capturable)."""
    H, W = like.shape[-2:]
    if torch.is_tensor(lips_rect):
        lr = lips_rect.to(device=like.device, dtype=torch.int64)
        rows = torch.arange(H, device=like.device)[:, None]
        cols = torch.arange(W, device=like.device)[None, :]
        return (rows >= lr[0]) & (rows < lr[1]) & (cols >= lr[2]) & (cols < lr[3])
    r0, r1, c0, c1 = [int(v) for v in lips_rect]
    m = torch.zeros(H, W, dtype=torch.bool, device=like.device)
    m[r0:r1, c0:c1] = True
    return m


def mouth_loss(image, alpha, gt, mouth_mask, lips_mask, bg, p_xyz=None, warm=True, lambda_dssim=0.2):
    """Loss block of the mouth branch (train_mouth.py:186-221) -> (loss, Ll1).  Outside the lips rectangle the
    mouth-mask fringe of the render is painted with the background; the target shows the image inside the mouth mask
    only.  ``warm`` (iteration > warm_step) adds the alignment and alpha terms."""
    bg3 = bg[:, None, None]
    gt_green = torch.where(mouth_mask[None], gt, bg3.expand_as(gt))
    image_green = torch.where((lips_mask ^ mouth_mask)[None], bg3.expand_as(image), image)
    Ll1, s = l1_and_ssim(image_green, gt_green)
    loss = Ll1 + lambda_dssim * (1.0 - s)
    if warm:
        lm = lips_mask.to(alpha.dtype)
        if p_xyz is not None:
            loss = loss + 1e-5 * p_xyz.abs().mean()
        loss = loss + 1e-3 * (((1 - alpha) * lm).mean() + (alpha * (1 - lm)).mean())
    return loss, Ll1


def fuse_loss(image, gt, lambda_dssim=0.2):
    """train_fuse_con.py:176-181 (iteration >= bg_iter = 0, always): whole-frame L1 + DSSIM -> (loss, Ll1)."""
    if image.is_cuda and image.dim() == 3 and image.shape[0] == 3:
        from .losses import plain_loss_fused
        return plain_loss_fused(image, gt, lambda_dssim)
    Ll1, s = l1_and_ssim(image, gt)
    return Ll1 + lambda_dssim * (1.0 - s), Ll1


@dataclass(frozen=True)
class MouthPhase:
    align: bool = True
    warm: bool = True
    late: bool = False        # iteration > bg_iter: black background, geometry and the motion field frozen


def mouth_phase(iteration: int, opt=OptimizationParams, warm_step: int = 3000,
                bg_iter: Optional[int] = None) -> MouthPhase:
    """train_mouth.py:48-52, 152-196 (mode_long = False): bg_iter = motion_stop_iter = iterations - 1000."""
    bg_iter = opt.iterations - 1000 if bg_iter is None else bg_iter
    align = iteration > 1000 if iteration < warm_step else True
    return MouthPhase(align=align, warm=iteration > warm_step, late=iteration > bg_iter)


def _drop_graph(trainer):
    graphs.drop_plan(trainer._graph)
    trainer._graph = None
    trainer._graph_key = None


class MouthTrainer:
    """One iteration of train_mouth.py: the mouth Gaussians + MouthMotionNetwork are optimised, the (trained) face
    Gaussians + face field only supply the jaw-movement feature."""

    def __init__(self, gaussians: GaussianModel, motion_net, gaussians_face: GaussianModel, motion_net_face,
                 background, opt=OptimizationParams, cameras_extent: float = 0.2, densify: bool = True, seed: int = 0,
                 warm_step: int = 3000, bg_iter: Optional[int] = None):
        self.bg_iter = bg_iter
        self.g, self.motion_net = gaussians, motion_net
        self.g_face, self.motion_net_face = gaussians_face, motion_net_face
        self.bg = background
        self.opt, self.extent, self.densify, self.warm_step = opt, cameras_extent, densify, warm_step
        self.device = gaussians.get_xyz.device
        self.on_gpu = self.device.type == "cuda"
        self.iteration = 0
        self.rng = random.Random(seed)                                       # k = randint(10, 50), train_mouth.py:175
        self.gen = torch.Generator(device=self.device).manual_seed(seed)
        self.motion_optimizer = make_motion_optimizer(motion_net, self.on_gpu)
        self._base_lr = [float(g["lr"]) for g in self.motion_optimizer.param_groups]
        gaussians.training_setup(opt, fused=self.on_gpu)
        self.optimizers = StepOptimizers(self.motion_optimizer, self.g.optimizer)
        self._graph = None
        self._graph_key = None
        # the selection size of a captured step lives on the device; it rides on the optimizers' learning-rate upload
        # (MultiTensorAdam.reserve_extra_i64) instead of a fill launch per step -- `_k_own` until that table exists
        self._k_own = torch.full((1,), 10, dtype=torch.int64, device=self.device) if self.on_gpu else None
        if self.optimizers.combined is not None:
            self.optimizers.combined.reserve_extra_i64(1)
        self.last = {}

    @property
    def _k_dev(self):
        combined = self.optimizers.combined
        view = combined.extra_i64() if combined is not None else None
        return view if view is not None else self._k_own

    def _stage_k(self, k):
        """Call in FRONT of _set_learning_rates (whose upload carries the value)."""
        combined = self.optimizers.combined
        if combined is not None and combined.extra_i64() is not None:
            combined.set_extra_i64([k])
        elif self._k_own is not None:
            self._k_own.fill_(k)

    def _set_learning_rates(self, it):
        lambda_lr(self.motion_optimizer, self._base_lr, motion_lr_factor(it - 1, self.warm_step, self.opt.iterations))
        self.g.update_learning_rate(it)
        self.optimizers.push_lrs()

    def _freeze_late(self):
        """train_mouth.py:189-196: after bg_iter the motion field and the Gaussians' geometry stop learning."""
        for p in self.motion_net.parameters():
            p.requires_grad_(False)
        for k in GEOMETRY:
            self.g._p[k].requires_grad_(False)      # (every late iteration: density control rebuilds the leaves)

    def forward(self, frame: Frame, phase: MouthPhase, k: int):
        from .renderer import render_motion_mouth_con
        bg = torch.zeros_like(self.bg) if phase.late else self.bg
        pkg = render_motion_mouth_con(frame, self.g, self.motion_net, self.g_face, self.motion_net_face, None, bg,
                                      personalized=False, align=phase.align, k=k)
        td = frame.talking_dict
        dev = self.device
        mouth = td["mouth_mask"].to(dev)
        want_p = phase.warm and pkg["p_motion"] is not None
        if self.on_gpu and torch.is_tensor(td["lips_rect"]) and pkg["render"].shape[0] == 3:
            from .losses import mouth_loss_fused
            p_raw = dict.get(pkg["p_motion"], "_p") if want_p else None
            p_xyz = pkg["p_motion"]["p_xyz"] if (want_p and p_raw is None) else None
            loss, Ll1 = mouth_loss_fused(pkg["render"], pkg["alpha"], frame.original_image.to(dev), mouth,
                                         td["lips_rect"].to(dev), bg, p_xyz, warm=phase.warm,
                                         lambda_dssim=self.opt.lambda_dssim, p_raw=p_raw)
            return pkg, loss, Ll1
        p_xyz = pkg["p_motion"]["p_xyz"] if want_p else None
        lips = _lips_mask(mouth, td["lips_rect"])
        loss, Ll1 = mouth_loss(pkg["render"], pkg["alpha"], frame.original_image.to(dev), mouth, lips, bg, p_xyz,
                               warm=phase.warm, lambda_dssim=self.opt.lambda_dssim)
        return pkg, loss, Ll1

    def _stats_on(self, it):
        return self.densify and it < self.opt.densify_until_iter

    def _density_due(self, it):
        o = self.opt
        return self._stats_on(it) and ((it > o.densify_from_iter and it % o.densification_interval == 0)
                                       or it % o.opacity_reset_interval == 0)

    @torch.no_grad()
    def _accumulate_stats(self, pkg):
        """train_mouth.py:262-263 (device-only: part of a captured step)."""
        vis = pkg["visibility_filter"]
        radii = pkg["radii"].to(self.g.max_radii2D.dtype)
        self.g.max_radii2D.copy_(torch.max(self.g.max_radii2D, torch.where(vis, radii, torch.zeros_like(radii))))
        self.g.add_densification_stats(pkg["viewspace_points"].grad, vis)

    @torch.no_grad()
    def _density_control(self, it, frame: Frame):
        """train_mouth.py:265-283, behind the statistics of this iteration."""
        o = self.opt
        if not self._stats_on(it):
            return
        if it > o.densify_from_iter and it % o.densification_interval == 0:
            densify_and_prune_at(self.g, it, o.densify_until_iter, o, self.extent, self.gen)
            if it > 2000:
                # Gaussians that took the background's green are pushed towards removal (:276-279)
                green = green_mask(self.g, frame.camera_center.to(self.device), (100, 180, 100))
                self.g.xyz_gradient_accum[green] /= 2
                self.g._opacity.data[green] = self.g.inverse_opacity_activation(
                    torch.ones_like(self.g._opacity.data[green]) * 0.1)
                self.g._scaling.data[green] /= 10
        if it % o.opacity_reset_interval == 0:
            self.g.reset_opacity()

    def _zero_grad(self):
        self.optimizers.zero_grad()

    def _body(self, frame: Frame, phase: MouthPhase, k, stats_on: bool):
        """Everything of an iteration without a density-control event; free of host round trips when `k` is a
        device tensor (the captured form)."""
        from .losses import defer_finalize
        with defer_finalize():          # (backward follows at once; the loss value is read after the step)
            pkg, loss, Ll1 = self.forward(frame, phase, k)
        backward(loss, self.device)
        if stats_on:
            self._accumulate_stats(pkg)
        self.optimizers.step()
        self._zero_grad()
        return loss, Ll1, pkg

    def _key(self, it):
        return (mouth_phase(it, self.opt, self.warm_step, self.bg_iter), self._stats_on(it), self.g.active_sh_degree)

    def enable_graph(self, example: Frame, headroom: float = 1.5, warmup_steps: int = 2):
        """Capture the step of the NEXT iterations' phase (the warm-up steps are real steps: they advance the
        iteration counter).  step() falls back to eager launches on density-control iterations and drops the graph
        when the phase or the parameter set changes."""
        _drop_graph(self)
        total = max(1, warmup_steps) + 2
        key = self._key(self.iteration + total + 1)
        phase, stats_on, _ = key
        if phase.late:
            self._freeze_late()

        def pre():
            self.iteration += 1
            self._stage_k(self.rng.randint(10, 50))
            self._set_learning_rates(self.iteration)

        def body(frame):
            return self._body(frame, phase, self._k_dev, stats_on)
        self._graph = graphs.GraphedStage(body, example, self.device,
                                          lambda counts: graphs.stage_capacities(counts, headroom), warmup_steps, pre)
        self._graph_key = key
        return self._graph

    def step(self, frame: Frame):
        self.iteration += 1
        it = self.iteration
        k = self.rng.randint(10, 50)
        if self._graph is not None:
            self._stage_k(k)                    # (travels with the learning rates)
        self._set_learning_rates(it)
        if it % 1000 == 0:
            self.g.oneupSHdegree()                                                                # train_mouth.py:110-111
        phase = mouth_phase(it, self.opt, self.warm_step, self.bg_iter)
        if phase.late:
            self._freeze_late()
        due = self._density_due(it)
        steps = it < self.opt.iterations
        if self._graph is not None and (due or not steps or self._key(it) != self._graph_key):
            _drop_graph(self)
        if self._graph is not None:
            loss, Ll1 = self._graph.replay(frame)[:2]
            if self._graph.overflow_due():
                _drop_graph(self)               # the scene outgrew the captured capacities: eager launches from here on
        else:
            graphs.begin_eager_step()
            pkg, loss, Ll1 = self.forward(frame, phase, k)
            backward(loss, self.device)
            if self._stats_on(it):
                self._accumulate_stats(pkg)
                self._density_control(it, frame)
            if steps:
                self.optimizers.step()
                self._zero_grad()
        self.last = dict(loss=loss.detach(), l1=Ll1.detach(), num_points=self.g.num_points, phase=phase, k=k)
        return self.last


class FuseTrainer:
    """One iteration of train_fuse_con.py: face and mouth are rendered, composited over the per-camera background
    and compared with the whole frame; both motion fields and most of the geometry are frozen from the first
    iteration (bg_iter = 0), so the step tunes colours (both models) and the face's opacity."""

    FROZEN_FACE = ("xyz", "scaling", "rotation")
    FROZEN_MOUTH = ("xyz", "opacity", "scaling", "rotation")

    def __init__(self, gaussians: GaussianModel, motion_net, gaussians_mouth: GaussianModel, motion_net_mouth,
                 background, opt=OptimizationParams, seed: int = 0, lpips=None):
        """``lpips`` (instag_amd.lpips.LPIPSWeights): from iteration > iterations // 2 the step adds
        0.05 * PatchLPIPS(image, gt_image, p), p = 2 * randint(16, 21) (train_fuse_con.py:186-193)."""
        self.g, self.motion_net = gaussians, motion_net
        self.g_mouth, self.motion_net_mouth = gaussians_mouth, motion_net_mouth
        self.bg, self.opt = background, opt
        self.device = gaussians.get_xyz.device
        self.on_gpu = self.device.type == "cuda"
        self.iteration = 0
        gaussians.training_setup(opt, fused=self.on_gpu)
        gaussians_mouth.training_setup(opt, fused=self.on_gpu)
        self.optimizers = StepOptimizers(gaussians.optimizer, gaussians_mouth.optimizer)
        for net in (motion_net, motion_net_mouth):
            for p in net.parameters():
                p.requires_grad_(False)
        for k in self.FROZEN_FACE:
            gaussians._p[k].requires_grad_(False)
        for k in self.FROZEN_MOUTH:
            gaussians_mouth._p[k].requires_grad_(False)
        self._graph = None
        self._graph_key = None
        self.last = {}
        self.lpips = lpips
        self.rng = random.Random(seed)                                       # patch size, train_fuse_con.py:192
        self._patch_op = None
        # the patch size of a captured step lives on the device and rides on the learning-rate upload (MouthTrainer._k_dev)
        self._p_own = None
        if lpips is not None and self.on_gpu:
            self._p_own = torch.full((1,), 32, dtype=torch.int64, device=self.device)
            if self.optimizers.combined is not None:
                self.optimizers.combined.reserve_extra_i64(1)

    @property
    def _p_dev(self):
        combined = self.optimizers.combined
        view = combined.extra_i64() if (combined is not None and self.lpips is not None) else None
        return view if view is not None else self._p_own

    def _stage_p(self, p):
        """Call in FRONT of _set_learning_rates (whose upload carries the value)."""
        combined = self.optimizers.combined
        if combined is not None and combined.extra_i64() is not None:
            combined.set_extra_i64([p])
        else:
            self._p_own.fill_(p)

    def _lpips_on(self, it) -> bool:
        from .lpips import fuse_lpips_on
        return self.lpips is not None and fuse_lpips_on(it, self.opt)

    def _draw_patch(self, it):
        """The iteration's patch size (None before the term starts; the generator is drawn from only when it is on)."""
        from .lpips import draw_fuse_patch
        return draw_fuse_patch(self.rng) if self._lpips_on(it) else None

    def forward(self, frame: Frame, p=None):
        """``p``: the LPIPS patch size of this iteration (an int, or the device scalar of a captured step); None = off."""
        from .renderer import render_fuse
        dev = self.device
        scene_bg = frame.talking_dict.get("background")
        out = render_fuse(frame, self.g, self.motion_net, self.g_mouth, self.motion_net_mouth, None, self.bg,
                          scene_background=None if scene_bg is None else scene_bg.to(dev))
        gt = frame.original_image.to(dev)
        loss, Ll1 = fuse_loss(out["image"], gt, self.opt.lambda_dssim)
        if p is not None:
            from .lpips import FUSE_LPIPS_WEIGHT, FUSE_PATCH_RANGE, PatchLPIPS
            if self._patch_op is None:
                self._patch_op = PatchLPIPS(self.lpips, gt.shape[-2], gt.shape[-1], *FUSE_PATCH_RANGE)
            loss = loss + FUSE_LPIPS_WEIGHT * self._patch_op(out["image"], gt, p)
        return out, loss, Ll1

    def _set_learning_rates(self, it):
        self.g.update_learning_rate(it)           # train_fuse_con.py:85 (the mouth model keeps its initial rates)
        self.optimizers.push_lrs()

    def _body(self, frame: Frame, p=None):
        from contextlib import nullcontext
        from .losses import defer_finalize
        # (backward follows at once; the loss value is read after the step -- unless the LPIPS term is ADDED to it here)
        with (defer_finalize() if p is None else nullcontext()):
            out, loss, Ll1 = self.forward(frame, p)
        backward(loss, self.device)
        self.optimizers.step()
        self.optimizers.zero_grad()
        return loss, Ll1, out["image"], out

    def enable_graph(self, example: Frame, headroom: float = 1.5, warmup_steps: int = 2):
        """Capture the whole step (the stage has no density control: densify_until_iter = 0; with ``lpips`` it has two
        phases, before and after iterations // 2 -- the graph holds the one of the iterations right after the capture,
        and one graph serves every patch size; warm-up steps that would straddle the boundary are preceded by eager
        steps up to it).  step() drops a graph of the first half at iterations // 2 + 1 and launches eagerly from
        there: call enable_graph again once ``_lpips_on(iteration + 1)`` to replay the second half (capturing costs
        warm-up steps, which are train steps, so step() does not do it behind the caller's back)."""
        _drop_graph(self)
        total = max(1, warmup_steps) + 2
        on = self._lpips_on(self.iteration + total + 1)
        # the warm-up steps run the captured body: they must all lie on the capture's side of iterations // 2
        while self._lpips_on(self.iteration + 1) != on:
            self.step(example)
            on = self._lpips_on(self.iteration + total + 1)

        def pre():
            self.iteration += 1
            if on:
                from .lpips import draw_fuse_patch
                self._stage_p(draw_fuse_patch(self.rng))
            self._set_learning_rates(self.iteration)

        def body(frame):
            return self._body(frame, self._p_dev if on else None)
        self._graph = graphs.GraphedStage(body, example, self.device,
                                          lambda counts: graphs.stage_capacities(counts, headroom), warmup_steps, pre)
        self._graph_key = on
        return self._graph

    def step(self, frame: Frame):
        self.iteration += 1
        it = self.iteration
        p = self._draw_patch(it)
        if self._graph is not None and p is not None:
            self._stage_p(p)                    # (travels with the learning rates)
        self._set_learning_rates(it)
        if self._graph is not None and (it >= self.opt.iterations or self._graph_key != (p is not None)):
            _drop_graph(self)
        if self._graph is not None:
            loss, Ll1, image = self._graph.replay(frame)[:3]
            if self._graph.overflow_due():
                _drop_graph(self)
        elif it < self.opt.iterations:
            graphs.begin_eager_step()
            loss, Ll1, image = self._body(frame, p)[:3]
        else:
            out, loss, Ll1 = self.forward(frame, p)      # last iteration: no optimizer step (:242)
            backward(loss, self.device)
            self.optimizers.zero_grad()
            image = out["image"]
        self.last = dict(loss=loss.detach(), l1=Ll1.detach(), image=image.detach())
        if self.lpips is not None:
            self.last["patch"] = p
        return self.last
