"""Identity-free pretraining of the universal motion fields (UMF) over K identities: the face field
(PretrainFaceTrainer, described first) and the mouth field (PretrainMouthTrainer, at the end).

Counterpart of /root/reference/pretrain_face.py:34-522 restricted to the step, as train.py is for train_face.py.  Each
identity has its own Gaussians and personalised motion field (PMF); one UMF is shared by all of them and is what the
stage produces: ``chkpnt_ema_face_latest.pth``, the file train_face.py:66-68 starts the face adaptation from
(load_pretrained_motion).  An iteration trains the identity the caller picks (IdentitySampler mirrors the reference's
``randint(0, K - 1)``):
  render (static before warm_step, then render_motion(personalized=True, align=False, return_attn=True))
  -> L1 + lambda * DSSIM with the mouth / hair painting of the face branch, and after warm_step: the regularisers of both
     fields, the alpha term, the contrast of the identity's PMF against the other identities' PMFs, the attention terms
  -> backward -> statistics / density control of that identity -> AdamW (UMF) + Adam (identity) -> EMA of the UMF.

On the device the deformation, every per-Gaussian loss term and the contrast are one operator (glue.pretrain_deform),
the personalised attention map's lips term rides in the loss kernel's extra array (glue.window_mean_append), and the
EMA is part of the UMF's AdamW launch (optim.MultiTensorAdamEMA).  LPIPS (never reached: lpips_start = 99999999 K), the
mouth-opening / AU frame curriculum, logging and validation renders are out of scope.

The mouth stage is the counterpart of /root/reference/pretrain_mouth.py:34-358 in the same form.  It reads the face
stage's files (load_face_stage), trains one MouthMotionNetwork over K mouth clouds (centre_on_lips) and writes
``chkpnt_ema_mouth_latest.pth``, the file train_mouth.py:67 starts the mouth adaptation from.  An iteration:
  render (static before warm_step = 3000 K, then render_motion_mouth_con(personalized=True, align=False), k = 10)
  -> the mouth branch's compositing loss, and after warm_step: the regularisers of both fields (the mouth field's d_xyz
     AFTER the reference's in-place addition of the PMF's, gaussian_renderer/__init__.py:387), the alpha term and the
     contrast against one other identity (PartnerSampler)
  -> backward -> statistics / density control (green Gaussians damped, not pruned) -> AdamW + EMA, Adam.
The deformation and the per-Gaussian terms are one operator (glue.pretrain_mouth_deform); PretrainFaceTrainer and
PretrainMouthTrainer share _PretrainTrainer.  The frame curriculum of pretrain_mouth.py:132-159 (AU25 windows, the
mouth-mask size filter), logging and validation renders are out of scope here too; LPIPS is never reached.
"""
from __future__ import annotations

import contextlib
import os
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import diff_gauss, graphs
from .deferred import backward
from .gaussian_model import GaussianModel, OptimizationParams, green_mask
from .losses import face_loss
from .optim import StepOptimizers, lambda_lr, make_motion_optimizer
from .train import FACE_GREEN, densify_and_prune_at, restore_state, snapshot_state, update_densification_stats


# ---- schedule (pretrain_face.py:48-67: every boundary scaled by the number of identities K) --------------------------
@dataclass(frozen=True)
class PretrainSchedule:
    iterations: int           # opt.iterations * K
    warm_step: int            # 1000 K (face), 3000 K (mouth)
    densify_until: int        # (opt.iterations - 1000) K
    mouth_select_iter: int    # (opt.iterations - 10000) K
    lpips_start: int          # 99999999 K (no LPIPS, no mouth-mask dilation)


WARM_STEP = {"face": 1000, "mouth": 3000}     # pretrain_face.py:50, pretrain_mouth.py:42 (per identity)


def pretrain_schedule(K: int, opt=OptimizationParams, stage: str = "face") -> PretrainSchedule:
    """``stage`` = "face" (pretrain_face.py:48-67) or "mouth" (pretrain_mouth.py:38-52: the same boundaries with a warm
    step of 3000 K; its p_motion_start_iter is 0 and its lpips_start is never reached either)."""
    return PretrainSchedule(iterations=opt.iterations * K, warm_step=WARM_STEP[stage] * K,
                            densify_until=(opt.iterations - 1000) * K,
                            mouth_select_iter=(opt.iterations - 10000) * K, lpips_start=99999999 * K)


@dataclass(frozen=True)
class PretrainPhase:
    """What a pretraining iteration computes."""
    motion: bool = True            # render_motion(personalized=True) instead of the static render (it >= warm_step)
    warm: bool = True              # it > warm_step: regularisers, alpha, contrast and attention terms
    hair_mask_iter: bool = False   # hair painted to background in image and target, hair attention terms off


def pretrain_phase(iteration: int, K: int, opt=OptimizationParams, hair_mask_interval: int = 7) -> PretrainPhase:
    s = pretrain_schedule(K, opt)
    it = iteration
    hair = (s.warm_step < it < s.lpips_start - 1000) and it % hair_mask_interval != 0
    return PretrainPhase(motion=it >= s.warm_step, warm=it > s.warm_step, hair_mask_iter=hair)


def pretrain_mouth_phase(iteration: int, K: int, opt=OptimizationParams) -> PretrainPhase:
    """pretrain_mouth.py:193-198, :230: static render below warm_step, the personalised mouth render from warm_step on
    (p_motion_start_iter = 0), the warm terms above it.  The mouth stage has no hair iterations."""
    s = pretrain_schedule(K, opt, "mouth")
    return PretrainPhase(motion=iteration >= s.warm_step, warm=iteration > s.warm_step, hair_mask_iter=False)


def motion_lr_lambda(i: int, K: int, opt=OptimizationParams, stage: str = "face") -> float:
    """The universal field's LambdaLR factor on the stage's schedule (pretrain_face.py:42, pretrain_mouth.py:90)."""
    s = pretrain_schedule(K, opt, stage)
    return 0.5 ** (i / s.mouth_select_iter) if i < s.mouth_select_iter else 0.1 ** (i / s.iterations)


class IdentitySampler:
    """The identity of each iteration, ``randint(0, K - 1)`` from a seeded generator (pretrain_face.py:55)."""

    def __init__(self, K: int, seed: int = 0):
        self.K = int(K)
        self.rng = random.Random(seed)

    def __call__(self) -> int:
        return self.rng.randint(0, self.K - 1)


class PartnerSampler:
    """The contrast partner of a mouth pretraining step (pretrain_mouth.py:261-262): ``randint(0, K - 1)`` from a seeded
    generator, redrawn until it differs from the trained identity.  K = 1 has no other identity (the reference's loop
    would not end): None, and the step carries no contrast term."""

    def __init__(self, K: int, seed: int = 0):
        self.K = int(K)
        self.rng = random.Random(seed)

    def __call__(self, idx: int) -> Optional[int]:
        if self.K < 2:
            return None
        j = self.rng.randint(0, self.K - 1)
        while j == idx:
            j = self.rng.randint(0, self.K - 1)
        return j


@torch.no_grad()
def centre_on_lips(g: GaussianModel) -> GaussianModel:
    """pretrain_mouth.py:75-77 on a fresh mouth cloud: ``_xyz /= 2; _xyz[:, 1] -= 0.05`` (in place)."""
    g._xyz.data /= 2
    g._xyz.data[:, 1] -= 0.05
    return g


def load_face_stage(root: str, names: Sequence[str], motion_net_face, make_face_gaussians):
    """What the mouth stage reads from the face stage (pretrain_mouth.py:80-98): every identity's face Gaussians from
    <root>/<name>/chkpnt_face_latest.pth (GaussianModel.restore without optimizer) and the face UMF's EMA weights from
    <root>/chkpnt_ema_face_latest.pth -- the files PretrainFaceTrainer.save_checkpoints writes.  ``make_face_gaussians()``
    builds an empty face-type GaussianModel.  -> (faces, motion_net_face)"""
    faces = []
    for name in names:
        model_params = torch.load(os.path.join(root, name, "chkpnt_face_latest.pth"), weights_only=False)[0]
        faces.append(make_face_gaussians().restore(model_params, None))
    load_pretrained_motion(motion_net_face, os.path.join(root, "chkpnt_ema_face_latest.pth"))
    return faces, motion_net_face


# ---- EMA of the UMF (torch_ema 0.3 ExponentialMovingAverage(parameters, decay=0.995)) ---------------------------------
class MotionEMA:
    """Shadows = clones of the parameters at construction; update(): n += 1, d = min(decay, (1 + n) / (10 + n)),
    s -= (1 - d) (s - p) for EVERY tensor.  ``counter`` = int32 [n, ticket] on the parameters' device: on the GPU the
    update is part of the UMF's AdamW launch (optim.MultiTensorAdamEMA), which advances n there; update() is the
    host-side statement of the same arithmetic."""

    def __init__(self, parameters, decay: float = 0.995):
        self.params = list(parameters)
        self.decay = float(decay)
        self.shadow_params = [p.detach().clone().contiguous() for p in self.params]
        self.counter = torch.zeros(2, dtype=torch.int32, device=self.params[0].device)

    @property
    def num_updates(self) -> int:
        return int(self.counter[0])

    @torch.no_grad()
    def update(self):
        n = self.num_updates + 1
        self.counter[0] = n
        one_minus_decay = 1.0 - min(self.decay, (1 + n) / (10 + n))
        for s, p in zip(self.shadow_params, self.params):
            tmp = s - p
            tmp.mul_(one_minus_decay)
            s.sub_(tmp)

    @contextlib.contextmanager
    def average_parameters(self):
        """The parameters hold the shadows inside the block (in place: captured graphs stay valid) and their own values
        again afterwards."""
        backup = [p.detach().clone() for p in self.params]
        with torch.no_grad():
            for p, s in zip(self.params, self.shadow_params):
                p.copy_(s)
        try:
            yield
        finally:
            with torch.no_grad():
                for p, b in zip(self.params, backup):
                    p.copy_(b)


# ---- checkpoints in the reference's formats (pretrain_face.py:160-171) -------------------------------------------------
def load_pretrained_motion(motion_net, path: str):
    """train_face.py:66-68: ``(motion_params, _, _) = torch.load(pretrain_ckpt_path)``, loaded into the UMF."""
    motion_params, _, _ = torch.load(path, map_location=next(motion_net.parameters()).device, weights_only=False)
    motion_net.load_state_dict(motion_params)
    return motion_net


# ---- the other identities' personalised fields, without gradient ------------------------------------------------------
@torch.no_grad()
def other_pmf_heads(pmfs: Sequence[torch.nn.Module], xyz, audio, exp) -> List[torch.Tensor]:
    """The deformation heads h_j [N,11] (mouth-type PMFs: [N,7], ``exp`` None) of the other identities' PMFs at the
    trained identity's positions (pretrain_face.py:136, pretrain_mouth.py:265): only ``_h`` -- the alignment head, whose output the contrast never reads, is skipped.  On
    the device each is the forward-only tri-plane encode, shared attention MLPs and glue + sigma_net kernels."""
    out = []
    for net in pmfs:
        enc_x = net.encode_x(xyz, bound=net.bound)
        out.append(net._trunk(xyz, audio, exp, None, enc_x=enc_x)[3])
    return out


class _PretrainTrainer:
    """What the face and the mouth pretraining share: K identities (GaussianModel with its PMF in ``neural_motion_grid``,
    each with its own training_setup optimizer), one universal field with AdamW over get_params(5e-3, 5e-4) and its EMA,
    the iteration in the reference's order, lazy capture per key into one private pool, and the checkpoints.  A stage
    supplies STAGE (the checkpoint tag), _phase, forward_loss, _density_due, _density_control and, where a step draws
    something on the host that a captured step bakes in, _draw."""

    STAGE = ""

    def __init__(self, identities: Sequence[GaussianModel], motion_net, background, opt=OptimizationParams,
                 names: Optional[Sequence[str]] = None, cameras_extent: float = 0.2, densify: bool = True,
                 seed: int = 0):
        self.ids = list(identities)
        self.K = len(self.ids)
        assert self.K >= 1
        self.names = list(names) if names is not None else [f"id{i}" for i in range(self.K)]
        self.motion_net = motion_net
        self.bg = background
        self.opt = opt
        self.sched = pretrain_schedule(self.K, opt, self.STAGE)
        self.extent = cameras_extent
        self.densify = densify
        self.iteration = 0
        dev = self.ids[0].get_xyz.device
        self.device = dev
        self.on_gpu = dev.type == "cuda"
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self.ema = MotionEMA(motion_net.parameters(), decay=0.995)
        self._check_limits()
        self.motion_optimizer = make_motion_optimizer(motion_net, self.on_gpu, ema=self.ema)
        self._motion_base_lr = [float(g["lr"]) for g in self.motion_optimizer.param_groups]
        for g in self.ids:
            g.training_setup(opt, fused=self.on_gpu)
        # what a step of identity k advances: two launches, the universal field's AdamW + EMA, then the identity's Adam
        self.optimizers = [StepOptimizers(self.motion_optimizer, g.optimizer, combine=False) for g in self.ids]
        lambda_lr(self.motion_optimizer, self._motion_base_lr, motion_lr_lambda(0, self.K, opt, self.STAGE))
        self.last = {}
        self._graph_mode = None       # set by enable_graph
        self._graph_cache = {}        # _key -> _PretrainGraph
        self._pool = None             # one private memory pool for every capture of this trainer
        self.captures = 0

    def _check_limits(self):
        pass

    # ---- what a stage supplies -------------------------------------------------------------------------------------
    def _phase(self, it) -> PretrainPhase:
        raise NotImplementedError

    def forward_loss(self, idx: int, frame, phase: PretrainPhase, drawn=None):
        raise NotImplementedError

    def _draw(self, idx, phase):
        """What the host draws for this step and a captured step bakes in (part of its key); None: nothing."""
        return None

    def _density_due(self, it):
        raise NotImplementedError

    def _density_control(self, g: GaussianModel, it, frame):
        raise NotImplementedError

    # ---- learning rates --------------------------------------------------------------------------------------------
    def _set_learning_rates(self, idx, it):
        f = motion_lr_lambda(it - 1, self.K, self.opt, self.STAGE)      # LambdaLR: step `it` runs with lambda(it - 1)
        lambda_lr(self.motion_optimizer, self._motion_base_lr, f)
        self.ids[idx].update_learning_rate(it)
        self.optimizers[idx].push_lrs()

    def _forward_backward(self, idx, frame, phase, drawn=None):
        from .losses import defer_finalize
        with defer_finalize():          # (backward follows at once; the loss value is read after the step)
            pkg, loss, l1 = self.forward_loss(idx, frame, phase, drawn)
        backward(loss, self.device)
        return pkg, loss, l1

    # ---- one iteration ---------------------------------------------------------------------------------------------
    def _body(self, idx, frame, phase, stats_on: bool, steps: bool, density_it: Optional[int] = None, drawn=None):
        """One iteration of identity ``idx`` in the reference's order: forward, loss, backward, statistics, [density
        control at iteration ``density_it``], optimizers (+ EMA).  Free of host round trips without density control
        (the captured form)."""
        g = self.ids[idx]
        pkg, loss, l1 = self._forward_backward(idx, frame, phase, drawn)
        with torch.no_grad():
            if stats_on:
                update_densification_stats(g, pkg["viewspace_points"].grad, pkg["radii"])
            if density_it is not None:
                self._density_control(g, density_it, frame)
            if steps:
                self.optimizers[idx].step()          # (+ the EMA update, in the universal field's launch)
            self.optimizers[idx].zero_grad()
        return pkg, loss, l1

    def _key(self, idx, it, drawn=None):
        """What a captured step of identity ``idx`` at iteration ``it`` bakes in."""
        key = (idx, self._phase(it), it < self.sched.densify_until, it < self.sched.iterations,
               self.ids[idx].active_sh_degree)
        return key if drawn is None else key + (drawn,)

    def step(self, idx: int, frame):
        """One iteration on identity ``idx``, in the reference's order.  In graph mode a step without a density-control
        event replays the captured step of its key, capturing it first if needed."""
        if not self.on_gpu:
            raise RuntimeError(f"{type(self).__name__}.step runs on the GPU (the pretraining operators are HIP kernels)")
        self.iteration += 1
        it = self.iteration
        g = self.ids[idx]
        phase = self._phase(it)
        drawn = self._draw(idx, phase)
        self._set_learning_rates(idx, it)
        if it % 1000 == 0:
            g.oneupSHdegree()
        due = self._density_due(it)
        stats_on, steps = it < self.sched.densify_until, it < self.sched.iterations
        if self._graph_mode is not None and not due:
            key = self._key(idx, it, drawn)
            gs = self._graph_cache.get(key)
            if gs is None:
                gs = self._graph_cache[key] = self._capture(idx, frame, key)
                self.captures += 1
            gs.replay(frame)
            loss, l1 = gs.loss, gs.l1
            if gs.check_due() and gs.check_overflow():
                # a replayed step needed more instances than its capacity (image truncated to the nearest Gaussians):
                # captured again, sized from fresh counts, when the key comes back
                del self._graph_cache[key]
        else:
            # eager launches in exact mode: another identity's plan must not size this step's rasterizer calls
            diff_gauss.set_capacity_plan(None)
            pkg, loss, l1 = self._body(idx, frame, phase, stats_on, steps, it if due else None, drawn)
            del pkg
            if due:
                # identity idx's parameter set changed: its captured steps are stale (the others' are not -- they read
                # only its personalised field, which density control leaves as it is)
                self._graph_cache = {k: v for k, v in self._graph_cache.items() if k[0] != idx}
        self.last = dict(loss=loss.detach(), l1=l1.detach(), identity=idx, num_points=g.num_points, phase=phase)
        if drawn is not None:
            self.last["drawn"] = drawn
        return self.last

    # ---- graph mode --------------------------------------------------------------------------------------------------
    def enable_graph(self, headroom: float = 1.5, warmup_steps: int = 2):
        """Switch graph mode on.  Steps are captured lazily, one per (identity, phase, statistics on, optimizers on,
        SH degree[, what the host drew]), all into one private memory pool (graphs.py protocol).  A capture does NOT
        consume iterations: its warm-up steps run on the current state, which is put back before the capture
        (parameters, optimizer moments and step counters, EMA shadows and counter, densification statistics).
        Density-control iterations run eagerly and drop the identity's captured steps; an overflow of a step's instance
        capacity drops that step."""
        assert self.on_gpu, "graph mode needs the GPU"
        if self._pool is None:
            from . import _lib
            self._pool = _lib.GraphPool(self.device)
        self._graph_mode = dict(headroom=float(headroom), warmup_steps=max(1, int(warmup_steps)))

    def disable_graph(self):
        self._graph_cache = {}
        self._graph_mode = None
        diff_gauss.set_capacity_plan(None)

    def _capture(self, idx, frame, key):
        _, phase, stats_on, steps, _ = key[:5]
        drawn = key[5] if len(key) > 5 else None
        mode, dev, it = self._graph_mode, self.device, self.iteration
        static = frame.clone_static()
        # every tensor a step of identity idx writes that outlives the step (the optimizer state created first)
        g, opts = self.ids[idx], self.optimizers[idx]
        opts.prepare()
        ts = [p.data for p in self.motion_net.parameters()] + list(self.ema.shadow_params) + [self.ema.counter]
        ts += [p.data for p in g._p.values()] + [p.data for p in g.neural_motion_grid.parameters()]
        stats = (g.xyz_gradient_accum, g.denom, g.max_radii2D)
        saved = snapshot_state(ts, opts, stats)

        def pre():
            self._set_learning_rates(idx, it)

        def one_step():
            self._body(idx, static, phase, stats_on, steps, None, drawn)

        counts = graphs.measure(one_step, mode["warmup_steps"], pre)
        plan = graphs.install(graphs.stage_capacities(counts, mode["headroom"]), dev)
        graphs.warm(plan, one_step, dev, pre)
        restore_state(saved, ts, opts, stats)
        del saved
        self._set_learning_rates(idx, it)
        graph = torch.cuda.CUDAGraph()
        with graphs.capture(graph, plan, False, pool=self._pool.handle):
            pkg, loss, l1 = self._body(idx, static, phase, stats_on, steps, None, drawn)
        del pkg
        return _PretrainGraph(graph, plan, static, loss.detach(), l1.detach())

    # ---- checkpoints (pretrain_face.py:160-171, pretrain_mouth.py:311-322) ----------------------------------------------
    def save_checkpoints(self, root: str):
        """<root>/chkpnt_<stage>_latest.pth = (universal field state_dict, optimizer state_dict, iteration);
        chkpnt_ema_<stage>_latest.pth = the same with the EMA weights; <root>/<name>/chkpnt_<stage>_{iteration,latest}.pth
        = (gaussians.capture(), field state_dict, optimizer state_dict, iteration) per identity."""
        it, tag = self.iteration, self.STAGE
        os.makedirs(root, exist_ok=True)
        torch.save((self.motion_net.state_dict(), self.motion_optimizer.state_dict(), it),
                   os.path.join(root, f"chkpnt_{tag}_latest.pth"))
        with self.ema.average_parameters():
            # (state_dict() aliases the parameters: it is written while they hold the shadows)
            torch.save((self.motion_net.state_dict(), self.motion_optimizer.state_dict(), it),
                       os.path.join(root, f"chkpnt_ema_{tag}_latest.pth"))
        for name, g in zip(self.names, self.ids):
            d = os.path.join(root, name)
            os.makedirs(d, exist_ok=True)
            ckpt = (g.capture(), self.motion_net.state_dict(), self.motion_optimizer.state_dict(), it)
            torch.save(ckpt, os.path.join(d, f"chkpnt_{tag}_{it}.pth"))
            torch.save(ckpt, os.path.join(d, f"chkpnt_{tag}_latest.pth"))


class PretrainFaceTrainer(_PretrainTrainer):
    """K identities and one UMF with AdamW(get_params(5e-3, 5e-4), betas (0.9, 0.99), eps 1e-8, weight decay 0.01:
    pretrain_face.py:135 passes none, so torch's default applies) and its EMA (pretrain_face.py:53-193)."""

    STAGE = "face"

    def __init__(self, identities: Sequence[GaussianModel], motion_net, background, opt=OptimizationParams,
                 names: Optional[Sequence[str]] = None, cameras_extent: float = 0.2, densify: bool = True,
                 seed: int = 0, share_audio_net: bool = False):
        if share_audio_net:
            raise NotImplementedError(
                "share_audio_net: the UMF's audio-net tensors would sit in the UMF's optimizer and in every identity's "
                "optimizer, and one fused Adam launch over both would update the same tensors twice, racing")
        super().__init__(identities, motion_net, background, opt, names, cameras_extent, densify, seed)

    def _check_limits(self):
        if self.on_gpu:
            from . import _lib
            if self.K - 1 > _lib.lib().instag_pretrain_deform_max_others():
                raise ValueError(f"at most {_lib.lib().instag_pretrain_deform_max_others() + 1} identities")

    def _phase(self, it):
        return pretrain_phase(it, self.K, self.opt)

    # ---- forward + loss --------------------------------------------------------------------------------------------
    def forward_loss(self, idx: int, frame, phase: PretrainPhase, drawn=None):
        """-> (pkg, loss, Ll1) of identity ``idx`` on ``frame`` (no backward)."""
        from .renderer import render, render_motion
        g = self.ids[idx]
        dev = self.device
        td = frame.talking_dict
        face, hair, mouth = td["face_mask"].to(dev), td["hair_mask"].to(dev), td["mouth_mask"].to(dev)
        gt = frame.original_image.to(dev)
        if not phase.motion:
            pkg = render(frame, g, None, self.bg)
            loss, l1 = face_loss(pkg["render"], gt, face, hair, mouth, self.bg, lambda_dssim=self.opt.lambda_dssim)
            return pkg, loss, l1
        heads = []
        if phase.warm and self.K > 1:
            heads = other_pmf_heads([o.neural_motion_grid for j, o in enumerate(self.ids) if j != idx], g.get_xyz,
                                    td["auds"].to(dev), td["au_exp"].to(dev))
        pkg = render_motion(frame, g, self.motion_net, None, self.bg, return_attn=True, personalized=True,
                            align=False, pretrain_heads=heads, pretrain_reg=phase.warm,
                            need_geometry=False)      # (no loss term of this step reads depth / normal)
        if not phase.warm:
            loss, l1 = face_loss(pkg["render"], gt, face, hair, mouth, self.bg, lambda_dssim=self.opt.lambda_dssim)
            return pkg, loss, l1
        from .glue import window_mean_append
        lips = td["lips_rect"].to(dev)
        extra = window_mean_append(pkg["p_attn"], pkg["motion_reg"], lips, 1, 5e-3)
        loss, l1 = face_loss(pkg["render"], gt, face, hair, mouth, self.bg, alpha=pkg["alpha"], attn=pkg["attn"],
                             lips_rect=lips, extra=extra, lambda_dssim=self.opt.lambda_dssim, w_alpha=1e-3,
                             w_attn=1e-4, w_lips=5e-3, w_extra=1.0, hair_mask_iter=phase.hair_mask_iter)
        return pkg, loss, l1

    # ---- density control ------------------------------------------------------------------------------------------
    def _density_due(self, it):
        o = self.opt
        return self.densify and it > o.densify_from_iter and it % o.densification_interval == 0

    @torch.no_grad()
    def _density_control(self, g: GaussianModel, it, frame):
        """pretrain_face.py:172-186: densify_and_prune (before densify_until), then the green-Gaussian prune (no bound).
        No opacity reset: pretrain_face.py has none."""
        if it < self.sched.densify_until:
            densify_and_prune_at(g, it, self.sched.densify_until, self.opt, self.extent, self.gen)
        g.prune_points(green_mask(g, frame.camera_center.to(self.device), FACE_GREEN))


MOUTH_PRETRAIN_GREEN = (20, 235, 20)       # green_mask thresholds of pretrain_mouth.py:341


class PretrainMouthTrainer(_PretrainTrainer):
    """Identity-free pretraining of the universal MOUTH motion field (pretrain_mouth.py:113-358).  ``identities``: the K
    mouth clouds, each with a mouth-type PMF (hidden 16, 7 outputs) in ``neural_motion_grid``; ``faces``: their frozen
    face Gaussians; ``motion_net_face``: the frozen face UMF -- both only supply the jaw-movement feature.  The shared
    MouthMotionNetwork trains with AdamW(get_params(5e-3, 5e-4), betas (0.9, 0.99), eps 1e-8) (:89: its groups carry
    weight_decay = 0 themselves except the three encoders, which take torch's default 0.01, and the audio attention net's
    1e-4) and EMA 0.995.  An iteration: static render before warm_step, then render_motion_mouth_con(personalized=True,
    align=False) with the default k = 10; mouth compositing loss; after warm_step the regularisers of both fields, the
    alpha term and the contrast against ONE other identity (``drawn``, from PartnerSampler; none at K = 1).
    ``fused_deform=False`` (measurement only): today's torch-composed personalised branch and torch loss terms instead of
    glue.pretrain_mouth_deform."""

    STAGE = "mouth"

    def __init__(self, identities: Sequence[GaussianModel], motion_net, faces: Sequence[GaussianModel], motion_net_face,
                 background, opt=OptimizationParams, names: Optional[Sequence[str]] = None,
                 cameras_extent: float = 0.2, densify: bool = True, seed: int = 0, fused_deform: bool = True):
        self.faces = list(faces)
        assert len(self.faces) == len(identities)
        self.motion_net_face = motion_net_face
        self.fused_deform = bool(fused_deform)
        self.partner = PartnerSampler(len(identities), seed)
        super().__init__(identities, motion_net, background, opt, names, cameras_extent, densify, seed)

    def _phase(self, it):
        return pretrain_mouth_phase(it, self.K, self.opt)

    def _draw(self, idx, phase):
        # (pretrain_mouth.py:261-262 draws inside `iteration > warm_step`: no draw, and no key entry, before that)
        return self.partner(idx) if phase.warm else None

    # ---- forward + loss (pretrain_mouth.py:193-276) ----------------------------------------------------------------
    def forward_loss(self, idx: int, frame, phase: PretrainPhase, drawn=None):
        """-> (pkg, loss, Ll1) of identity ``idx`` on ``frame`` (no backward); ``drawn`` = the contrast partner."""
        from .losses import mouth_loss_fused
        from .renderer import render, render_motion_mouth_con
        g, dev, td = self.ids[idx], self.device, frame.talking_dict
        mouth, lips, gt = td["mouth_mask"].to(dev), td["lips_rect"].to(dev), frame.original_image.to(dev)
        lam = self.opt.lambda_dssim
        if not phase.motion:
            pkg = render(frame, g, None, self.bg)
            loss, l1 = mouth_loss_fused(pkg["render"], None, gt, mouth, lips, self.bg, warm=False, lambda_dssim=lam)
            return pkg, loss, l1
        other = None
        if phase.warm and drawn is not None:
            other = other_pmf_heads([self.ids[drawn].neural_motion_grid], g.get_xyz, td["auds"].to(dev), None)[0]
        if not self.fused_deform:
            pkg = render_motion_mouth_con(frame, g, self.motion_net, self.faces[idx], self.motion_net_face, None, self.bg,
                                          personalized=True, align=False)
            extra = composed_mouth_terms(pkg["motion"], pkg["p_motion"], other).reshape(1) if phase.warm else None
        else:
            pkg = render_motion_mouth_con(frame, g, self.motion_net, self.faces[idx], self.motion_net_face, None, self.bg,
                                          personalized=True, align=False, pretrain_other=other, pretrain_reg=phase.warm)
            extra = pkg["motion_reg"]
        loss, l1 = mouth_loss_fused(pkg["render"], pkg["alpha"], gt, mouth, lips, self.bg, warm=phase.warm,
                                    lambda_dssim=lam, extra=extra)
        return pkg, loss, l1

    # ---- density control (pretrain_mouth.py:325-347) ---------------------------------------------------------------
    def _density_due(self, it):
        o = self.opt
        return (self.densify and it < self.sched.densify_until and it > o.densify_from_iter
                and it % o.densification_interval == 0)

    @torch.no_grad()
    def _density_control(self, g: GaussianModel, it, frame):
        """densify_and_prune, then the Gaussians that took the background's green are damped: statistics halved, opacity
        to 0.1, scale / 10.  No prune by colour and no opacity reset."""
        densify_and_prune_at(g, it, self.sched.densify_until, self.opt, self.extent, self.gen)
        green = green_mask(g, frame.camera_center.to(self.device), MOUTH_PRETRAIN_GREEN)
        g.xyz_gradient_accum[green] /= 2
        g._opacity.data[green] = g.inverse_opacity_activation(torch.ones_like(g._opacity.data[green]) * 0.1)
        g._scaling.data[green] /= 10


def composed_mouth_terms(motion, p_motion, other_head=None):
    """The per-Gaussian loss terms of pretrain_mouth.py:231-276 from a render_motion_mouth_con(personalized=True)
    package with torch operators (the path glue.pretrain_mouth_deform replaces): ``motion['d_xyz']`` there is the mouth
    field's own displacement, so the reference's in-place sum is formed here."""
    p_xyz, p_rot = p_motion["d_xyz"], p_motion["d_rot"]
    total = 1e-5 * (motion["d_xyz"] + p_xyz).abs().mean() + 1e-5 * motion["d_rot"].abs().mean()
    total = total + 1e-5 * p_xyz.abs().mean() + 1e-5 * p_rot.abs().mean()
    if other_head is not None:
        total = total + torch.relu(((other_head[..., :3] * 1e-2) * p_xyz).sum(-1)).mean()
    return total


class _PretrainGraph(graphs.CapturedStep):
    """One captured pretraining step with its capacity plan, static frame and (detached) loss outputs."""

    def __init__(self, graph, plan, static, loss, l1):
        self.graph, self.plan, self.static, self.loss, self.l1 = graph, plan, static, loss, l1

    def replay(self, frame):
        self._replays += 1
        self.static.copy_from(frame)
        self.graph.replay()


def build_pretrainer(K: int, n_gaussians: int, device, sh_degree: int = 1, seed: int = 0, opt=OptimizationParams,
                     densify: bool = False, audio_extractor: str = "deepspeech") -> PretrainFaceTrainer:
    """Synthetic K-identity pretrainer: K clouds of n_gaussians (different seeds) with their PMFs, one UMF."""
    from types import SimpleNamespace
    from .motion_net import MotionNetwork, PersonalizedMotionNetwork
    from .scene_synth import synthetic_gaussians
    torch.manual_seed(seed)
    args = SimpleNamespace(audio_extractor=audio_extractor, type="face")
    ids = []
    for k in range(K):
        pmf = PersonalizedMotionNetwork(args=args).to(device)
        g = GaussianModel(sh_degree, neural_motion_grid=pmf)
        g.load_raw(synthetic_gaussians(n_gaussians, sh_degree=sh_degree, seed=seed + k), device)
        ids.append(g)
    umf = MotionNetwork(args=args).to(device)
    bg = torch.tensor([0.0, 1.0, 0.0], device=device)
    return PretrainFaceTrainer(ids, umf, bg, opt=opt, densify=densify, seed=seed)


def build_mouth_pretrainer(K: int, n_mouth: int, n_face: int, device, sh_degree: int = 1, seed: int = 0,
                           opt=OptimizationParams, densify: bool = False, fused_deform: bool = True,
                           audio_extractor: str = "deepspeech") -> PretrainMouthTrainer:
    """Synthetic K-identity mouth pretrainer: K mouth clouds of n_mouth Gaussians (different seeds, centred on the lips)
    with their mouth-type PMFs, K frozen face clouds of n_face with a frozen face UMF, one MouthMotionNetwork."""
    from types import SimpleNamespace
    from .motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    from .scene_synth import synthetic_gaussians
    torch.manual_seed(seed)
    face_args = SimpleNamespace(audio_extractor=audio_extractor, type="face")
    mouth_args = SimpleNamespace(audio_extractor=audio_extractor, type="mouth")
    ids, faces = [], []
    for k in range(K):
        g = GaussianModel(sh_degree, neural_motion_grid=PersonalizedMotionNetwork(args=mouth_args).to(device))
        g.load_raw(synthetic_gaussians(n_mouth, sh_degree=sh_degree, seed=seed + k), device)
        ids.append(centre_on_lips(g))
        f = GaussianModel(sh_degree, neural_motion_grid=PersonalizedMotionNetwork(args=face_args).to(device))
        faces.append(f.load_raw(synthetic_gaussians(n_face, sh_degree=sh_degree, seed=seed + 100 + k), device))
    face_umf = MotionNetwork(args=face_args).to(device)
    umf = MouthMotionNetwork(args=mouth_args).to(device)
    bg = torch.tensor([0.0, 1.0, 0.0], device=device)
    return PretrainMouthTrainer(ids, umf, faces, face_umf, bg, opt=opt, densify=densify, seed=seed,
                                fused_deform=fused_deform)
