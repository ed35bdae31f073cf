"""One adaptation train step of InsTaG's face branch on synthetic frames, single- or multi-GPU.

Counterpart of /root/reference/train_face.py:110-788 restricted to the hot path: render_motion
(:346-350) -> L1 + 0.2*(1-SSIM) (:450-456) + regularisers (:508-540) -> backward (:625) ->
densification statistics / density control (:667-746) -> AdamW / Adam steps (:781-788), in the reference's
iteration-dependent phases (face_phase: alignment, warm terms, hair iterations, monocular normal / depth
priors :458-504, the late phase's LPIPS patch term :333-335, 596-620 with ``FaceTrainer(..., lpips=LPIPSWeights)``).
Logging is out of scope.

Two execution modes with identical arithmetic:
  * eager  -- every operator is launched from Python (one host round trip per rasterizer pass);
  * graph  -- the whole step (forward, backward, statistics, optimizers) is captured ONCE into a
    hipGraph (torch.cuda.CUDAGraph) and replayed; the rasterizer runs in its sync-free capacity mode
    (diff_gauss.CapacityPlan), per-frame inputs are copied into static device buffers, learning rates
    live in device scalars.  The step is launch-bound in eager mode (~590 kernels), so this is the
    MI355X-native way to run it.

Data parallelism over frames (an addition): identical replicas, rank r renders its
own frame, gradients of [Gaussians | UMF | PMF] are flattened into ONE bucket and all-reduced
(RCCL over xGMI; gloo in the CPU tests); densification statistics stay per-rank sums / maxima and are
exchanged when a densification reads them, so every replica applies identical optimizer and
densify/prune decisions with one collective per step.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, Optional

import os
import random
import torch
import torch.distributed as dist

from . import _lib, graphs
from .deferred import backward, deferred_grads, root_gradient
from .gaussian_model import GaussianModel, OptimizationParams, green_mask
from .losses import face_loss
from .optim import StepOptimizers, lambda_lr, make_motion_optimizer


@dataclass
class Frame:
    """What the reference keeps per camera: matrices + talking_dict (scene/cameras.py, dataset_readers.py)."""
    image_height: int
    image_width: int
    FoVx: float
    FoVy: float
    world_view_transform: torch.Tensor
    full_proj_transform: torch.Tensor
    camera_center: torch.Tensor
    talking_dict: dict
    original_image: torch.Tensor      # [3,H,W] in [0,1]

    TENSORS = ("world_view_transform", "full_proj_transform", "camera_center", "original_image")
    DICT_TENSORS = ("auds", "au_exp", "face_mask", "hair_mask", "mouth_mask", "lips_rect")
    # present only for the stages that read them: monocular normal [3,H,W] / depth [H,W] priors
    # (train_face.py:466-504), per-camera scene background [3,H,W] in [0,1] (train_fuse_con.py:113)
    OPTIONAL_DICT_TENSORS = ("normal", "depth", "background")

    def _dict_keys(self):
        return self.DICT_TENSORS + tuple(k for k in self.OPTIONAL_DICT_TENSORS if self.talking_dict.get(k) is not None)

    def _named_tensors(self):
        return [(k, getattr(self, k)) for k in self.TENSORS] + [(k, self.talking_dict[k]) for k in self._dict_keys()]

    def packed(self, device=None, pin: bool = False) -> "Frame":
        """Copy whose tensors are views into ONE byte buffer, so that feeding a frame to a captured step is a
        single device copy instead of one per tensor.  ``pin`` (host copies): page-locked memory, so that the upload
        of the whole frame is one asynchronous copy (HostFrameFeeder)."""
        named = self._named_tensors()
        device = device if device is not None else named[0][1].device
        offs, total = [], 0
        for _, t in named:
            offs.append(total)
            total += (t.numel() * t.element_size() + 255) // 256 * 256
        buf = torch.zeros(total, dtype=torch.uint8, device=device)
        if pin and buf.device.type == "cpu":
            buf = buf.pin_memory()
        views = {}
        for (k, t), o in zip(named, offs):
            nbytes = t.numel() * t.element_size()
            v = buf[o:o + nbytes].view(t.dtype).view(t.shape)
            v.copy_(t)
            views[k] = v
        td = {k: views[k] for k in self._dict_keys()}
        f = Frame(self.image_height, self.image_width, self.FoVx, self.FoVy, views["world_view_transform"],
                  views["full_proj_transform"], views["camera_center"], td, views["original_image"])
        f._buf = buf
        f._layout = tuple((k, tuple(t.shape), t.dtype) for k, t in named)
        return f

    def clone_static(self):
        return self.packed()

    def copy_from(self, other: "Frame"):
        assert (self.image_height, self.image_width) == (other.image_height, other.image_width)
        assert abs(self.FoVx - other.FoVx) < 1e-12 and abs(self.FoVy - other.FoVy) < 1e-12, \
            "graph mode bakes the field of view into the captured launches"
        if not isinstance(other, Frame):
            from .frame_store import StoredFrame
            if isinstance(other, StoredFrame):         # a frame of a device-resident 8-bit store: one unpack launch
                other.store.unpack_into(self, other.index)
                return
        if getattr(self, "_buf", None) is not None and getattr(other, "_buf", None) is not None \
                and self._layout == other._layout:
            self._buf.copy_(other._buf, non_blocking=True)
            return
        for k in self.TENSORS:
            getattr(self, k).copy_(getattr(other, k), non_blocking=True)
        for k in self._dict_keys():
            self.talking_dict[k].copy_(other.talking_dict[k], non_blocking=True)


class HostFrameFeeder:
    """Frames that live in (pinned) HOST memory, uploaded ahead of the step that reads them.

    The reference uploads a frame's tensors inside the iteration that uses them (train_face.py:324-327 masks and image,
    gaussian_renderer/__init__.py:188-189 audio window and expression vector: a handful of blocking ``.cuda()`` copies,
    ~4 MB at 512x512).  Here a frame is ONE packed byte buffer (Frame.packed): while step i runs, frame i+1 travels on a
    second stream into one of ``slots`` device staging buffers, and step i+1's first action -- the device-to-device copy
    into the captured step's static frame -- reads the staging buffer.

    All ordering is done on the HOST (event.synchronize(), no stream-to-stream waits): a cross-stream wait is a barrier
    packet in front of the replayed graph, and two of them per step cost 2.6 % of the step (scripts/probes/
    host_frames_probe2.py: 0.933 -> 0.958 ms), more than the upload itself, which overlaps (0.938 ms).  The host runs a few
    steps ahead of the device in replay mode, so a staging slot is reused only ``slots`` steps later and the host-side
    wait for its last reader returns at once."""

    def __init__(self, example: Frame, device, slots: int = 4):
        self.device = torch.device(device)
        self.slots = int(slots)
        self.stage = [example.packed(self.device) for _ in range(self.slots)]
        # (no stream of its own: the capture warm-up stream exists anyway and is idle outside enable_graph)
        self.stream = _lib.warmup_stream(self.device)
        self.ready = [torch.cuda.Event() for _ in range(self.slots)]
        self.consumed = [torch.cuda.Event() for _ in range(self.slots)]
        for e in self.consumed:
            e.record(torch.cuda.current_stream(self.device))

    @staticmethod
    def to_host(frame: Frame) -> Frame:
        return frame.packed("cpu", pin=True)

    def prefetch(self, host_frame: Frame, slot: int):
        """Start the upload of ``host_frame`` into staging slot ``slot`` (once the slot's last reader has finished)."""
        self.consumed[slot].synchronize()
        with torch.cuda.stream(self.stream):
            self.stage[slot].copy_from(host_frame)
            self.ready[slot].record(self.stream)

    def take(self, slot: int) -> Frame:
        """The staged frame (its upload has completed when this returns)."""
        self.ready[slot].synchronize()
        return self.stage[slot]

    def release(self, slot: int):
        """Everything enqueued on the current stream so far is the last reader of staging slot ``slot``."""
        self.consumed[slot].record(torch.cuda.current_stream(self.device))

    def run(self, step, host_frames, n: int):
        """``step(frame)`` over n frames (host_frames cyclically), each uploaded one step ahead."""
        k = self.slots
        self.prefetch(host_frames[0], 0)
        for i in range(n):
            if i + 1 < n:
                self.prefetch(host_frames[(i + 1) % len(host_frames)], (i + 1) % k)
            step(self.take(i % k))
            self.release(i % k)


def make_frame(cam, frame_data) -> Frame:
    td = dict(auds=frame_data["auds"], au_exp=frame_data["au_exp"], face_mask=frame_data["face_mask"],
              hair_mask=frame_data["hair_mask"], mouth_mask=frame_data["mouth_mask"],
              lips_rect=frame_data["lips_rect"])
    for k in Frame.OPTIONAL_DICT_TENSORS:
        if frame_data.get(k) is not None:
            td[k] = frame_data[k]
    f = Frame(cam.image_height, cam.image_width, cam.FoVx, cam.FoVy, cam.world_view_transform,
              cam.full_proj_transform, cam.camera_center, td, frame_data["gt_image"])
    return f.packed() if frame_data["gt_image"].is_cuda else f


def with_grad(params: List[torch.Tensor]) -> List[torch.Tensor]:
    """The parameters that received a gradient this step.  Which ones do depends on the step's phase only (e.g. the
    personalised field's deformation head is never evaluated with personalized=False), so every rank gets the same
    list; a parameter without gradient is not exchanged and -- as on one GPU -- not stepped."""
    return [p for p in params if p.grad is not None]


def flat_grad_bucket(params: List[torch.Tensor]) -> torch.Tensor:
    """Concatenate the gradients of ``params`` (all of which have one, see with_grad) into one contiguous fp32 bucket."""
    return torch.cat([p.grad.reshape(-1) for p in params])


def scatter_grad_bucket(params: List[torch.Tensor], bucket: torch.Tensor):
    """Hand the reduced gradients back as VIEWS of the bucket (no copy: ~45 parameter tensors would be ~45 launches per
    step, a third of a captured step's time).  The bucket must stay alive and untouched until the optimizers have read
    it -- it does: the next step's gradients are concatenated into a fresh tensor (eager) / the captured step rewrites
    it only in its first graph, the optimizers run in the second."""
    o = 0
    for p in params:
        n = p.numel()
        p.grad = bucket[o:o + n].view_as(p)
        o += n


def allreduce_gradients(params: List[torch.Tensor], extras: Optional[List[torch.Tensor]] = None, average=True):
    """One fused-bucket all-reduce(SUM) of all gradients (+ extra stat tensors, summed not averaged)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    world = dist.get_world_size()
    extras = extras or []
    params = with_grad(params)
    if not params and not extras:
        return                      # nothing to exchange (same on every rank: the set depends on the phase only)
    g = flat_grad_bucket(params) if params else torch.empty(0, dtype=extras[0].dtype, device=extras[0].device)
    n_g = g.numel()
    bucket = torch.cat([g] + [e.reshape(-1).to(g.dtype) for e in extras])
    dist.all_reduce(bucket, op=dist.ReduceOp.SUM)
    if average:
        bucket[:n_g] /= world
    scatter_grad_bucket(params, bucket[:n_g])
    o = n_g
    for e in extras:
        e.copy_(bucket[o:o + e.numel()].view_as(e))
        o += e.numel()


@dataclass(frozen=True)
class FacePhase:
    """What a face-branch iteration computes (train_face.py:340-350, 426-575)."""
    align: bool = True             # personalised field's alignment on (iteration > 1000)
    warm: bool = True              # iteration > warm_step: motion / alpha / attention regularisers
    hair_mask_iter: bool = False   # hair painted to background in image and target, hair attention terms off
    priors: bool = False           # iteration > warm_step + 2000: monocular-normal term
    prior_depth: bool = False      # ... and, outside the 100 iterations after an opacity reset, the depth term


C3_PHASE = FacePhase()             # the phase config C3 / bench.py measures (warm_step < iteration <= warm_step + 2000)
FACE_GREEN = (30, 225, 30)         # green_mask thresholds of the face branch (train_face.py:735, pretrain_face.py:183)


def face_phase(iteration: int, opt=OptimizationParams, warm_step: int = 3000, hair_mask_interval: int = 7,
               mode_long: bool = False) -> FacePhase:
    """Phase of iteration `iteration` under the reference's schedule (train_face.py:39-46, 340-350, 458-478)."""
    lpips_start_iter = opt.densify_until_iter - 1500
    hair = (warm_step < iteration < lpips_start_iter - 1000) and iteration % hair_mask_interval != 0
    align = iteration > 1000 if iteration < warm_step else True
    priors = (not mode_long) and iteration > warm_step + 2000
    return FacePhase(align=align, warm=iteration > warm_step, hair_mask_iter=hair, priors=priors,
                     prior_depth=priors and iteration % opt.opacity_reset_interval > 100)


def motion_lr_factor(i: int, warm_step: int, iterations: int) -> float:
    """The motion field's LambdaLR factor after ``i`` scheduler steps (train_face.py:60, train_mouth.py:64): x0.1 during
    warm-up, then 0.5^(i / iterations)."""
    return 0.1 if i < warm_step else 0.5 ** (i / iterations)


@torch.no_grad()
def update_densification_stats(g: GaussianModel, vs_grad, radii, grad_add=None):
    """Densification statistics of one rendered frame (train_face.py:670-671; scene/gaussian_model.py:683-685): the
    densify_stats kernel, torch operators where its layout does not hold.  With several ranks they stay LOCAL sums /
    maxima and are exchanged once, when a densification reads them (FaceTrainer.sync_densification_stats): sum and max
    commute with the per-step accumulation."""
    if vs_grad.is_cuda and g.max_radii2D.dtype == torch.float32 and radii.dtype == torch.int32 \
            and vs_grad.is_contiguous():
        from .glue import densify_stats
        densify_stats(vs_grad, radii, g.max_radii2D, g.xyz_gradient_accum, g.denom, grad_add)
        return
    if grad_add is not None:
        vs_grad.add_(grad_add)
    vis = radii > 0
    rmax = torch.where(vis, radii.to(g.max_radii2D.dtype), torch.zeros_like(g.max_radii2D))
    g.max_radii2D.copy_(torch.max(g.max_radii2D, rmax))
    g.add_densification_stats(vs_grad, vis)


@torch.no_grad()
def densify_and_prune_at(g: GaussianModel, it: int, until: int, opt, extent: float, generator):
    """The reference's densify_and_prune call at iteration ``it`` of a schedule that densifies until ``until``
    (train_face.py:675-678, train_mouth.py:268-271, pretrain_face.py:176-179)."""
    size_threshold = 20 if it > opt.opacity_reset_interval else None
    g.densify_and_prune(opt.densify_grad_threshold, 0.05 + 0.25 * it / until, extent, size_threshold,
                        generator=generator)


_MOMENTS = ("exp_avg", "exp_avg_sq", "step")


@torch.no_grad()
def snapshot_state(tensors, optimizers: StepOptimizers, stats):
    """Copies of a training state: ``tensors`` (parameters and whatever else a step writes), the optimizers' moments
    and step counters, the densification statistics ``stats``."""
    opt = [None if not st else {k: st[k].detach().clone() for k in _MOMENTS if torch.is_tensor(st.get(k))}
           for st in optimizers.states()]
    return dict(params=[t.detach().clone() for t in tensors], opt=opt, stats=[t.detach().clone() for t in stats])


@torch.no_grad()
def restore_state(snap, tensors, optimizers: StepOptimizers, stats):
    """Copy a snapshot_state() back IN PLACE (same parameter set required), so captured graphs stay valid.  Optimizer
    state that did not exist yet at the snapshot (no step had run) goes back to zero moments and a zero step count,
    which is what a first step starts from."""
    assert len(tensors) == len(snap["params"]), "the parameter set changed since the snapshot"
    for t, src in zip(tensors, snap["params"]):
        assert t.shape == src.shape, "the parameter set changed since the snapshot"
        t.copy_(src)
    for st, saved in zip(optimizers.states(), snap["opt"]):
        if not st:
            continue
        for k in _MOMENTS:
            if torch.is_tensor(st.get(k)):
                if saved and k in saved:
                    st[k].copy_(saved[k])
                else:
                    st[k].zero_()
    for dst, src in zip(stats, snap["stats"]):
        dst.copy_(src)


_DENSITY_WARM = set()


@torch.no_grad()
def warm_density_control(device, sh_degree: int = 1, opt=OptimizationParams):
    """Run every torch operator of a density-control event once, on a 256-Gaussian dummy model.  torch loads a kernel's
    code object on the kernel's first launch; the masked gathers, concatenations, random draws and reductions of
    densify / prune / opacity reset otherwise pay that (~0.8 s in total on this image) inside the first event of a run,
    with the device idle.  Called once per device by FaceTrainer.enable_graph when density control is on."""
    device = torch.device(device)
    key = (device.type, device.index, sh_degree)
    if key in _DENSITY_WARM or device.type != "cuda":
        return
    _DENSITY_WARM.add(key)
    g = GaussianModel(sh_degree).create_random(256, device, seed=0)
    g.training_setup(opt, fused=True)
    gen = torch.Generator(device=device).manual_seed(0)
    for _ in range(2):
        n = g.num_points
        g.xyz_gradient_accum = torch.rand(n, 1, device=device)
        g.denom = torch.ones(n, 1, device=device)
        g.max_radii2D = torch.rand(n, device=device) * 30.0
        g._p["scaling"].data[: n // 2] -= 3.0                        # both the clone and the split selection non-empty
        g.densify_and_prune(0.5, 0.005, 0.2, 20, generator=gen)
        g.reset_opacity()
        g.prune_points(green_mask(g, torch.zeros(3, device=device), FACE_GREEN))
        g.prune_points(g.get_xyz[:, -1] < -0.07)
    torch.cuda.synchronize(device)


class FaceTrainer:
    """Holds the Gaussians, the UMF (motion_net) and the PMF (gaussians.neural_motion_grid) and steps them.
    ``schedule=None`` runs every step in the C3 phase; ``schedule="reference"`` follows train_face.py's
    iteration-dependent phases (face_phase) and its densification order."""

    def __init__(self, gaussians: GaussianModel, motion_net, background, opt=OptimizationParams,
                 cameras_extent: float = 0.2, densify: bool = True, seed: int = 0, schedule: Optional[str] = None,
                 warm_step: int = 3000, lpips=None):
        """``lpips`` (instag_amd.lpips.LPIPSWeights): with ``schedule="reference"`` the iterations above
        densify_until_iter - 1500 close the mouth mask and add 0.01 * PatchLPIPS(image_white, gt_image_white, p,
        lips_rect, bg), p = 2 * randint(32, 48) (train_face.py:333-335, 596-620)."""
        assert schedule in (None, "reference")
        self.schedule = schedule
        self.warm_step = warm_step
        self.g = gaussians
        self.motion_net = motion_net
        self.bg = background
        self.opt = opt
        self.extent = cameras_extent
        self.densify = densify
        self.iteration = 0
        dev = gaussians.get_xyz.device
        self.device = dev
        self.gen = torch.Generator(device=dev).manual_seed(seed)     # identical on every rank
        self.on_gpu = dev.type == "cuda"
        # learning rates are device scalars on the GPU, so that a captured step can be replayed
        self.motion_optimizer = make_motion_optimizer(motion_net, self.on_gpu)
        self._motion_base_lr = [float(g["lr"]) for g in self.motion_optimizer.param_groups]
        self.g.training_setup(self.opt, fused=self.on_gpu)
        # on the GPU one launch steps both (train_face.py:781-788 steps them back to back)
        self.optimizers = StepOptimizers(self.motion_optimizer, self.g.optimizer)
        self.last = {}
        self._graph = None            # the captured step replayed last
        self._graph_cache = {}        # phase -> captured step
        self._graph_mode = None       # set by enable_graph: headroom / split / sticky capacity of the captured steps
        self._pool = None             # one private memory pool for every capture of this trainer (re-captures reuse it)
        self.lpips = lpips
        self.rng = random.Random(seed)                                  # patch size, train_face.py:609
        self._patch_op = None
        # the LPIPS patch size of the step being run: a host int (eager launches), "device" (a captured step reads
        # _p_dev, which rides on the learning-rate upload like MouthTrainer._k_dev), None = the term is off
        self._lpips_p = None
        self._p_own = None
        if lpips is not None and self.on_gpu:
            self._p_own = torch.full((1,), 64, dtype=torch.int64, device=dev)
            if self.optimizers.combined is not None:
                self.optimizers.combined.reserve_extra_i64(1)
        self.recaptures = 0
        self.recapture_seconds = 0.0  # host time of the re-captures
        self.density_seconds = 0.0    # host time of the density-control events (they synchronise)

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

    def lpips_on(self, it: int) -> bool:
        from .lpips import face_lpips_on
        return self.lpips is not None and self.schedule == "reference" and face_lpips_on(it, self.opt)

    def _set_learning_rates(self, it):
        """Per-step schedules (train_face.py:60, scene/gaussian_model.py:421-427) written into the lr slots."""
        f = motion_lr_factor(it - 1, self.warm_step, self.opt.iterations)      # LambdaLR: step `it` runs with lambda(it - 1)
        lambda_lr(self.motion_optimizer, self._motion_base_lr, f)
        self.g.update_learning_rate(it)
        self.optimizers.push_lrs()          # one small copy into the device-side learning-rate table

    def _all_params(self):
        ps = self.g.per_gaussian_parameters()
        ps += [p for p in self.motion_net.parameters()]
        if self.g.neural_motion_grid is not None:
            ps += [p for p in self.g.neural_motion_grid.parameters()]
        return ps

    # ---- loss block (train_face.py:450-456, 508-540) --------------------------------------------------------
    def phase_of(self, it: int) -> FacePhase:
        return face_phase(it, self.opt, self.warm_step) if self.schedule == "reference" else C3_PHASE

    def loss_fn(self, frame: Frame, pkg, warm: bool, hair_mask_iter: bool = False, priors: bool = False,
                prior_depth: bool = False, lpips_p=None):
        """-> (loss, Ll1).  `warm` = iteration > warm_step: motion regularisers, alpha and attention terms;
        `priors` / `prior_depth`: the monocular normal / depth terms of train_face.py:458-504; `lpips_p`: the patch
        size of the late phase's LPIPS term (:333-335 closed mouth mask, :596-620), None = off."""
        dev = self.bg.device
        td = frame.talking_dict
        mouth_mask = td["mouth_mask"].to(dev)
        if lpips_p is not None:
            from .lpips import close_mask
            mouth_mask = close_mask(mouth_mask)
        extra = alpha = attn = lips = None
        w_extra = 1e-5
        if warm:
            m, pm = pkg["motion"], pkg["p_motion"]
            if pkg.get("motion_reg") is not None:
                extra, w_extra = pkg["motion_reg"], 1.0        # already weighted, computed by the deform operator
            else:
                # (the dictionary entries: render_motion has written the combined, scaled displacements back into
                # them, as the reference's in-place arithmetic does)
                extra = (m["d_xyz"].abs().mean() + m["d_rot"].abs().mean() + m["d_opa"].abs().mean()
                         + m["d_scale"].abs().mean() + pm["p_xyz"].abs().mean())
            alpha, attn, lips = pkg["alpha"], pkg["attn"], td["lips_rect"].to(dev)
        loss, Ll1 = face_loss(pkg["render"], frame.original_image.to(dev), td["face_mask"].to(dev),
                              td["hair_mask"].to(dev), mouth_mask, self.bg, alpha=alpha, attn=attn,
                              lips_rect=lips, extra=extra, lambda_dssim=self.opt.lambda_dssim, w_extra=w_extra,
                              hair_mask_iter=hair_mask_iter)
        if priors:
            from .losses import geometry_prior_loss
            loss = loss + geometry_prior_loss(pkg["normal"], pkg["depth"], td["normal"].to(dev),
                                              td["depth"].to(dev) if prior_depth else None, td["face_mask"].to(dev),
                                              td["hair_mask"].to(dev), mouth_mask, use_depth=prior_depth)
        if lpips_p is not None:
            from .lpips import FACE_LPIPS_WEIGHT, FACE_PATCH_RANGE, PatchLPIPS
            gt = frame.original_image.to(dev)
            keep = (td["face_mask"].to(dev) | td["hair_mask"].to(dev)) & ~mouth_mask
            if hair_mask_iter:
                keep = keep & ~td["hair_mask"].to(dev)
            gt_white = torch.where(keep[None], gt, self.bg[:, None, None].expand_as(gt))
            if self._patch_op is None:
                self._patch_op = PatchLPIPS(self.lpips, gt.shape[-2], gt.shape[-1], *FACE_PATCH_RANGE)
            loss = loss + FACE_LPIPS_WEIGHT * self._patch_op(pkg["render"], gt_white, lpips_p, td["lips_rect"].to(dev),
                                                             self.bg)
        return loss, Ll1

    def _lpips_arg(self):
        return self._p_dev if isinstance(self._lpips_p, str) else self._lpips_p

    # ---- one step ---------------------------------------------------------------------------------------------
    def _forward_loss(self, frame: Frame, phase: FacePhase, backward_cut: bool = False):
        """render_motion and the loss block of one face step -> (pkg, loss, Ll1)."""
        from .renderer import render_motion
        # (depth and normal are read by the prior terms alone: outside that phase the forward blend is colour-only)
        pkg = render_motion(frame, self.g, self.motion_net, None, self.bg, return_attn=True, personalized=False,
                            align=phase.align, motion_reg_weight=1e-5 if phase.warm else None,
                            need_geometry=phase.priors, backward_cut=backward_cut)
        from contextlib import nullcontext
        from .losses import defer_finalize
        # (backward follows at once and the loss value is read after the step: the loss block's scalar stage rides in
        # its backward launch -- unless the prior terms are ADDED to the value here, which needs it now)
        lpips_p = self._lpips_arg()
        with (nullcontext() if (phase.priors or lpips_p is not None) else defer_finalize()):
            loss, Ll1 = self.loss_fn(frame, pkg, warm=phase.warm, hair_mask_iter=phase.hair_mask_iter,
                                     priors=phase.priors, prior_depth=phase.prior_depth, lpips_p=lpips_p)
        return pkg, loss, Ll1

    def _forward_backward(self, frame: Frame, phase: FacePhase = C3_PHASE, fold_aux: bool = False):
        pkg, loss, Ll1 = self._forward_loss(frame, phase)
        from . import diff_gauss
        # fold_aux (only callers that run _stats_and_optimizers(pkg) next): the auxiliary image's share of the screen-space
        # gradient is added by the statistics kernel instead of by a launch of its own at the end of backward
        fold = bool(fold_aux and self.on_gpu)
        diff_gauss.FOLD_AUX_M2D = fold
        try:
            backward(loss, self.device)
        except BaseException:
            diff_gauss.reset_aux_state()       # a failed backward must not withhold the NEXT step's aux share
            raise
        finally:
            diff_gauss.FOLD_AUX_M2D = False
        if fold:
            pkg["_m2d_aux"] = diff_gauss.take_folded_aux(pkg["viewspace_points"])
        return pkg, loss, Ll1

    def _forward_backward_cut(self, frame: Frame, phase: FacePhase = C3_PHASE):
        """The step's forward and the FIRST part of its backward: from the loss through the loss block, the rasterizer
        and the deform operator -- up to the tensors render_motion names as the cut (the motion fields' head outputs,
        the routed position, the attention colours).  Afterwards the gradients of every per-Gaussian parameter except
        the position (SH coefficients, opacity, scale, rotation: 20 of 24 floats per Gaussian at SH degree 1, 8 MB at
        100k) are FINAL and in ``.grad``; ``finish()`` runs the rest of the backward pass (motion fields, encoders,
        position).  A data-parallel step exchanges the first bucket while ``finish()`` computes (GraphedStep "early").
        -> (pkg, loss, Ll1, early_params, finish)"""
        from . import diff_gauss
        assert self.on_gpu
        pkg, loss, Ll1 = self._forward_loss(frame, phase, backward_cut=True)
        cut = dict.get(pkg, "_cut")
        if not cut:
            raise RuntimeError("the three-segment step needs render_motion's fused path (align=True on the GPU)")
        cut = [c for c in cut if c is not None and c.requires_grad]
        vs = pkg["viewspace_points"]
        early = [q for k, q in self.g._p.items() if k != "xyz" and q.requires_grad]
        try:
            with deferred_grads(self.device):
                got = torch.autograd.grad(loss, cut + early + [vs], grad_outputs=root_gradient(loss), allow_unused=True,
                                          retain_graph=False)
        except BaseException:
            diff_gauss.reset_aux_state()
            raise
        g_cut, g_early, g_vs = got[:len(cut)], got[len(cut):len(cut) + len(early)], got[-1]
        have = []
        for q, gq in zip(early, g_early):
            if gq is not None:
                q.grad = gq
                have.append(q)
        # (the aux image's share of the screen-space gradient was put into vs.grad by the block's exit)
        if g_vs is not None:
            vs.grad = g_vs if vs.grad is None else vs.grad.add_(g_vs)
        roots = [(c, gc) for c, gc in zip(cut, g_cut) if gc is not None]

        def finish():
            with deferred_grads(self.device):
                torch.autograd.backward([c for c, _ in roots], [gc for _, gc in roots])

        return pkg, loss, Ll1, have, finish

    @torch.no_grad()
    def sync_densification_stats(self):
        """Several ranks: every replica gets the statistics of all ranks' frames (sum of the gradient norms and
        visibility counts, maximum of the screen radii) before a densification decides on them."""
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        g = self.g
        both = torch.cat([g.xyz_gradient_accum.reshape(-1), g.denom.reshape(-1)])
        dist.all_reduce(both, op=dist.ReduceOp.SUM)
        n = g.xyz_gradient_accum.numel()
        g.xyz_gradient_accum.copy_(both[:n].view_as(g.xyz_gradient_accum))
        g.denom.copy_(both[n:].view_as(g.denom))
        dist.all_reduce(g.max_radii2D, op=dist.ReduceOp.MAX)

    @torch.no_grad()
    def _stats_and_optimizers(self, pkg, distributed: bool, it: Optional[int] = None, frame: Optional[Frame] = None):
        """Everything of an iteration behind loss.backward(), in the reference's order (train_face.py:667-788):
        statistics -> [gradient exchange] -> [densify / prune / opacity reset] -> optimizers."""
        update_densification_stats(self.g, pkg["viewspace_points"].grad, pkg["radii"], dict.get(pkg, "_m2d_aux"))
        if distributed:
            allreduce_gradients(self._all_params())
        if it is not None:
            self._maybe_densify(it, frame)
        self.optimizers.step()

    def _zero_grad(self):
        self.optimizers.zero_grad()

    def _densify_due(self, it):
        o = self.opt
        if not self.densify:
            return False
        densify = it < o.densify_until_iter and it > o.densify_from_iter and it % o.densification_interval == 0
        reset = it < o.densify_until_iter and it % o.opacity_reset_interval == 0
        prune = self.schedule == "reference" and it > o.densify_from_iter and it % o.densification_interval == 0
        return densify or reset or prune

    @torch.no_grad()
    def _maybe_densify(self, it, frame: Optional[Frame] = None):
        """Adaptive density control of the face branch (train_face.py:667-746).  Runs BEFORE the optimizers, as in
        the reference: the rebuilt Gaussian parameters carry no gradient, so only the motion network steps in such an
        iteration.  Any change of the parameter set drops a captured graph."""
        if not self._densify_due(it):
            return False
        import time
        t0 = time.perf_counter()
        o = self.opt
        interval_hit = it > o.densify_from_iter and it % o.densification_interval == 0
        if it < o.densify_until_iter:
            if interval_hit:
                self.sync_densification_stats()
                densify_and_prune_at(self.g, it, o.densify_until_iter, o, self.extent, self.gen)
            if it % o.opacity_reset_interval == 0:
                self.g.reset_opacity()
        if self.schedule == "reference" and interval_hit:
            # train_face.py:729-746: Gaussians that took the background's green, and the ones behind z = -0.07
            green = green_mask(self.g, frame.camera_center.to(self.device), FACE_GREEN)
            # (two prunes in the reference; both tests are per Gaussian, so one rebuild with the union removes the same rows)
            self.g.prune_points(green | (self.g.get_xyz[:, -1] < -0.07))
        self._drop_graph(keep_mode=True)          # (graph mode stays on: the next iteration captures its step again)
        self.density_seconds += time.perf_counter() - t0
        return True

    def _drop_graph(self, keep_mode: bool = False):
        """Forget every captured step (the parameter set changed, or the caller wants eager launches).  ``keep_mode``:
        graph mode stays on -- step() captures again when it next needs a step of some phase."""
        graphs.drop_plan(self._graph, *self._graph_cache.values())
        self._graph = None
        self._graph_cache = {}
        if not keep_mode:
            self._graph_mode = None

    def _recapture(self, frame: Frame, phase: FacePhase, min_capacity: int = 0, lpips: bool = False):
        """Capture the step of ``phase`` again WITHOUT running a single train step: graph mode is on (enable_graph was
        called once, its warm-up steps warmed every library and measured the instance counts) and only the parameter
        set (densify / prune / opacity reset) or the needed capacity changed since.  The capacity follows the Gaussian
        count; the training state and the iteration counter are untouched, so the decision to capture may be taken by
        every rank of a data-parallel run independently of what the others replay."""
        import time
        t0 = time.perf_counter()
        mode = self._graph_mode
        n = max(1, self.g.num_points)
        cap = max(int(mode["capacity"] * max(1.0, n / mode["capacity_n"])), int(min_capacity))
        g = GraphedStep(self, frame, mode["headroom"], 0, mode["split"], phase, min_capacity=cap, lpips=lpips)
        mode["capacity"], mode["capacity_n"] = g.capacity, n
        self._graph_cache[(phase, True) if lpips else phase] = g
        self.recaptures += 1
        self.recapture_seconds += time.perf_counter() - t0
        return g

    def _overflow_decision(self, graph) -> int:
        """Every CHECK_EVERY replays: did any step since the last look need more instances than the captured capacity?
        One synchronising read of the sticky device flags, made COLLECTIVE with several ranks (all-reduce MAX of flag
        and peak), so that every rank takes the same decision in the same step and captures with the same capacity.
        -> 0, or the peak need."""
        over = graph.plan.overflowed()
        peak = max([v for _, v in over], default=0)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = torch.tensor([peak], dtype=torch.int64, device=self.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            peak = int(t.item())
        return peak

    def step(self, frame: Frame):
        self.iteration += 1
        it = self.iteration
        lp = self.lpips_on(it)
        patch = None
        if lp:
            from .lpips import draw_face_patch
            patch = draw_face_patch(self.rng)
            if self._graph_mode is not None:
                self._stage_p(patch)                # (travels with the learning rates; one graph serves every size)
        self._lpips_p = patch
        self._set_learning_rates(it)
        distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        phase = self.phase_of(it)
        mode = self._graph_mode
        g = None
        if self._densify_due(it):
            # the parameter set is about to change: every captured step is stale.  This iteration runs eagerly (density
            # control sits between backward and the optimizers); the next one captures again
            self._drop_graph(keep_mode=True)
        elif mode is not None:
            # one captured step per phase (FacePhase): the schedule alternates between a few of them (the hair
            # iterations toggle six times out of seven)
            g = self._graph_cache.get((phase, True) if lp else phase)      # (the phase key gains the LPIPS flag)
            if g is None and mode["auto"]:
                g = self._recapture(frame, phase, lpips=lp)
            if g is None:
                graphs.drop_plan(self._graph)          # a phase nobody captured (auto off): eager launches
            self._graph = g
        if g is not None:
            g.replay(frame)
            loss, Ll1 = g.loss, g.l1
            if g.check_due():
                peak = self._overflow_decision(g)
                if peak:
                    # some replayed step needed more instances than the captured capacity (its image was truncated to
                    # the nearest Gaussians, gradients of the dropped ones zero): capture again, sized from the peak
                    # need -- lazily, phase by phase, without consuming iterations (_recapture)
                    mode["capacity"] = max(mode["capacity"], int(1.4 * peak) + 4096)
                    mode["auto"] = True
                    self._drop_graph(keep_mode=True)
        else:
            graphs.begin_eager_step()
            pkg, loss, Ll1 = self._forward_backward(frame, phase, fold_aux=True)
            self._stats_and_optimizers(pkg, distributed, it, frame)
            self._zero_grad()
        self.last = dict(loss=loss.detach(), l1=Ll1.detach(), num_points=self.g.num_points, phase=phase)
        if self.lpips is not None:
            self.last["patch"] = patch
        return self.last

    # ---- state snapshot (benchmark windows start from the same state; in place, so captured graphs stay valid) ----
    def _stats(self):
        return self.g.xyz_gradient_accum, self.g.denom, self.g.max_radii2D

    def snapshot(self):
        snap = dict(iteration=self.iteration,
                    **snapshot_state([p.data for p in self._all_params()], self.optimizers, self._stats()))
        if self.lpips is not None:
            snap["rng"] = self.rng.getstate()
        return snap

    def restore(self, snap):
        """Copy a snapshot() back IN PLACE (restore_state); no densification in between."""
        restore_state(snap, [p.data for p in self._all_params()], self.optimizers, self._stats())
        self.iteration = snap["iteration"]
        if "rng" in snap:
            self.rng.setstate(snap["rng"])

    # ---- graph mode --------------------------------------------------------------------------------------------
    def enable_graph(self, example_frame: Frame, headroom: float = 1.4, warmup_steps: int = 3,
                     split_for_allreduce: Optional[bool] = None, phase: Optional[FacePhase] = None,
                     min_capacity: int = 0, auto_recapture: bool = True, keep_state: bool = False):
        """Capture the whole step into a hipGraph and switch graph mode on.  Runs `warmup_steps` eager steps plus two
        capacity-mode steps first to measure the instance counts and warm every library: real train steps that advance
        the iteration counter -- unless ``keep_state``, which restores parameters, optimizer state, statistics and the
        counter afterwards.  The graph holds the launches of one phase (FacePhase): `phase`, or the phase of the
        iteration right after the capture.  Captured steps are kept per phase; every one of them is dropped when the
        parameter set changes (densify / prune / opacity reset) or a replay overflowed the instance capacity.  With
        ``auto_recapture`` step() then captures the step it needs again by itself, without warm-up steps and without
        touching the training state (_recapture); without it such a step launches eagerly."""
        self._graph = None
        after = self.iteration + (0 if keep_state else max(1, warmup_steps) + 2) + 1
        lp = self.lpips_on(after)
        if phase is None:
            phase = self.phase_of(after)                                       # the iteration right after capture
        snap = self.snapshot() if keep_state else None
        if self.densify and self.on_gpu:
            warm_density_control(self.device, self.g.max_sh_degree, self.opt)
        self._graph = GraphedStep(self, example_frame, headroom, max(1, warmup_steps), split_for_allreduce, phase,
                                  min_capacity=min_capacity, restore=snap, lpips=lp)
        self._graph_cache[(phase, True) if lp else phase] = self._graph
        prev = self._graph_mode
        self._graph_mode = dict(headroom=headroom, split=self._graph.split, auto=bool(auto_recapture),
                                capacity=max(self._graph.capacity, prev["capacity"] if prev else 0),
                                capacity_n=max(1, self.g.num_points))
        return self._graph


class GraphedStep(graphs.CapturedStep):
    def __init__(self, trainer: FaceTrainer, example: Frame, headroom: float, warmup_steps: int,
                 split_for_allreduce: Optional[bool] = None, phase: FacePhase = C3_PHASE, min_capacity: int = 0,
                 restore=None, lpips: bool = False):
        """``warmup_steps`` > 0: the cold path (eager steps measure the instance count and warm every library; with
        ``restore`` = a trainer.snapshot() the training state is put back afterwards).  0: the warm path of
        FaceTrainer._recapture -- nothing runs, ``min_capacity`` is the capacity."""
        # (``lpips``: the step carries the late phase's LPIPS term and reads its patch size from the trainer's device
        # scalar; the trainer's field says so while the step is measured, warmed and captured, and is put back afterwards)
        prev, trainer._lpips_p = trainer._lpips_p, ("device" if lpips else None)
        try:
            self._build(trainer, example, headroom, warmup_steps, split_for_allreduce, phase, min_capacity, restore, lpips)
        finally:
            trainer._lpips_p = prev

    def _build(self, trainer, example, headroom, warmup_steps, split_for_allreduce, phase, min_capacity, restore, lpips):
        self.phase = phase
        t = self.trainer = trainer
        dev = t.device
        assert dev.type == "cuda", "graph mode needs the GPU"
        self.distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        # two graphs with the (eager) gradient all-reduce between them; can be forced for single-rank tests.
        # "early": THREE graphs -- A' (forward, backward down to the motion fields' outputs), A'' (the motion fields'
        # backward), B (scale, hand back, statistics, optimizers): the bucket of the per-Gaussian gradients that are
        # final after A' (8 of the 10 MB at 100k Gaussians) is exchanged WHILE A'' runs, the small second bucket
        # (positions + networks) behind it.  It is the form several ranks use.
        if split_for_allreduce is None:
            split_for_allreduce = "early" if self.distributed else False
        # (the cut runs through the fused deform operator, which needs the alignment on: a phase without it -- the same
        # on every rank -- takes the two-graph form)
        self.early = split_for_allreduce == "early" and bool(phase.align)
        self.split = bool(split_for_allreduce)
        self.static = example.clone_static()
        cold = warmup_steps > 0

        def pre():
            t.iteration += 1
            if lpips:
                from .lpips import draw_face_patch
                t._stage_p(draw_face_patch(t.rng))
            t._set_learning_rates(t.iteration)

        def eager_step():
            pkg = t._forward_backward(self.static, phase, fold_aux=True)[0]
            t._stats_and_optimizers(pkg, self.distributed)
            t._zero_grad()

        if cold:
            cap = graphs.face_capacity(graphs.measure(eager_step, warmup_steps, pre), headroom, min_capacity)
        else:
            assert min_capacity > 0, "a warm capture needs the capacity of an earlier one"
            cap = int(min_capacity)
            t.optimizers.prepare()           # tables of the new parameter set: allocations / uploads outside the capture
            from . import renderer
            renderer.prepare_screenspace(t.g)      # (likewise the zeros behind the screen-space gradient carrier)
        self.plan = graphs.install([cap, cap], dev)
        if cold:
            graphs.warm(self.plan, eager_step, dev, pre)
            if restore is not None:
                t.restore(restore)
                t._set_learning_rates(max(1, t.iteration))
        # With several ranks the gradient exchange stays outside the graphs:
        #    graph A = forward + backward (+ bucket fill), eager all-reduce, graph B = statistics + optimizers.
        # other threads (the collective library's watchdog) may touch the HIP runtime while this thread captures
        options = {"capture_error_mode": "thread_local"} if self.distributed else {}
        if t._pool is None:
            t._pool = _lib.GraphPool(dev)
        options["pool"] = t._pool.handle
        options["light"] = not cold
        self.graph_a = torch.cuda.CUDAGraph()
        self.graph_b = None
        dot = os.environ.get("INSTAG_GRAPH_DOT")       # diagnostics: the captured step's nodes and edges (DOT)
        if dot:
            self.graph_a.enable_debug_mode()
        self.graph_a2 = None
        if not self.split:
            with graphs.capture(self.graph_a, self.plan, cold, **options):
                pkg, loss, l1 = t._forward_backward(self.static, phase, fold_aux=True)
                t._stats_and_optimizers(pkg, False)
                t._zero_grad()
            del pkg
        elif self.early:
            with graphs.capture(self.graph_a, self.plan, cold, **options):
                pkg, loss, l1, early, finish = t._forward_backward_cut(self.static, phase)
                self._vs_grad, self._radii = pkg["viewspace_points"].grad, pkg["radii"]
                self._params_early = early
                self._bucket_early = flat_grad_bucket(early)
            self.graph_a2 = torch.cuda.CUDAGraph()
            with graphs.capture(self.graph_a2, self.plan, False, **options):
                finish()
                ids = {id(q) for q in early}
                self._params = [q for q in with_grad(t._all_params()) if id(q) not in ids]
                self._bucket = flat_grad_bucket(self._params)
            del pkg, finish
            self.graph_b = torch.cuda.CUDAGraph()
            with graphs.capture(self.graph_b, self.plan, False, **options):
                with torch.no_grad():
                    if self.distributed:
                        self._bucket_early.mul_(1.0 / dist.get_world_size())
                        self._bucket.mul_(1.0 / dist.get_world_size())
                    scatter_grad_bucket(self._params_early, self._bucket_early)
                    scatter_grad_bucket(self._params, self._bucket)
                    update_densification_stats(t.g, self._vs_grad, self._radii)
                    t.optimizers.step()
                    t._zero_grad()
        else:
            with graphs.capture(self.graph_a, self.plan, cold, **options):
                pkg, loss, l1 = t._forward_backward(self.static, phase)
                self._vs_grad, self._radii = pkg["viewspace_points"].grad, pkg["radii"]
                self._params = with_grad(t._all_params())
                self._bucket = flat_grad_bucket(self._params)
            del pkg
            self.graph_b = torch.cuda.CUDAGraph()
            with graphs.capture(self.graph_b, self.plan, False, **options):
                with torch.no_grad():
                    if self.distributed:
                        # mean over ranks of the summed gradients
                        self._bucket.mul_(1.0 / dist.get_world_size())
                    scatter_grad_bucket(self._params, self._bucket)
                    update_densification_stats(t.g, self._vs_grad, self._radii)    # local until a densification
                    t.optimizers.step()
                    t._zero_grad()
        if dot:
            self.graph_a.debug_dump(dot)
        self.loss, self.l1 = loss.detach(), l1.detach()          # (detached, released after the capture: graphs.py)
        self.capacity = cap

    def replay(self, frame: Frame):
        self._replays += 1
        self.static.copy_from(frame)
        self.graph_a.replay()
        if self.graph_a2 is not None:
            # the first bucket travels while the motion fields' backward runs (the collective library works on its own
            # stream, ordered behind graph A' by the stream it was issued from); graph B waits for both exchanges
            work = dist.all_reduce(self._bucket_early, op=dist.ReduceOp.SUM, async_op=True) if self.distributed else None
            self.graph_a2.replay()
            if self.distributed:
                work2 = dist.all_reduce(self._bucket, op=dist.ReduceOp.SUM, async_op=True)
                work.wait()
                work2.wait()
            self.graph_b.replay()
            return
        if self.graph_b is not None:
            if self.distributed:
                dist.all_reduce(self._bucket, op=dist.ReduceOp.SUM)       # the division by the world size is in graph B
            self.graph_b.replay()


def build_trainer(n_gaussians, device, sh_degree=1, seed=0, densify=False, encoder_cls=None, raw=None, schedule=None,
                  audio_extractor="deepspeech"):
    """Synthetic config-C3 trainer: N Gaussians + PMF + UMF with random-init weights."""
    from .motion_net import MotionNetwork, PersonalizedMotionNetwork
    from .scene_synth import synthetic_gaussians
    torch.manual_seed(seed)
    args = SimpleNamespace(audio_extractor=audio_extractor, type="face")
    pmf = PersonalizedMotionNetwork(args=args, encoder_cls=encoder_cls).to(device)
    umf = MotionNetwork(args=args, encoder_cls=encoder_cls).to(device)
    g = GaussianModel(sh_degree, neural_motion_grid=pmf)
    g.load_raw(raw if raw is not None else synthetic_gaussians(n_gaussians, sh_degree=sh_degree, seed=seed), device)
    bg = torch.tensor([0.0, 1.0, 0.0], device=device)
    return FaceTrainer(g, umf, bg, densify=densify, seed=seed, schedule=schedule)
