"""How good a trained head is, measured on the device, and the frames the reference writes out.

The reference scores its result twice: train_face.py:821-878 reports L1 and utils/image_utils.py ``psnr`` on held-out
cameras at the test iterations (``face_validation``), and metrics.py:105-217 reports PSNR and LPIPS between the 8-bit
frames of the rendered and the ground-truth videos (``Evaluator`` with ``quantize=True``); LMD, metrics.py:8-102, is the
mean distance between the mouth landmarks of the two frames, each set taken off its own mean (``landmarks.lmd_torch``),
and joins the report when the Evaluator is given a ``landmarks.LandmarkNet`` and either one face box per frame or a
``face_detect.FaceDetector``, the face detector the reference's meter runs in front of the landmark network on the
rendered and on the ground-truth frame.  synthesize_fuse.py:65-76 dilates the mouth alpha and writes ``uint8 [H,W,3]``
frames (``infer_compose``, reached through ``infer.FuseRenderer(dilate=, as_uint8=)``).

    r = FuseRenderer(g, net, gm, netm, bg).enable_graph(frames[0], frames_per_replay=4)
    print(Evaluator(r, lpips=FrameLPIPS(weights, H, W)).evaluate(frames, gts, scene_backgrounds))

On the GPU ``frame_metrics`` and ``infer_compose`` are csrc/metrics.hip; the ``*_torch`` functions are the plain-torch
statement of the same figures (any dtype, CPU or GPU) that the tests compare against and the CPU path uses.  The sums
of a whole evaluation stay on the device (``Meter``); ``Meter.report`` is the only place that synchronises.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import losses
from . import lpips as LP

COLUMNS = ("l1", "mse", "psnr", "psnr_rgb", "ssim")
FLAG_CLAMP, FLAG_QUANTIZE = 1, 2
MAX_DILATE = 31
MAX_LPIPS_FRAME = 1024                 # csrc/lpips.hip make_plan: square patches up to 1024 pixels


# ---- plain-torch statement -------------------------------------------------------------------------------------------
def quantize_frame(x):
    """What an 8-bit video frame keeps of ``x``: synthesize_fuse.py:76 ``(x.clamp(0,1) * 255).astype(uint8)`` (a
    truncation) read back as metrics.py:205-206 does, ``frame / 255.0`` as a FloatTensor.  fp32 in, fp32 out."""
    return (x.float().clamp(0, 1) * 255).to(torch.uint8).float() / 255.0


def frame_metrics_torch(pred, gt, clamp=True, quantize=False, dtype=None):
    """[B,3,H,W] x 2 -> per_frame [B,5] = (l1, mse, psnr, psnr_rgb, ssim), see ``frame_metrics``.  ``dtype``: the
    arithmetic's (default: the input's); quantisation is always done in fp32, as a frame is written, before the cast."""
    dtype = dtype or pred.dtype
    if quantize:
        pred, gt = quantize_frame(pred), quantize_frame(gt)
    elif clamp:
        pred = pred.clamp(0, 1)
    pred, gt = pred.to(dtype), gt.to(dtype)
    rows = []
    for p, g in zip(pred, gt):
        mse = ((p - g) ** 2).mean()
        rows.append(torch.stack([losses.l1_loss(p, g), mse, -10 * torch.log10(mse),      # metrics.py:127
                                 losses.psnr(p, g).mean(), losses.ssim(p, g)]))
    return torch.stack(rows)


def infer_compose_torch(face, a_face, mouth, a_mouth, bg, scene=None, dilate=1):
    """synthesize_fuse.py:65-76 for renders over ``bg``: -> (image [3,H,W] clamped to [0,1], frame uint8 [H,W,3])."""
    a_d = a_mouth if dilate == 1 else F.max_pool2d(a_mouth[None], dilate, 1, dilate // 2)[0]
    bg3 = bg[:, None, None]
    if scene is None:
        scene = torch.zeros_like(face)
    mouth_image = mouth - bg3 * (1.0 - a_mouth) + scene * (1.0 - a_d)
    image = (face - bg3 * (1.0 - a_face) + mouth_image * (1.0 - a_face)).clamp(0, 1)
    return image, (image.permute(1, 2, 0) * 255).to(torch.uint8)


# ---- device state ----------------------------------------------------------------------------------------------------
class Meter:
    """Running sums of an evaluation on ``device``: double[6] = the five frame figures and the frame count (what
    ``instag_frame_metrics`` adds to), then the LPIPS sum and its count, then the LMD sum and its count (its mean joins
    the report only where an evaluation measured it).  Means are means of per-frame values, as the
    reference's meters keep them (metrics.py:123-133: the mean of per-frame PSNR, not the PSNR of the mean MSE)."""

    def __init__(self, device="cpu"):
        self.state = torch.zeros(10, dtype=torch.float64, device=device)
        self.lmd_skipped = None                         # a host count, kept only by an evaluation that detects faces

    def clear(self):
        self.state.zero_()
        self.lmd_skipped = None

    def add_rows(self, per_frame):
        """CPU path of ``frame_metrics``: rows [n,5] into the sums."""
        self.state[:5] += per_frame.double().sum(0)
        self.state[5] += per_frame.shape[0]

    def add_lpips(self, values, slot: int = 6):
        """``values`` [n] fp32 into the LPIPS slot (one launch on the device, no synchronisation)."""
        n = int(values.shape[0])
        if n == 0:
            return
        if not self.state.is_cuda:
            self.state[slot] += values.double().sum()
            self.state[slot + 1] += n
            return
        from . import _lib
        values = values.contiguous().float()
        _lib.check(_lib.lib().instag_meter_add(_lib.ptr(values), n, _lib.ptr(self.state[slot:]), _lib.current_stream()),
                   "meter_add")

    def add_lmd(self, values):
        """``values`` [n] fp32 into the LMD slot, as ``add_lpips``."""
        self.add_lpips(values, slot=8)

    def report(self) -> dict:
        """Synchronises.  -> means over the frames seen; ``lpips`` is None when nothing was added to its slot."""
        s = self.state.cpu().tolist()
        n = s[5]
        out = {k: (s[i] / n if n else float("nan")) for i, k in enumerate(COLUMNS)}
        out["lpips"] = s[6] / s[7] if s[7] else None
        if s[9]:
            out["lmd"] = s[8] / s[9]                    # only where an evaluation measured it
        if self.lmd_skipped is not None:
            out["lmd_skipped"] = int(self.lmd_skipped)   # frames a face detector found no face in (Evaluator)
        out["frames"] = int(n)
        return out


# ---- operators -------------------------------------------------------------------------------------------------------
@torch.no_grad()
def frame_metrics(pred, gt, clamp=True, quantize=False, meter: Optional[Meter] = None, n_valid: Optional[int] = None):
    """Per-frame figures of ``pred`` against ``gt``, both [B,3,H,W] fp32 -> [B,5], columns ``COLUMNS``:

      l1, mse          means over the frame
      psnr             -10 log10(mse), metrics.py:127 (+inf for identical frames, as numpy gives)
      psnr_rgb         utils/image_utils.py ``psnr``: 20 log10(1 / sqrt(mse_c)) per channel, then the mean
      ssim             utils/loss_utils.py:42-72 (``losses.ssim``)

    ``clamp``: pred is clamped to [0,1] first.  ``quantize``: both are reduced to what an 8-bit frame keeps
    (``quantize_frame``), which makes the figures those of metrics.py on the written videos.  ``meter``: the first
    ``n_valid`` (default B) frames' figures are added to it -- the padded tail of a batched replay stays out.
    On the device: one tile launch and one finalize launch on the current stream, no synchronisation."""
    assert pred.dim() == 4 and pred.shape[1] == 3 and pred.shape == gt.shape, "frame_metrics: [B,3,H,W] twice"
    B, _, H, W = pred.shape
    n_valid = B if n_valid is None else int(n_valid)
    if not 0 <= n_valid <= B:
        raise ValueError(f"frame_metrics: n_valid {n_valid} outside [0, {B}]")
    if not pred.is_cuda:
        rows = frame_metrics_torch(pred.float(), gt.float(), clamp, quantize)
        if meter is not None:
            meter.add_rows(rows[:n_valid])
        return rows
    from . import _lib
    L = _lib.lib()
    pred, gt = pred.contiguous().float(), gt.contiguous().float()
    partials = torch.empty(L.instag_frame_metrics_num_partials(B, H, W), dtype=torch.float64, device=pred.device)
    per_frame = torch.empty(B, 5, dtype=torch.float32, device=pred.device)
    if meter is not None:
        assert meter.state.device == pred.device, "frame_metrics: the meter lives on another device"
    flags = (FLAG_CLAMP if clamp else 0) | (FLAG_QUANTIZE if quantize else 0)
    _lib.check(L.instag_frame_metrics(_lib.ptr(pred), _lib.ptr(gt), B, H, W, flags, _lib.ptr(partials),
                                      _lib.ptr(per_frame), None if meter is None else _lib.ptr(meter.state), n_valid,
                                      _lib.current_stream()), "frame_metrics")
    return per_frame


@torch.no_grad()
def infer_compose(face, a_face, mouth, a_mouth, bg, scene=None, dilate=1, as_uint8=False):
    """The inference epilogue (synthesize_fuse.py:65-76) of two renders over ``bg``: -> (image [3,H,W] in [0,1],
    frame uint8 [H,W,3] or None).  ``dilate`` (odd, 1 = off, at most 31; the reference's --dilate is 13): the scene
    background shows through the mouth pass where the dilate x dilate maximum of its alpha is below one.  One HIP
    launch on the device."""
    dilate = int(dilate)
    if dilate < 1 or dilate > MAX_DILATE or dilate % 2 == 0:
        raise ValueError(f"infer_compose: dilate must be odd and in 1 .. {MAX_DILATE}, got {dilate}")
    if not face.is_cuda:
        image, u8 = infer_compose_torch(face, a_face.reshape(1, *face.shape[1:]), mouth,
                                        a_mouth.reshape(1, *face.shape[1:]), bg, scene, dilate)
        return image, (u8 if as_uint8 else None)
    from . import _lib
    _, H, W = face.shape
    assert mouth.shape == face.shape and a_face.numel() == H * W and a_mouth.numel() == H * W
    assert scene is None or scene.shape == face.shape
    face, a_face, mouth, a_mouth, bg = (t.contiguous().float() for t in (face, a_face, mouth, a_mouth, bg))
    scene = None if scene is None else scene.contiguous().float()
    image = torch.empty_like(face)
    u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=face.device) if as_uint8 else None
    _lib.check(_lib.lib().instag_infer_compose(_lib.ptr(face), _lib.ptr(a_face), _lib.ptr(mouth), _lib.ptr(a_mouth),
                                               _lib.ptr(bg), _lib.ptr(scene), dilate, _lib.ptr(image), _lib.ptr(u8),
                                               H, W, _lib.current_stream()), "infer_compose")
    return image, u8


class FrameLPIPS:
    """LPIPS of whole frames, called as metrics.py:164-165 calls the package: ``lpips(truth, pred, normalize=True)``,
    inputs in [0,1] mapped to [-1,1].  ``(pred, gt, meter=None, n_valid=None) -> [B]`` for [B,3,H,W] batches.

    On the device a frame is ONE patch of the patch operator (csrc/lpips.hip), which takes square patches of
    31 .. 1024 pixels: any other shape raises ValueError -- there is no fallback on the device.  Forward only: the
    operator is driven without autograd, so nothing is recorded for a backward; its workspace holds the layers'
    activations either way, because each layer of the forward reads the one before from it.  On the CPU the call is
    ``lpips_torch``."""

    def __init__(self, weights: LP.LPIPSWeights, H: int, W: int):
        self.w, self.H, self.W = weights, int(H), int(W)
        self._plans = {}

    def _plan(self, device):
        if self.H != self.W or not LP.MIN_PATCH <= self.H <= MAX_LPIPS_FRAME:
            raise ValueError(f"FrameLPIPS: the HIP operator takes square frames of {LP.MIN_PATCH} .. {MAX_LPIPS_FRAME} "
                             f"pixels, got {self.H}x{self.W}")
        key = (device.type, device.index)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = LP._Plan(self.w, device, self.H, self.W, self.H, self.H)
            plan.p_dev.fill_(self.H)
        return plan

    @torch.no_grad()
    def __call__(self, pred, gt, meter: Optional[Meter] = None, n_valid: Optional[int] = None):
        if pred.dim() == 3:
            pred, gt = pred[None], gt[None]
        assert tuple(pred.shape[1:]) == (3, self.H, self.W) and pred.shape == gt.shape, \
            f"FrameLPIPS was built for [B,3,{self.H},{self.W}] frames"
        if not pred.is_cuda:
            values = LP.lpips_torch(gt * 2 - 1, pred * 2 - 1, self.w).reshape(-1)
        else:
            plan = self._plan(pred.device)
            pred, gt = pred.contiguous().float(), gt.contiguous().float()
            values = torch.cat([plan.forward(g, p, plan.p_dev, self.H, None, None, False)[0][:1]
                                for p, g in zip(pred, gt)])
        if meter is not None:
            meter.add_lpips(values[:values.shape[0] if n_valid is None else int(n_valid)])
        return values


# ---- whole evaluations -----------------------------------------------------------------------------------------------
class Evaluator:
    """Scores what ``renderer`` (infer.FuseRenderer) renders against ground-truth frames.  ``quantize=True``: the figures
    metrics.py prints for the two videos synthesize_fuse.py writes (PSNR, and LPIPS when ``lpips`` -- a FrameLPIPS -- is
    given), plus L1 / MSE / SSIM of the same 8-bit frames.  ``group``: frames per render and per metrics launch
    (default: the renderer's captured ``frames_per_replay``, 1 without a graph).  ``lmd``: ``(LandmarkNet, boxes [N,4] or
    [4])`` -- the report gains ``lmd``, the reference's mouth landmark distance between the 8-bit rendered and
    ground-truth frames, both cropped by the frame's box; a frame whose box has a NaN stays out of its mean.  Or
    ``(LandmarkNet, face_detect.FaceDetector)``: as in the reference's meter (metrics.py:78-79) the boxes are detected
    separately on the 8-bit rendered frame and on the ground truth, ``detector.last(...)`` being the reference's
    ``[-1]``; a frame where either has no detection is left out of the mean and counted in the report as
    ``lmd_skipped`` (the reference would raise there; reading the boxes synchronises once per group)."""

    def __init__(self, renderer, lpips: Optional[FrameLPIPS] = None, quantize: bool = True, group: Optional[int] = None,
                 lmd=None):
        self.renderer, self.lpips, self.quantize, self.group, self.lmd = renderer, lpips, bool(quantize), group, lmd

    @torch.no_grad()
    def evaluate(self, frames, gts, scene_backgrounds=None) -> dict:
        """``gts``: one [3,H,W] image in [0,1] per frame.  Renders in groups (a short last group is padded with its
        last frame, which ``n_valid`` keeps out of the sums), one ``frame_metrics`` call per group, one synchronisation
        at the end.  -> ``Meter.report()``."""
        assert len(frames) == len(gts) and (scene_backgrounds is None or len(scene_backgrounds) == len(frames))
        r = self.renderer
        K = int(self.group or getattr(r, "frames_per_replay", 1))
        meter = Meter(r.bg.device)
        if self.lmd is not None:
            from . import landmarks as LM
            net, detector = self.lmd[0], self.lmd[1] if hasattr(self.lmd[1], "last") else None
            if detector is None:
                boxes = LM.check_boxes(self.lmd[1], len(frames))
            else:
                meter.lmd_skipped = 0
        for g0 in range(0, len(frames), K):
            idx = [min(g0 + k, len(frames) - 1) for k in range(K)]
            n = min(K, len(frames) - g0)
            out = r.render_batch([frames[j] for j in idx],
                                 None if scene_backgrounds is None else [scene_backgrounds[j] for j in idx])
            images = out[0] if isinstance(out, tuple) else out
            gt = torch.stack([gts[j] for j in idx])
            frame_metrics(images, gt, clamp=True, quantize=self.quantize, meter=meter, n_valid=n)
            if self.lpips is not None:
                if self.quantize:
                    images, gt = quantize_frame(images), quantize_frame(gt)
                self.lpips(images[:n], gt[:n], meter=meter)
            if self.lmd is not None and detector is not None:
                as_u8 = lambda t: (t[:n].clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)             # metrics.py:69
                p8, g8 = as_u8(images), as_u8(gt)
                pb, gb = LM.check_boxes(detector.last(p8)), LM.check_boxes(detector.last(g8))
                keep = torch.nonzero(LM.usable(pb) & LM.usable(gb))[:, 0]
                meter.lmd_skipped += n - int(keep.shape[0])
                if keep.numel():
                    k = keep.to(p8.device)
                    meter.add_lmd(LM.lmd_torch(net.landmarks(p8[k], pb[keep]), net.landmarks(g8[k], gb[keep])))
            elif self.lmd is not None:
                keep = [k for k in range(n) if bool(LM.usable(boxes[idx[k]][None]))]
                if keep:
                    as_u8 = lambda t: (t[keep].clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)   # metrics.py:69
                    rows = boxes[[idx[k] for k in keep]]
                    meter.add_lmd(LM.lmd_torch(net.landmarks(as_u8(images), rows), net.landmarks(as_u8(gt), rows)))
        return meter.report()


@torch.no_grad()
def face_validation(gaussians, motion_net, frames, gts, bg, backgrounds=None) -> dict:
    """train_face.py:830-874 without the TensorBoard images: per held-out frame ``render_motion(align=True)``, the clamp,
    ``image - bg (1 - alpha) + background (1 - alpha)`` (:847) against the clamped ground truth; -> the means of
    ``l1_loss`` and of utils/image_utils.py ``psnr`` (the ``psnr_rgb`` column) as {"l1", "psnr"}.  ``backgrounds``: one
    [3,H,W] image in [0,1] per frame (default: the frame's own ``talking_dict["background"]``, black without one)."""
    from .renderer import render_motion
    meter = Meter(bg.device)
    for i, (frame, gt) in enumerate(zip(frames, gts)):
        pkg = render_motion(frame, gaussians, motion_net, None, bg, return_attn=True, frame_idx=0, align=True)
        image = torch.clamp(pkg["render"], 0.0, 1.0)
        alpha = pkg["alpha"]
        back = backgrounds[i] if backgrounds is not None else frame.talking_dict.get("background")
        image = image - bg[:, None, None] * (1.0 - alpha)
        if back is not None:
            image = image + back * (1.0 - alpha)
        frame_metrics(image[None], torch.clamp(gt, 0.0, 1.0)[None], clamp=False, meter=meter)
    rep = meter.report()
    return {"l1": rep["l1"], "psnr": rep["psnr_rgb"]}
