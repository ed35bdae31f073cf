"""Render composition on the MI355X operators: ``render``, ``render_motion``, ``render_motion_mouth_con``, ``render_fuse``.

Counterpart of the reference's gaussian_renderer/__init__.py: render :37-133, render_motion :151-298,
render_motion_mouth_con :302-435 (same argument meaning and returned dictionary keys).  ``viewpoint_camera`` needs the
attributes the reference reads: FoVx, FoVy, image_height, image_width, world_view_transform, full_proj_transform,
camera_center, and ``talking_dict`` with ``auds`` [8,29,16] and ``au_exp`` [6] for render_motion.

Both motion renders are one sequence of stages: evaluate the fields (_evaluate_fields) ->
choose and run one deformation path (-> _Deformed) -> publish the reference's in-place updates (_publish, called by
the path) -> rasterize, with the attention passes (_render_passes) -> package.
"""
from __future__ import annotations

import math
import os as _os
from typing import NamedTuple

import torch

from . import _keepalive
from .diff_gauss import GaussianRasterizationSettings, GaussianRasterizer
from .motion_net import LazyOutputs, MotionNetwork as _MotionNetwork

# Fuse stage (training): the mouth pass on a second stream beside the face pass (1.45 -> 1.26 ms per captured step in
# round 2).  Round 2 shipped it switched off behind a segmentation fault inside hipGraphLaunch of a LATER, unrelated
# face-step graph that only a soak of the stage tests showed.  Round 3 removed the two ownership defects the bisect
# pointed at: side streams drawn from torch's round-robin pool could be the SAME HIP stream
# under two names once a process had asked for more than 32 (the "fuse" stream is created late, so it was the one that
# could alias an operator's lane or a capture's warm-up stream: _lib.side_stream now guarantees distinct handles), and
# captured steps kept their loss -- hence their autograd graph and every parameter's gradient accumulator -- alive, bound
# to a per-capture stream that later backward passes then hopped to inside an open capture (one capture stream, detached
# outputs).  The GPU suite passes with the switch on; INSTAG_CONCURRENT_FUSE=0 switches it off.
CONCURRENT_FUSE_PASSES = _os.environ.get("INSTAG_CONCURRENT_FUSE", "1") == "1"


def _side_stream(device, tag="attn"):
    """Second HIP stream per device and purpose (from _lib.side_stream's registry) for work forked beside the main pass
    (an attention raster pass, the fuse stage's mouth pass): a pass alone leaves most CUs idle, bound by its longest tile."""
    from . import _lib
    return _lib.side_stream(device, ("renderer", tag))


def _settings(cam, pc, bg_color, scaling_modifier, debug=False):
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width),
        tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
        sh_degree=pc.active_sh_degree, campos=cam.camera_center, prefiltered=False, debug=debug)


# ---- constants -------------------------------------------------------------------------------------------------------
_CONSTANTS = {}          # kind -> {(device, shape, dtype): tensor}
_CARRIER_COUNTS = 8      # gradient-carrier buffers kept (Gaussian counts of past density-control events are dropped)


def _constant(kind, like, make, keep=None):
    """Read-only ``make(like)`` (torch.zeros_like / torch.ones_like), created once per kind, device, shape and dtype.
    While the current stream is capturing, a constant that is not there yet is returned fresh and NOT kept: it could
    only come from the capture's pool and would be replayed as a fill.  ``keep``: the most entries of THIS kind; one more
    drops them (the other kinds' are not touched)."""
    kept = _CONSTANTS.setdefault(kind, {})
    key = (like.device, tuple(like.shape), like.dtype)
    t = kept.get(key)
    if t is None:
        t = make(like)
        if not (like.is_cuda and torch.cuda.is_current_stream_capturing()):
            if keep is not None and len(kept) >= keep:
                kept.clear()
            kept[key] = t
    return t


def prepare_screenspace(pc):
    """Allocate the zeros behind the screen-space gradient carrier for this Gaussian count now (a trainer calls it in
    front of a stream capture, where a first use would fall under _constant's capture rule)."""
    return _constant("carrier", pc.get_xyz, torch.zeros_like, keep=_CARRIER_COUNTS)


def _gradient_carrier(pc):
    # gradient carrier of the screen-space means (gaussian_renderer/__init__.py:47-52 builds it as zeros + 0 with
    # retain_grad(); a leaf receives the same .grad and saves a launch).  Nothing reads or writes its VALUE -- the
    # rasterizer takes it for the gradient's sake only -- so every step's leaf is a fresh view of one zeroed buffer per
    # Gaussian count instead of a fill launch at the head of the step (4 us + a launch gap on the chain)
    return prepare_screenspace(pc).detach().requires_grad_(True)


def _neutral_expression(cam, dev):
    """Read-only zeros of the frame's ``au_exp``: the neutral expression the mouth branch feeds the face field."""
    return _constant("neutral", cam.talking_dict["au_exp"].to(dev, non_blocking=True), torch.zeros_like)


def _begin(cam, pc, pipe, bg_color, scaling_modifier):          # -> (gradient carrier, rasterizer) of one render
    debug = getattr(pipe, "debug", False)
    return _gradient_carrier(pc), GaussianRasterizer(_settings(cam, pc, bg_color, scaling_modifier, debug))


def render(viewpoint_camera, pc, pipe=None, bg_color=None, scaling_modifier=1.0, override_color=None):
    """Static render (no motion fields)."""
    screenspace_points, rasterizer = _begin(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    opacity = pc.get_opacity
    shs, colors = (pc.get_features, None) if override_color is None else (None, override_color)
    image, depth, normal, alpha, radii, extra = rasterizer(
        means3D=pc.get_xyz, means2D=screenspace_points, shs=shs, colors_precomp=colors, opacities=opacity,
        scales=pc.get_scaling, rotations=pc.get_rotation, cov3Ds_precomp=None, extra_attrs=torch.ones_like(opacity))
    return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
            "depth": depth, "alpha": alpha, "normal": normal, "radii": radii}


# ---- stage 1: the fields ---------------------------------------------------------------------------------------------
class _Fields(NamedTuple):
    motion: dict             # the universal field's predictions
    p_motion: object         # the personalised field's, None when neither personalized nor align
    xyz_route: object        # the positions as the last encode handed them on (gridencoder.passthrough)
    p_route: object          # likewise the fused shift's operand, None without one


def _evaluate_fields(cam, pc, motion_net, personalized, align, condition, *, announce, fused_shift, p_exp=None,
                     flush_on_shift_grad=False):
    """Frame inputs, the personalised and the universal field -> _Fields.  What the two renders do differently is a
    parameter: ``condition`` = the universal field's third argument, or a callable(audio_feat) that makes it right before
    that call; ``announce(audio_feat)`` = the render's start_audio calls (device only); ``fused_shift(p_preds)`` = the raw
    alignment head if the universal field can add it to the positions inside its tri-plane kernel, else None (device
    only); ``p_exp`` = the expression the personalised field takes as well, None for none; ``flush_on_shift_grad``."""
    from . import gridencoder as _ge
    xyz = xyz_route = pc.get_xyz
    dev = xyz.device
    audio_feat = cam.talking_dict["auds"].to(dev, non_blocking=True)
    if xyz.is_cuda:
        announce(audio_feat)
    # The Gaussians' positions feed three operators (personalised field, universal field, deformation): on the device
    # each encode hands the position on as one of its outputs, so the three gradients are summed inside the encoders'
    # backward kernels instead of by autograd add launches on the tail of the step (gridencoder.passthrough)
    carrier, p_preds, x_shift = {}, None, None
    if personalized or align:
        with _ge.passthrough(carrier):
            p_preds = pc.neural_motion_grid(pc.get_xyz, audio_feat, *(() if p_exp is None else (p_exp,)))
        xyz = xyz_route = carrier.pop("xyz", xyz_route)
    if align:
        p_raw = fused_shift(p_preds) if xyz.is_cuda else None
        if p_raw is not None:
            x_shift = (p_raw, 1e-2)           # xyz + p_xyz (= p[:, :3] * 1e-2) is formed inside the tri-plane kernel
            if flush_on_shift_grad and p_raw.requires_grad:
                # backward reaches p when the universal field is done and the personalised field's chain is about to
                # start: the weight gradients queued so far can run beside it (instag_amd/deferred.py)
                from . import deferred
                p_raw.register_hook(lambda g, dev=dev: deferred.flush_async(dev))
        else:
            xyz = xyz + p_preds["p_xyz"]
    cond = condition(audio_feat) if callable(condition) else condition
    with _ge.passthrough(carrier):
        preds = motion_net(xyz, audio_feat, cond, **({} if x_shift is None else {"x_shift": x_shift}))
    if x_shift is not None or not align:
        xyz_route = carrier.pop("xyz", xyz_route)     # (align without the fused shift encodes xyz + p_xyz, not xyz)
    return _Fields(preds, p_preds, xyz_route, carrier.pop("shift", None))


# ---- stages 2 and 3: one deformation path, which publishes what the reference updates in place -------------------------
class _Deformed(NamedTuple):
    means3D: object
    scales: object
    rotations: object
    opacity: object
    motion_reg: object = None     # partial sums of the step's regularisers, when the path's operator computes them
    cut: object = None            # outputs of the _BackwardCut node (fused face path with backward_cut=True)


class _BackwardCut(torch.autograd.Function):
    """Identity on a set of tensors, as ONE autograd node: the place where FaceTrainer's three-segment data-parallel
    step cuts the backward pass.  ``torch.autograd.grad(loss, cut_outputs)`` stops AT this node -- it runs the loss
    block, the rasterizer and the deform operator and nothing of the motion fields (without the node the capture
    points would sit on the encoders' own nodes, and the engine would have to run every producer of those nodes'
    other inputs -- the whole sigma-net / attention-head backward -- before it could hand the gradients out);
    ``torch.autograd.backward(cut_outputs, grads)`` continues from here."""

    @staticmethod
    def forward(ctx, *tensors):
        ctx.set_materialize_grads(False)
        return tuple(t.view_as(t) for t in tensors)

    @staticmethod
    def backward(ctx, *grads):
        return grads


def _publish(motion_preds, motion_net, raw, **formulas):
    """The reference updates its result in place (d_xyz += ..., d_xyz *= p_scale, gaussian_renderer/__init__.py:207-217,
    :387): the dictionary it returns under "motion" -- and motion_net.cache, the same object, which the mouth branch reads
    at inference (:362-363) -- holds the combined, scaled values, and so do the regularisers of train_face.py:508-514.
    The operators never materialise them: entry ``key`` becomes ``formulas[key](*raw)``, built on first access, in
    ``motion_preds`` from the attached tensors and, if the network keeps one, in its cache from the detached ones."""
    cache = getattr(motion_net, "cache", None)
    detached = tuple(t.detach() for t in raw)
    for key, formula in formulas.items():
        motion_preds[key] = lambda formula=formula: formula(*raw)
        if cache is not None:
            cache[key] = lambda formula=formula: formula(*detached)


def _aligned_d_xyz(h, p):
    """d_xyz * p_scale (:217) from an 11-column head output and the raw alignment head."""
    return (h[..., :3] * 1e-2) * (torch.tanh(p[..., 3:] / 5) * 0.25 + 1)


# The clauses of the paths' predicates.  (Before they were shared, some sites asked ``is not None`` and some
# ``torch.is_tensor``, some through LazyOutputs.get and some through dict.get: for what the networks return -- an eager
# tensor or no entry -- these agree.  Only the personalised field's head is lazy, and _present does not run it.)
def _raw(preds, key, cols=None):
    """preds[key] if it is a tensor (of ``cols`` columns), else None."""
    t = preds.get(key) if preds is not None else None
    return t if torch.is_tensor(t) and (cols is None or t.shape[-1] == cols) else None


def _present(preds, key):
    """Whether preds has the entry, without evaluating a lazy one."""
    return preds is not None and dict.get(preds, key) is not None


def _face_operator_ok(pc, f, detach_motion):
    """On the device, with gradients into the fields, and an 11-column universal head: what every face operator needs."""
    return pc.get_xyz.is_cuda and not detach_motion and _raw(f.motion, "_h", 11) is not None


def _pretrain_face_applies(pc, f, personalized, align, detach_motion):
    return personalized and not align and _face_operator_ok(pc, f, detach_motion) and _present(f.p_motion, "_h")


def _deform_pretrain_face(pc, motion_net, f, others, with_reg):
    """The pretraining operator (glue.pretrain_deform): both heads and the other identities' in one kernel per pass."""
    from .glue import pretrain_deform
    h_u, h_p = f.motion["_h"], f.p_motion["_h"]
    outs = pretrain_deform(f.xyz_route, pc._scaling, pc._rotation, pc._opacity, h_u, h_p, others, with_reg=with_reg)
    _publish(f.motion, motion_net, (h_u, h_p), d_xyz=lambda u, p: u[..., :3] * 1e-2 + p[..., :3] * 1e-2,
             d_scale=lambda u, p: u[..., 8:11] + p[..., 8:11], d_rot=lambda u, p: u[..., 3:7] + p[..., 3:7])
    return _Deformed(*outs[:4], motion_reg=outs[4] if with_reg else None)


def _fused_pers_applies(pc, f, personalized, align, detach_motion, motion_reg_weight):
    return (align and personalized and motion_reg_weight is None and _face_operator_ok(pc, f, detach_motion)
            and _present(f.p_motion, "_p") and _present(f.p_motion, "_h"))


def _deform_fused_pers(pc, motion_net, f):
    """personalized + align (synthesize_fuse.py:55 with --personalized): the two fields' head outputs add before
    everything the deform operator does ((d_xyz + p.d_xyz) * p_scale, scaling + d_scale + p.d_scale, ...), so the same
    operator serves with h + h_p -- one add launch instead of ~20 elementwise ones each way."""
    from .glue import deform_activate
    h_sum = f.motion["_h"] + f.p_motion["_h"]
    p = f.p_route if f.p_route is not None else f.p_motion["_p"]
    outs = deform_activate(f.xyz_route, pc._scaling, pc._rotation, pc._opacity, h_sum, p)
    _publish(f.motion, motion_net, (h_sum, p), d_xyz=_aligned_d_xyz, d_scale=lambda h, p: h[..., 8:11],
             d_rot=lambda h, p: h[..., 3:7])
    return _Deformed(*outs[:4])


def _fused_applies(pc, f, personalized, align, detach_motion):
    return align and not personalized and _face_operator_ok(pc, f, detach_motion) and _present(f.p_motion, "_p")


def _deform_fused(pc, motion_net, f, motion_reg_weight, backward_cut, with_attn):
    """align: deltas + softplus / normalize / sigmoid in one HIP kernel per pass (glue.deform_activate), which also
    computes the regulariser (on the scaled displacement) when given its weight."""
    from .glue import deform_activate
    xyz, h, cut = f.xyz_route, f.motion["_h"], None
    p = f.p_route if f.p_route is not None else f.p_motion["_p"]
    if backward_cut:
        # every tensor through which a gradient crosses from the rasterizer side (deform operator, attention
        # colours) to the motion fields goes through one identity node: the three-segment step's cut
        amb = f.motion["_amb3"] if with_attn else None
        cut = list(_BackwardCut.apply(*[t for t in (xyz, h, p, amb) if t is not None]))
        xyz, h, p = cut[:3]
    outs = deform_activate(xyz, pc._scaling, pc._rotation, pc._opacity, h, p, motion_reg_weight)
    _publish(f.motion, motion_net, (f.motion["_h"], f.p_motion["_p"]), d_xyz=_aligned_d_xyz)
    return _Deformed(*outs[:4], motion_reg=outs[4] if motion_reg_weight is not None else None, cut=cut)


def _deform_composed_face(pc, motion_net, f, personalized, align, detach_motion):
    """The reference's lines with torch operators: every combination the operators above do not take."""
    m, pm = f.motion, f.p_motion
    d_xyz, d_scale, d_rot = m["d_xyz"], m["d_scale"], m["d_rot"]
    own = {}
    if personalized:
        d_xyz, d_scale, d_rot = d_xyz + pm["d_xyz"], d_scale + pm["d_scale"], d_rot + pm["d_rot"]
        own.update(d_scale=lambda x, s, r: s, d_rot=lambda x, s, r: r)
    if align:
        d_xyz = d_xyz * pm["p_scale"]
    if personalized or align:
        _publish(m, motion_net, (d_xyz, d_scale, d_rot), d_xyz=lambda x, s, r: x, **own)
    if detach_motion:
        d_xyz, d_scale, d_rot = d_xyz.detach(), d_scale.detach(), d_rot.detach()
    return _Deformed(f.xyz_route + d_xyz, pc.scaling_activation(pc._scaling + d_scale),
                     pc.rotation_activation(pc._rotation + d_rot), pc.get_opacity)


def _mouth_scale(motion_net):
    return getattr(motion_net, "XYZ_SCALE", (1e-2 / 5, 1e-2, 1e-2 / 5))


def _deform_pretrain_mouth(pc, motion_net, f, other, with_reg):
    """The mouth pretraining operator (glue.pretrain_mouth_deform); render_motion_mouth_con's guard is its predicate."""
    h, hs, h_p = _raw(f.motion, "_h", 7), _raw(f.motion, "_hs"), _raw(f.p_motion, "_h", 7)
    if h is None or hs is None or h_p is None:
        raise RuntimeError("pretrain_other / pretrain_reg: both fields' raw 7-column heads are needed")
    from .glue import pretrain_mouth_deform
    scale = _mouth_scale(motion_net)
    outs = pretrain_mouth_deform(f.xyz_route, pc._scaling, pc._rotation, pc._opacity, h, hs, h_p, other,
                                 with_reg=with_reg, xyz_scale=scale)
    _publish(f.motion, motion_net, (h, hs, h_p),
             d_xyz=lambda h, hs, h_p: (h[..., :3] * h.new_tensor(scale)) * torch.sigmoid(hs) * 2 + h_p[..., :3] * 1e-2)
    return _Deformed(*outs[:4], motion_reg=outs[4] if with_reg else None)


def _mouth_activate_applies(f, personalized):
    h = _raw(f.motion, "_h", 7)
    return not personalized and h is not None and h.is_cuda and _raw(f.motion, "_hs") is not None


def _deform_mouth_activate(pc, motion_net, f):
    """Gated displacement + softplus / normalize / sigmoid in one HIP kernel per pass (glue.mouth_activate)."""
    from .glue import mouth_activate
    return _Deformed(*mouth_activate(f.xyz_route, pc._scaling, pc._rotation, pc._opacity, f.motion["_h"],
                                     f.motion["_hs"], _mouth_scale(motion_net)))


def _deform_composed_mouth(pc, f, personalized):
    # (unlike :387, and the pretraining path above, this path has never written the sum back to the dictionary)
    d_xyz = f.motion["d_xyz"]
    if personalized:
        d_xyz = d_xyz + f.p_motion["d_xyz"]
    return _Deformed(f.xyz_route + d_xyz, pc.get_scaling, pc.rotation_activation(pc._rotation), pc.get_opacity)


# ---- stage 4: the raster passes --------------------------------------------------------------------------------------
def _attention_colors(preds):
    if preds.get("_amb3") is not None:
        return preds["_amb3"]
    eye = preds["ambient_eye"]
    return torch.cat([preds["ambient_aud"], eye, torch.zeros_like(eye)], dim=-1)


def _render_passes(rasterizer, pc, screenspace_points, d, f, return_attn=False, personalized=False, need_geometry=True):
    """The main pass and the attention maps -> (the main pass's outputs, attn, p_attn, forked).  The universal field's
    map is rendered over the same (detached) geometry as the image, so it rides along the main pass as an auxiliary
    colour set (one preprocess / binning / sort instead of two); the personalised field's is a pass of its own."""
    from . import _lib
    dev = d.means3D.device
    ones = _constant("ones", d.opacity, torch.ones_like)       # the extra_attrs column

    def p_attn_pass(carrier):
        return rasterizer(means3D=d.means3D.detach(), means2D=carrier, shs=None,
                          colors_precomp=_attention_colors(f.p_motion), opacities=d.opacity.detach(),
                          scales=d.scales.detach(), rotations=d.rotations.detach(), cov3Ds_precomp=None,
                          extra_attrs=ones)[0]

    p_attn = None
    fork = return_attn and personalized and d.means3D.is_cuda and _lib.may_fork(dev)
    if fork:
        # the personalised pass only shares inputs with the main pass: it runs on a second stream
        main_stream, side = torch.cuda.current_stream(dev), _side_stream(dev)
        # The screen-space gradient carrier is a leaf that the side-stream pass AND the main pass write a gradient to.
        # A leaf's gradient accumulator runs on ONE stream (the one current at the leaf's first use): fed directly from
        # two streams, one of the producers always mismatches ("AccumulateGrad node's stream does not match").  The side
        # pass therefore gets a view made HERE, on the main stream: its gradient reaches the leaf through the view's
        # backward node, which runs where the view was made.
        side_carrier = screenspace_points.view_as(screenspace_points)
        side.wait_stream(main_stream)
        with torch.cuda.stream(side):
            p_attn = p_attn_pass(side_carrier)
    # (dc and rest coefficients as the pair the model stores: no concatenation, no slice copies in backward)
    shs = pc.get_features_pair if (d.means3D.is_cuda and hasattr(pc, "get_features_pair")) else pc.get_features
    extra = {} if need_geometry else {"geometry": False}
    if return_attn:
        # (with the cut, the attention colours are its fourth output -- absent if the field has no ``_amb3``)
        extra["aux_colors"] = _attention_colors(f.motion) if d.cut is None else (d.cut[3] if len(d.cut) > 3 else None)
    outs = rasterizer(means3D=d.means3D, means2D=screenspace_points, shs=shs, colors_precomp=None, opacities=d.opacity,
                      scales=d.scales, rotations=d.rotations, cov3Ds_precomp=None, extra_attrs=ones, **extra)
    if fork:
        main_stream.wait_stream(side)
        _keepalive.cross_stream(p_attn, main_stream)
    elif return_attn and personalized:
        p_attn = p_attn_pass(screenspace_points)
    return outs, (outs[6] if return_attn else None), p_attn, fork


def render_motion(viewpoint_camera, pc, motion_net, pipe=None, bg_color=None, scaling_modifier=1.0, frame_idx=None,
                  return_attn=False, personalized=False, align=False, detach_motion=False, motion_reg_weight=None,
                  pretrain_heads=None, pretrain_reg=True, need_geometry=True, backward_cut=False):
    """Render with the universal (motion_net) and personalised (pc.neural_motion_grid) motion fields.
    ``motion_reg_weight`` (extension): also return ``motion_reg`` = partial sums of weight * the motion regulariser of
    train_face.py:510-514, computed inside the fused deform operator (None when that operator is not used).
    ``pretrain_heads`` (extension, personalized=True and align=False only): the other identities' PMF head outputs
    [N,11] of the pretraining step (pretrain_face.py); the deformation runs in the pretraining operator
    (glue.pretrain_deform) and ``motion_reg`` holds partial sums of that step's regularisers and contrast term
    (``pretrain_reg=False``: not computed, ``motion_reg`` is None).
    ``need_geometry=False`` (extension): the caller reads neither ``depth`` nor ``normal`` -- both are None and the
    rasterizer runs its colour-only forward blend; everything else is bit-identical.
    ``backward_cut=True`` (extension, FaceTrainer's three-segment step): the fused align path routes what it reads of
    the fields through one _BackwardCut node, whose outputs are returned under ``_cut`` (None on every other path)."""
    screenspace_points, rasterizer = _begin(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    exp_feat = viewpoint_camera.talking_dict["au_exp"].to(pc.get_xyz.device, non_blocking=True)

    def announce(audio_feat):
        # both networks' audio branches depend only on the frame: start them now, each on its own side stream
        if hasattr(motion_net, "start_audio"):
            motion_net.start_audio(audio_feat, 1, exp_feat)
            if personalized and hasattr(pc.neural_motion_grid, "start_audio"):
                # (with align only, the personalised field's deformation head is never read: motion_net.py)
                pc.neural_motion_grid.start_audio(audio_feat, 2, exp_feat)

    # (the fused shift asks for the universal field's class and a non-None ``_p`` here, for an XYZ_SCALE attribute and a
    # tensor ``_p`` in the mouth render, and only this render flushes the deferred weight gradients from the shift's
    # gradient hook.  The first two look accidental; all three are kept as found -- unifying them is a behaviour change)
    f = _evaluate_fields(viewpoint_camera, pc, motion_net, personalized, align, exp_feat, announce=announce,
                         fused_shift=lambda p: p.get("_p") if isinstance(motion_net, _MotionNetwork) else None,
                         p_exp=exp_feat, flush_on_shift_grad=True)
    if pretrain_heads is not None:
        if not _pretrain_face_applies(pc, f, personalized, align, detach_motion):
            raise RuntimeError("pretrain_heads: the pretraining deform operator needs personalized=True, align=False, "
                               "both fields' fused heads and the GPU")
        d = _deform_pretrain_face(pc, motion_net, f, pretrain_heads, pretrain_reg)
    elif _fused_pers_applies(pc, f, personalized, align, detach_motion, motion_reg_weight):
        d = _deform_fused_pers(pc, motion_net, f)
    elif _fused_applies(pc, f, personalized, align, detach_motion):
        d = _deform_fused(pc, motion_net, f, motion_reg_weight, backward_cut, return_attn)
    else:
        d = _deform_composed_face(pc, motion_net, f, personalized, align, detach_motion)
    outs, rendered_attn, p_rendered_attn, forked = _render_passes(
        rasterizer, pc, screenspace_points, d, f, return_attn, personalized, need_geometry)
    image, depth, normal, alpha, radii = outs[:5]
    return LazyOutputs({"render": image, "viewspace_points": screenspace_points,
            "visibility_filter": lambda: radii > 0,      # one launch, only when somebody reads it
            "depth": depth, "alpha": alpha, "normal": normal, "radii": radii, "motion": f.motion,
            "p_motion": f.p_motion if personalized or align else None, "attn": rendered_attn,
            "p_attn": p_rendered_attn, "motion_reg": d.motion_reg,
            "_cut": d.cut if (return_attn and not forked) else None})


def _top_values(v, kmax, largest):
    """The kmax largest (smallest) values of a 1-D tensor, sorted, by row-wise top-k over 512-element rows until
    fewer than 10,000 candidates are left.  (torch.topk on a 1-D tensor of >= 10,000 elements takes a full-sort
    path on ROCm, which does not survive stream capture; the row-wise form selects the same values.)"""
    pad = float("-inf") if largest else float("inf")
    v = v.reshape(-1)
    while v.numel() >= 10000:
        rows = (v.numel() + 511) // 512
        v = torch.nn.functional.pad(v, (0, rows * 512 - v.numel()), value=pad).view(rows, 512)
        v = v.topk(min(kmax, 512), 1, largest, False).values.reshape(-1)
    return v.topk(min(kmax, v.numel()), 0, largest, True).values


def _extreme_values(v, k):
    """(the k largest values descending, the k smallest ascending) of a 1-D tensor: one HIP operator on the device
    (csrc/select.hip, k <= 64), torch.topk otherwise."""
    v = v.reshape(-1)
    k = min(int(k), v.numel())
    if v.is_cuda and v.dtype == torch.float32 and 1 <= k <= 64:
        from . import _lib
        L = _lib.lib()
        v = v.contiguous()
        top = torch.empty(k, dtype=torch.float32, device=v.device)
        bottom = torch.empty(k, dtype=torch.float32, device=v.device)
        ws = torch.empty(L.instag_extreme_values_workspace_bytes(v.numel(), k), dtype=torch.uint8, device=v.device)
        _lib.check(L.instag_extreme_values(_lib.ptr(v), v.numel(), k, _lib.ptr(top), _lib.ptr(bottom), _lib.ptr(ws),
                                           ws.numel(), _lib.current_stream()), "extreme_values")
        return top, bottom
    return _top_values(v, k, True), _top_values(v, k, False)


def _jaw_feature(h, column, scale, k):
    """[1,3] = [max, min, max - min] * 1e2 of the k-th largest / smallest value of scale * h[:, column] in one operator
    (csrc/select.hip instag_jaw_feature).  ``k``: int, or int64 tensor on the device (clamped to [1, 50])."""
    from . import _lib
    L = _lib.lib()
    N, stride = h.shape[0], h.shape[1]
    dev_k = torch.is_tensor(k)
    kmax = min(50, N) if dev_k else min(int(k), N)
    out = torch.empty(1, 3, dtype=torch.float32, device=h.device)
    ws = torch.empty(L.instag_jaw_feature_workspace_bytes(N, kmax), dtype=torch.uint8, device=h.device)
    _lib.check(L.instag_jaw_feature(_lib.ptr(h), N, stride, column, float(scale), kmax, _lib.ptr(k) if dev_k else None,
                                    0 if dev_k else kmax, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.current_stream()),
               "jaw_feature")
    return out


@torch.no_grad()
def _jaw_movement(pc_face, motion_net_face, audio_feat, neutral, k):
    """[1,3] jaw-movement feature of the mouth branch: [max, min, max - min] * 1e2 of the k-th largest / smallest vertical
    displacement the FACE field predicts -- for a neutral expression, or (``neutral`` None: inference) as the face pass
    left it in its cache.  (gaussian_renderer/__init__.py:361 evaluates the face field with autograd on and then reads
    it under no_grad only, :365-372: no gradient can reach it.  Evaluated without a graph here: same values, no
    activations saved, and -- when this pass runs on a stream of its own beside the face pass -- no gradient accumulators
    of the face field's parameters created on that stream.)"""
    preds = motion_net_face.cache if neutral is None else motion_net_face(pc_face.get_xyz, audio_feat, neutral)
    h_face = None if neutral is None else dict.get(preds, "_h")
    if (torch.is_tensor(h_face) and h_face.is_cuda and h_face.dim() == 2 and h_face.is_contiguous()
            and h_face.dtype == torch.float32 and h_face.shape[0] >= 1 and (torch.is_tensor(k) or 1 <= int(k) <= 64)
            and (not torch.is_tensor(k) or (k.is_cuda and k.dtype == torch.int64))):
        # d_xyz[:, 1] = h[:, 1] * 1e-2 (scene/motion_net.py:330): selection, gather and the three products in one operator
        return _jaw_feature(h_face.detach(), 1, 1e-2, k)
    dy = preds["d_xyz"][..., 1]
    if torch.is_tensor(k):
        # k on the device (int64 [1], 1 <= k <= 50): a captured step draws a new k per replay without a host
        # round trip -- the 50 largest / smallest once, the k-th of them by index
        kmax = min(50, dy.shape[0])
        kidx = (k.reshape(1) - 1).clamp(0, kmax - 1)
        top, bottom = _extreme_values(dy, kmax)
        motion_max, motion_min = top.gather(0, kidx)[0], bottom.gather(0, kidx)[0]
    else:
        top, bottom = _extreme_values(dy, k)
        motion_max, motion_min = top[-1], bottom[-1]
    return torch.stack([motion_max, motion_min, motion_max - motion_min]).reshape(1, 3) * 1e2


def render_motion_mouth_con(viewpoint_camera, pc, motion_net, pc_face, motion_net_face, pipe=None, bg_color=None,
                            scaling_modifier=1.0, frame_idx=None, return_attn=False, personalized=False, align=False,
                            k=10, inference=False, pretrain_other=None, pretrain_reg=None):
    """Mouth branch (gaussian_renderer/__init__.py:302-435): the mouth field is conditioned on a 3-element jaw
    movement feature derived (without gradient) from the k-th largest / smallest vertical displacement the FACE
    field predicts for the face Gaussians with a neutral expression.
    ``pretrain_reg`` (extension, personalized=True and align=False on the device only; None = off): the deformation
    runs in the mouth pretraining operator (glue.pretrain_mouth_deform), which adds the personalised displacement to
    the mouth field's as the reference does IN PLACE (:387); True also returns ``motion_reg`` = partial sums of the
    per-Gaussian loss terms of pretrain_mouth.py:231-276, False returns ``motion_reg`` = None.  ``pretrain_other``: the
    contrast partner's PMF head output [N,7] (None: no contrast term)."""
    pretrain = pretrain_reg is not None or pretrain_other is not None
    if pretrain and not (personalized and not align and not inference and pc.get_xyz.is_cuda):
        raise RuntimeError("pretrain_other / pretrain_reg: the mouth pretraining deform operator needs "
                           "personalized=True, align=False, inference=False and the GPU")
    if pretrain_other is not None and not pretrain_reg:
        raise RuntimeError("pretrain_other: the contrast term is part of the partial sums (pretrain_reg=True)")
    screenspace_points, rasterizer = _begin(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    neutral = None if inference else _neutral_expression(viewpoint_camera, pc.get_xyz.device)

    def announce(audio_feat):
        # the per-frame branches of both fields depend on the frame only: announce them now, each on its own side stream
        if hasattr(motion_net, "start_audio"):
            motion_net.start_audio(audio_feat, 2)
        if not inference and hasattr(motion_net_face, "start_audio"):
            motion_net_face.start_audio(audio_feat, 1, neutral)

    def fused_shift(p_preds):
        p_raw = dict.get(p_preds, "_p")
        return p_raw if torch.is_tensor(p_raw) and getattr(motion_net, "XYZ_SCALE", None) is not None else None

    f = _evaluate_fields(viewpoint_camera, pc, motion_net, personalized, align,
                         lambda audio_feat: _jaw_movement(pc_face, motion_net_face, audio_feat, neutral, k).detach(),
                         announce=announce, fused_shift=fused_shift)
    if pretrain:
        d = _deform_pretrain_mouth(pc, motion_net, f, pretrain_other, bool(pretrain_reg))
    elif _mouth_activate_applies(f, personalized):
        d = _deform_mouth_activate(pc, motion_net, f)
    else:
        d = _deform_composed_mouth(pc, f, personalized)
    image, depth, normal, alpha, radii = _render_passes(rasterizer, pc, screenspace_points, d, f)[0][:5]
    return LazyOutputs({"render": image, "viewspace_points": screenspace_points,
                        "visibility_filter": lambda: radii > 0,          # built on first access
                        "depth": depth, "alpha": alpha, "radii": radii, "motion": f.motion,
                        "p_motion": f.p_motion if personalized or align else None,
                        **({"motion_reg": d.motion_reg} if pretrain else {})})


def render_fuse(viewpoint_camera, pc, motion_net, pc_mouth, motion_net_mouth, pipe=None, bg_color=None,
                scene_background=None, personalized=False, inference=False, k=10, compose=True):
    """Face + mouth composition of the fuse stage: train_fuse_con.py:102-121 (training: both passes carry gradients
    and were rendered over ``bg_color``, which is taken out again) / synthesize_fuse.py:46-66 (inference: the mouth
    field reads the face field's cached motion).  ``scene_background`` [3,H,W] in [0,1] is what shows through both.
    -> dict(image, face=<render_motion pkg>, mouth=<render_motion_mouth_con pkg>).  ``compose=False`` (extension): the two
    passes only, ``image`` and ``mouth_image`` are None (the inference epilogue of metrics.infer_compose composes)."""
    from . import _lib
    dev = pc.get_xyz.device
    if CONCURRENT_FUSE_PASSES and dev.type == "cuda" and not inference and _lib.may_fork(dev):
        # In training the mouth pass re-evaluates the face field with a neutral expression (it does not read the face
        # pass's cache): the two passes share nothing but parameters, so the mouth pass -- forward here, and with it
        # its whole backward -- runs on a second stream beside the face pass.  Each pass alone is a chain of short
        # kernels that leaves most of the chip idle.
        main, side = torch.cuda.current_stream(dev), _side_stream(dev, "fuse")
        _lib.leaf_stream(side)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            mouth = render_motion_mouth_con(viewpoint_camera, pc_mouth, motion_net_mouth, pc, motion_net, pipe, bg_color,
                                            personalized=personalized, align=True, k=k, inference=False)
        face = render_motion(viewpoint_camera, pc, motion_net, pipe, bg_color, personalized=personalized, align=True)
        main.wait_stream(side)
        for t in (mouth["render"], mouth["alpha"], mouth["depth"], mouth["radii"]):
            _keepalive.cross_stream(t, main)
    else:
        face = render_motion(viewpoint_camera, pc, motion_net, pipe, bg_color, personalized=personalized, align=True)
        mouth = render_motion_mouth_con(viewpoint_camera, pc_mouth, motion_net_mouth, pc, motion_net, pipe, bg_color,
                                        personalized=personalized, align=True, k=k, inference=inference)
    if not compose:
        return {"image": None, "mouth_image": None, "face": face, "mouth": mouth}
    alpha, alpha_mouth = face["alpha"], mouth["alpha"]
    fr, mr = face["render"], mouth["render"]
    if (fr.is_cuda and fr.dim() == 3 and fr.shape[0] == 3 and fr.dtype == torch.float32 and mr.shape == fr.shape
            and alpha.numel() == fr.shape[1] * fr.shape[2] and alpha_mouth.numel() == alpha.numel()
            and (scene_background is None or scene_background.shape == fr.shape)):
        from .glue import fuse_compose          # ~13 broadcast launches forward, ~25 backward otherwise
        image, mouth_image = fuse_compose(fr, alpha, mr, alpha_mouth, bg_color, scene_background)
    else:
        bg3 = bg_color[:, None, None]
        if scene_background is None:
            scene_background = torch.zeros_like(fr)
        mouth_image = mr - bg3 * (1.0 - alpha_mouth) + scene_background * (1.0 - alpha_mouth)
        image = fr - bg3 * (1.0 - alpha) + mouth_image * (1.0 - alpha)
    return {"image": image, "mouth_image": mouth_image, "face": face, "mouth": mouth}
