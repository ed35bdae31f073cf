"""A motion field's tri-plane encode and the MLPs that read its rows as ONE forward launch (csrc/mlp.hip:
triplane_mlp_forward_kernel, triplane_mlp2_forward_kernel).

Boundary: ``PersonalizedMotionNetwork.forward`` up to the alignment head (encode_x + align_net) and
``_TriPlaneField._trunk`` up to the attention heads (encode_x + aud_ch_att_net + eye_att_net).  One autograd node per
field stands for the two nodes of the split path (gridencoder._tri_plane_encode, then mlp._FusedMLP or
mlp._SharedInputMLPs); its backward issues those nodes' launches, in their order, through the functions they use
themselves, so only the forward differs -- and that in the number of launches, not in a bit of any result.

``INSTAG_ENCODE_MLP=split`` selects the two-launch path everywhere (shapes without a fused kernel -- the mouth field's
tables do not fit LDS -- take it anyway).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib, gridencoder as _ge, mlp as _mlp
from ._lib import check, ptr


def enabled() -> bool:
    return os.environ.get("INSTAG_ENCODE_MLP", "fused") != "split"


def _two_layer(net) -> bool:
    return net.num_layers == 2 and _mlp.supported(net.dim_in, net.dim_hidden, net.dim_out, 2)


def supported(field, x, heads) -> bool:
    """Does ``field`` (a _TriPlaneField) have a fused kernel for its encode + ``heads`` (a list of one or two MLP modules)
    at positions ``x``?"""
    if not (enabled() and x.is_cuda and x.dim() == 2 and all(_two_layer(n) for n in heads)):
        return False
    encs = (field.encoder_xy, field.encoder_yz, field.encoder_xz)
    if not _ge.tri_plane_supported(*encs):
        return False
    e0 = encs[0]
    if any(n.dim_in != 3 * e0.num_levels for n in heads):
        return False
    a, b = heads[0], heads[-1]
    return bool(_lib.lib().instag_triplane_mlp_supported(e0.num_levels, e0.embeddings.shape[0], len(heads), a.dim_hidden,
                                                         a.dim_out, b.dim_hidden, b.dim_out))


def _encoder_args(field):
    e0 = field.encoder_xy
    return (field.encoder_xy.embeddings, field.encoder_yz.embeddings, field.encoder_xz.embeddings, e0.offsets,
            float(np.log2(e0.per_level_scale)), int(e0.base_resolution))


def _route(xyz, shift):
    """Hand the position (and shift) on as outputs of the node?  (gridencoder.passthrough, same rule as tri_plane_encode)"""
    return _ge._PASS is not None and torch.is_grad_enabled() and xyz.requires_grad \
        and xyz.is_contiguous() and xyz.dtype == torch.float32 \
        and (shift is None or (shift.is_contiguous() and shift.dtype == torch.float32))


def _prepare(xyz, embs, offsets, shift):
    xyz = xyz.contiguous().float()
    tabs = [e.contiguous().float() for e in embs]
    _ge._check_inputs(xyz=xyz, offsets=offsets, emb_xy=tabs[0], emb_yz=tabs[1], emb_xz=tabs[2])
    shift = None if shift is None else shift.contiguous().float()
    return xyz, tabs, shift


class _EncodeAlign(torch.autograd.Function):
    """(align_net(enc_x), enc_x[, xyz]) with enc_x = tri_plane_encode(xyz): _tri_plane_encode + _FusedMLP."""

    @staticmethod
    def forward(ctx, xyz, emb_xy, emb_yz, emb_xz, offsets, S, H, bound, w1, w2, passthrough, max_blocks):
        xyz, tabs, _ = _prepare(xyz, (emb_xy, emb_yz, emb_xz), offsets, None)
        w1c, w2c = w1.contiguous().float(), w2.contiguous().float()
        N, L, T = xyz.shape[0], offsets.shape[0] - 1, tabs[0].shape[0]
        HA, OA = w1c.shape[0], w2c.shape[0]
        keep = any(ctx.needs_input_grad)
        dev = xyz.device
        enc_x = torch.empty(N, 3 * L, device=dev, dtype=torch.float32)
        y = torch.empty(N, OA, dtype=torch.float32, device=dev)
        a1 = torch.empty(N, HA, dtype=torch.float32, device=dev) if keep else None
        s1 = _mlp.sign_words(N, dev) if keep else None
        check(_lib.lib().instag_triplane_mlp_forward(
            ptr(xyz), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(offsets), None, 0, 1.0, N, L, S, H, float(bound), T,
            ptr(w1c), ptr(w2c), ptr(enc_x), ptr(y), ptr(a1), ptr(s1), HA, OA, max_blocks, _lib.current_stream()),
            "triplane_mlp_forward")
        _mlp.STATS["fwd_flops"] += 2 * N * (3 * L * HA + HA * OA)
        ctx.save_for_backward(xyz, tabs[0], tabs[1], tabs[2], offsets, enc_x, w1c, w2c, a1, s1)
        ctx.meta = (N, L, S, H, float(bound), T, 1.0)
        ctx.weights = (w1, w2, None)
        ctx.routed = bool(passthrough)
        # an output nothing read arrives as None: the split path then runs no launch for it either
        ctx.set_materialize_grads(False)
        return (y, enc_x, xyz) if passthrough else (y, enc_x)

    @staticmethod
    def backward(ctx, dy, d_enc, g_xyz=None):
        xyz, t0, t1, t2, offsets, enc_x, w1, w2, a1, s1 = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_enc = any(need[:4])
        grads = (None, None, None)
        dx = d_enc
        if dy is not None:
            dx, *grads = _mlp.mlp_backward((enc_x, w1, w2, None, a1, None, s1, None), dy, want_enc, ctx.weights,
                                           (need[8], need[9], False))
            if d_enc is not None and dx is not None:
                dx = dx + d_enc                  # the sum autograd forms for a tensor with two consumers
        if not want_enc or dx is None:
            return (None,) * 8 + (grads[0], grads[1], None, None)
        if ctx.routed and g_xyz is None:
            g_xyz = torch.zeros_like(xyz)        # (as autograd hands _tri_plane_encode an output nothing read)
        dxyz, dt, _ = _ge.tri_plane_backward((xyz, t0, t1, t2, offsets), None, ctx.meta, dx, g_xyz, None, need[0], False)
        return (dxyz, dt[0], dt[1], dt[2], None, None, None, None, grads[0], grads[1], None, None)


class _EncodeHeads(torch.autograd.Function):
    """(MLP_a(enc_x), MLP_b(enc_x), enc_x[, xyz[, shift]]) with enc_x = tri_plane_encode(xyz, shift): _tri_plane_encode +
    _SharedInputMLPs."""

    @staticmethod
    def forward(ctx, xyz, emb_xy, emb_yz, emb_xz, offsets, S, H, bound, shift, shift_scale, wa1, wa2, wb1, wb2,
                passthrough, max_blocks):
        xyz, tabs, shift = _prepare(xyz, (emb_xy, emb_yz, emb_xz), offsets, shift)
        ws = [w.contiguous().float() for w in (wa1, wa2, wb1, wb2)]
        N, L, T = xyz.shape[0], offsets.shape[0] - 1, tabs[0].shape[0]
        (HA, OA), (HB, OB) = (ws[0].shape[0], ws[1].shape[0]), (ws[2].shape[0], ws[3].shape[0])
        keep = any(ctx.needs_input_grad)
        dev = xyz.device
        enc_x = torch.empty(N, 3 * L, device=dev, dtype=torch.float32)
        ya = torch.empty(N, OA, dtype=torch.float32, device=dev)
        yb = torch.empty(N, OB, dtype=torch.float32, device=dev)
        a1a = torch.empty(N, HA, dtype=torch.float32, device=dev) if keep else None
        a1b = torch.empty(N, HB, dtype=torch.float32, device=dev) if keep else None
        s1 = _mlp.sign_words(N, dev) if keep else None       # both heads' bits: A low half, B high half
        check(_lib.lib().instag_triplane_mlp2_forward(
            ptr(xyz), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(offsets), ptr(shift),
            0 if shift is None else shift.shape[1], float(shift_scale), N, L, S, H, float(bound), T,
            ptr(ws[0]), ptr(ws[1]), ptr(ws[2]), ptr(ws[3]), ptr(enc_x), ptr(ya), ptr(yb), ptr(a1a), ptr(a1b), ptr(s1),
            HA, OA, HB, OB, max_blocks, _lib.current_stream()), "triplane_mlp2_forward")
        _mlp.STATS["fwd_flops"] += 2 * N * (3 * L * HA + HA * OA + 3 * L * HB + HB * OB)
        ctx.save_for_backward(xyz, tabs[0], tabs[1], tabs[2], offsets, enc_x, ws[0], ws[1], a1a, s1, ws[2], ws[3], a1b,
                              *([shift] if shift is not None else []))
        ctx.meta = (N, L, S, H, float(bound), T, float(shift_scale))
        ctx.weights = (wa1, wa2, wb1, wb2)
        if passthrough:
            return (ya, yb, enc_x, xyz, shift) if shift is not None else (ya, yb, enc_x, xyz)
        return ya, yb, enc_x

    @staticmethod
    def backward(ctx, dya, dyb, d_enc, g_xyz=None, g_shift=None):
        # (all are tensors: autograd hands in zeros for an output that nothing read)
        saved = ctx.saved_tensors
        xyz, t0, t1, t2, offsets, enc_x, wa1, wa2, a1a, s1, wb1, wb2, a1b = saved[:13]
        shift = saved[13] if len(saved) > 13 else None
        need = ctx.needs_input_grad
        want_shift = shift is not None and need[8]
        want_enc = any(need[:4]) or want_shift
        dx, *grads = _mlp.shared_input_backward((enc_x, wa1, wa2, a1a, s1, wb1, wb2, a1b, s1), True, dya, dyb, d_enc,
                                                want_enc, ctx.weights, need[10:14])
        if not want_enc:
            return (None,) * 10 + (*grads, None, None)
        dxyz, dt, dshift = _ge.tri_plane_backward((xyz, t0, t1, t2, offsets), shift, ctx.meta, dx, g_xyz, g_shift,
                                                  need[0], want_shift)
        return (dxyz, dt[0], dt[1], dt[2], None, None, None, None, dshift, None, *grads, None, None)


def _publish_route(res, first, shift):
    if len(res) > first:
        _ge._PASS["xyz"] = res[first]
        if shift is not None:
            _ge._PASS["shift"] = res[first + 1]


def encode_align(field, xyz, bound, net, max_blocks=0):
    """-> (net(enc_x), enc_x) for ``net`` = the field's 2-layer alignment head; needs supported(field, xyz, [net])."""
    w1, w2 = (layer.weight for layer in net.net)
    res = _EncodeAlign.apply(xyz, *_encoder_args(field), bound, w1, w2, _route(xyz, None), max_blocks)
    _publish_route(res, 2, None)
    return res[0], res[1]


def encode_heads(field, xyz, bound, shift, net_a, net_b, max_blocks=0):
    """-> (net_a(enc_x), net_b(enc_x), enc_x); ``shift`` = None or (tensor [N, >=3], scale) as _TriPlaneField.encode_x;
    needs supported(field, xyz, [net_a, net_b])."""
    sh, scale = (None, 1.0) if shift is None else shift
    weights = [layer.weight for net in (net_a, net_b) for layer in net.net]
    res = _EncodeHeads.apply(xyz, *_encoder_args(field), bound, sh, scale, *weights, _route(xyz, sh), max_blocks)
    _publish_route(res, 3, sh)
    return res[0], res[1], res[2]
