"""Per-frame conditioning codes of a motion network as one HIP launch per pass (csrc/audio.hip).

Replaces, on the device, the reference's chain
    enc_a = audio_att_net(audio_net(a).unsqueeze(0))          scene/motion_net.py:283-289 / :672-677
    enc_e = cat(exp_encode_net(e[:-1]), e[-1:])               scene/motion_net.py:297-299 / :684-686
(~11 conv1d / GEMM launches plus activations, three times that in backward) by one launch each way.
A network built with audio_extractor == 'ave' has AudioNet_ave (scene/motion_net.py:132-149: three linear layers on
[8, 1, 512] windows) in AudioNet's place: the instag_frame_code_ave_* pair, 20 parameters instead of 26.
A 'hubert' network has the stock AudioNet at dim_in 1024 / mid 128 on windows of two samples, [8, 1024, 2]: the
instag_frame_code_wide_* pair, the 26 parameters of the stock family.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr

NPARAM = 26
NPARAM_AVE = 20
_ARRIVAL_SLOTS = 64


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


SPLIT_BACKWARD = True        # False: the single-workgroup backward kernel (tests compare the two)


class _Variant:
    """What tells the two kernel families apart on this side: the C symbols instag_<name>_{saved_floats, forward,
    backward_workspace_bytes, backward}, which take the same arguments but for the integer dimensions (`dims`, dim_aud
    last), and whether the backward pass can use a workspace."""

    def __init__(self, name, workspace):
        self.name, self.workspace = name, workspace

    def symbol(self, what):
        return getattr(_lib.lib(), f"instag_{self.name}_{what}")


_STOCK = _Variant("frame_code", True)          # AudioNet: a [8, dim_in, 16], dims (dim_in, mid, dim_aud), 26 parameters
_AVE = _Variant("frame_code_ave", False)       # AudioNet_ave: a [8, 512], dims (dim_aud,), 20 parameters
_WIDE = _Variant("frame_code_wide", False)     # AudioNet of a 'hubert' head: a [8, dim_in, 2], dims and parameters of _STOCK


class _FrameCodes(torch.autograd.Function):
    """`arrivals` None = the single-workgroup forward."""

    @staticmethod
    def forward(ctx, a, e, variant, dims, arrivals, *params):
        a = a.contiguous().float()
        params = tuple(None if p is None else p.contiguous() for p in params)
        dev = a.device
        n_saved = variant.symbol("saved_floats")(*dims)
        if n_saved < 0:
            raise RuntimeError("frame_codes: unsupported dimensions")
        enc_a = torch.empty(1, dims[-1], dtype=torch.float32, device=dev)
        enc_e = None
        if e is not None:
            e = e.contiguous().float()
            enc_e = torch.empty(6, dtype=torch.float32, device=dev)
        saved = torch.empty(n_saved, dtype=torch.float32, device=dev)
        check(variant.symbol("forward")(ptr(a), ptr(e), _ptr_array(params), ptr(enc_a), ptr(enc_e), ptr(saved), *dims,
                                        ptr(arrivals), _lib.current_stream()),
              variant.name + "_forward")
        ctx.variant, ctx.dims = variant, dims
        ctx.has_e = e is not None
        ctx.save_for_backward(a, saved, *( [e] if e is not None else [] ), *[p for p in params if p is not None])
        ctx.param_mask = [p is not None for p in params]
        if enc_e is None:
            return enc_a, torch.empty(0, device=dev)
        return enc_a, enc_e

    @staticmethod
    def backward(ctx, d_enc_a, d_enc_e):
        variant, dims = ctx.variant, ctx.dims
        tensors = list(ctx.saved_tensors)
        a, saved = tensors[0], tensors[1]
        e = tensors[2] if ctx.has_e else None
        rest = iter(tensors[3 if ctx.has_e else 2:])
        params = [next(rest) if m else None for m in ctx.param_mask]
        if d_enc_a is None:
            d_enc_a = torch.zeros(1, dims[-1], dtype=torch.float32, device=a.device)
        d_enc_a = d_enc_a.contiguous().float()
        d_enc_e = d_enc_e.contiguous().float() if (ctx.has_e and d_enc_e is not None) else None
        grads = [None if p is None else torch.empty_like(p) for p in params]
        # stock: eight workgroups (one per audio window), each with its own row of parameter gradients in `ws`;
        # 'ave' / wide: sixteen workgroups write disjoint rows of the large weight gradients, no workspace
        ws = torch.empty(variant.symbol("backward_workspace_bytes")(*dims), dtype=torch.uint8,
                         device=a.device) if (variant.workspace and SPLIT_BACKWARD) else None
        check(variant.symbol("backward")(ptr(a), ptr(e), _ptr_array(params), ptr(saved), ptr(d_enc_a), ptr(d_enc_e),
                                         _ptr_array(grads), *dims, ptr(ws), 0 if ws is None else ws.numel(),
                                         _lib.current_stream()),
              variant.name + "_backward")
        return (None, None, None, None, None, *grads)


def _attention_params(field):
    """The twelve audio_att_net tensors and the two expression weights (None, None without the expression branch) in
    the C ABI's order, or None when the modules are not the stock architecture."""
    att = field.audio_att_net
    try:
        aconvs = [att.attentionConvNet[i] for i in (0, 2, 4, 6, 8)]
        lin = att.attentionNet[0]
    except (IndexError, AttributeError, TypeError):
        return None
    if [(c.in_channels, c.out_channels) for c in aconvs] != [(att.dim_aud, 16), (16, 8), (8, 4), (4, 2), (2, 1)]:
        return None
    if att.seq_len != 8 or any(m.bias is None for m in aconvs + [lin]):
        return None
    out = []
    for m in aconvs + [lin]:
        out += [m.weight, m.bias]
    if getattr(field, "exp_eye", False):
        net = field.exp_encode_net.net
        if len(net) != 2 or tuple(net[0].weight.shape) != (16, 5) or tuple(net[1].weight.shape) != (5, 16):
            return None
        out += [net[0].weight, net[1].weight]
    else:
        out += [None, None]
    return out


def _is_ave(field) -> bool:
    return not hasattr(field.audio_net, "encoder_conv")


def _module_params_ave(field):
    """The 20 parameters of a network with AudioNet_ave in the C ABI's order, or None when the modules are not the
    stock architecture (three Linear with bias, 512 -> 256 -> 128 -> dim_aud)."""
    an = field.audio_net
    try:
        fcs = [an.encoder_fc1[i] for i in (0, 2, 4)]
        if len(an.encoder_fc1) != 5:
            return None
        slopes = [an.encoder_fc1[i].negative_slope for i in (1, 3)]
        shapes = [(m.in_features, m.out_features) for m in fcs]
    except (IndexError, AttributeError, TypeError):
        return None
    tail = _attention_params(field)
    if tail is None or slopes != [0.02, 0.02] or any(m.bias is None for m in fcs) \
            or shapes != [(512, 256), (256, 128), (128, field.audio_att_net.dim_aud)]:
        return None
    out = []
    for m in fcs:
        out += [m.weight, m.bias]
    return out + tail


def _module_params(field):
    """The 26 parameters in the C ABI's order, or None when the modules are not the stock architecture."""
    an = field.audio_net
    try:
        convs = [an.encoder_conv[i] for i in (0, 2, 4, 6)]
        fcs = [an.encoder_fc1[i] for i in (0, 2)]
    except (IndexError, AttributeError, TypeError):
        return None
    tail = _attention_params(field)
    if tail is None:
        return None
    mid = convs[0].out_channels
    chans = [(c.in_channels, c.out_channels) for c in convs]
    if chans != [(an.encoder_conv[0].in_channels, mid), (mid, mid), (mid, 64), (64, 64)]:
        return None
    if an.win_size != 16 or fcs[0].in_features != 64 or fcs[0].out_features != 64 \
            or fcs[1].out_features != field.audio_att_net.dim_aud or any(m.bias is None for m in convs + fcs):
        return None
    out = []
    for m in convs + fcs:
        out += [m.weight, m.bias]
    return out + tail


def supported(field, a, e) -> bool:
    if not (a.is_cuda and a.dim() == 3 and a.shape[0] == 8):
        return False
    if e is not None and (e.numel() != 6 or not getattr(field, "exp_eye", False)):
        return False
    if e is None and getattr(field, "exp_eye", False):
        return False
    if _is_ave(field):
        if tuple(a.shape[1:]) != (1, 512) or _module_params_ave(field) is None:
            return False
        return _lib.lib().instag_frame_code_ave_saved_floats(field.audio_att_net.dim_aud) > 0
    if a.shape[2] not in (16, 2):
        return False
    params = _module_params(field)
    if params is None or a.shape[1] != field.audio_net.encoder_conv[0].in_channels:
        return False
    # windows of two samples (a 'hubert' head): the wide family, which answers -1 unless mid == 128 and dim_in is one
    # of its sizes
    variant = _STOCK if a.shape[2] == 16 else _WIDE
    return variant.symbol("saved_floats")(a.shape[1], field.audio_net.encoder_conv[0].out_channels,
                                          field.audio_att_net.dim_aud) > 0


def frame_codes(field, a, e):
    """-> (enc_a [1, dim_aud], enc_e [6] or None) for a motion network `field` (UMF or PMF)."""
    ave = _is_ave(field)
    params = _module_params_ave(field) if ave else _module_params(field)
    # arrival counter of the forward's eight workgroups: one word per network (the universal and the personalised
    # field's branches run on different streams at the same time), zero between launches
    # (and per stream: frames streamed through several lanes at once must not share it either)
    # The words live in ONE table per (network, device), allocated outside any capture: a word first needed inside a
    # capture is a free slot of that table, never memory of the capture's private pool that would outlive its graph.
    # (Every stream of the package is a persistent registry stream, _lib.side_stream: handles are never reused.)
    capturing = torch.cuda.is_current_stream_capturing()
    tables = field.__dict__.setdefault("_frame_code_arrivals", {})
    entry = tables.get(a.device)
    if entry is None and not capturing:
        entry = tables[a.device] = (torch.zeros(_ARRIVAL_SLOTS, dtype=torch.int32, device=a.device), {})
    handle = torch.cuda.current_stream(a.device).cuda_stream
    if entry is not None and (handle in entry[1] or len(entry[1]) < _ARRIVAL_SLOTS):
        slot = entry[1].setdefault(handle, len(entry[1]))
        arrivals = entry[0][slot:slot + 1]
    elif ave or a.shape[2] == 2:
        arrivals = None                         # no word this call can own: the single-workgroup forward needs none
    else:
        arrivals = torch.zeros(1, dtype=torch.int32, device=a.device)      # owned by this call (and its capture) only
    e_flat = None if e is None else e.reshape(-1)
    if ave:
        enc_a, enc_e = _FrameCodes.apply(a.reshape(8, 512), e_flat, _AVE, (int(field.audio_att_net.dim_aud),), arrivals,
                                         *params)
    else:
        dims = (int(a.shape[1]), int(field.audio_net.encoder_conv[0].out_channels), int(field.audio_att_net.dim_aud))
        enc_a, enc_e = _FrameCodes.apply(a, e_flat, _STOCK if a.shape[2] == 16 else _WIDE, dims, arrivals, *params)
    return enc_a, (enc_e if e is not None else None)
