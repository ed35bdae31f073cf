"""Geometry priors of an identity: the Sapiens normal and depth networks and the two resizes around them.

What data_utils/sapiens/run.sh of the reference does (lite/scripts/{normal,depth}.sh, lite/demo/vis_{normal,depth}.py,
adhoc_image_dataset.py): the first 500 frames of gt_imgs/ are resized to 1024 x 768 on the 8-bit image, normalised,
go through ``sapiens_0.3b`` in fp32, the output map is resized bilinearly to the frame's own size, and
``sapiens/normal/sapiens_0.3b/<i>.npy`` ([H,W,3], n / (|n| + 1e-5)) and ``sapiens/depth/sapiens_0.3b/<i>.npy`` ([H,W])
are what it saves -- the files ``dataset.read_identity`` loads for a few-shot train split.

    nw = SapiensWeights.load("sapiens_0.3b_normal_render_people_epoch_66_torchscript.pt2")
    dw = SapiensWeights.load("sapiens_0.3b_render_people_epoch_100_torchscript.pt2")
    ids, normal, depth = geometry_identity("data/May", nw, dw, "cuda")        # writes the two .npy trees
    store, meta = open_identity("data/May", "train", "cuda", n_views=100, priors=dict(ids=ids, normal=normal, depth=depth))

The reference loads a TorchScript archive whose code is not in the reference tree, and no checkpoint was at hand: the
network below -- an mmpretrain ``VisionTransformer`` (patch 16 with padding 2, learned positions, no class token,
pre-LayerNorm blocks with eps 1e-6, exact GELU, a final LayerNorm) under an mmseg ``VitNormalHead`` / ``VitDepthHead``
(transposed convolutions 4 / 2 / 1 without bias, 1 x 1 convolutions, each with InstanceNorm and SiLU, and ``conv_seg``)
-- **is written from knowledge of the Sapiens release, not read from it.**  The head's depth, its widths and whether its
norms are affine are taken from the state dict's shapes, not from a table.  The 8-bit resize is this project's own
rule, stated in ``resize_u8_torch``; it is not checked against OpenCV, which is not a dependency.

On the GPU the chain runs in csrc/sapiens.hip (fp32, inference only); the ``*_torch`` functions are the plain-torch
statement of the same arithmetic (any dtype, CPU or GPU) that the tests compare against and a CPU device runs.  The
project ships no weights and fetches none.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from .convnet import FrameOperator, check_frames

MEAN, STD = (123.5, 116.5, 103.5), (58.5, 57.0, 57.5)
PATCH, PATCH_PAD, PATCH_K = 16, 2, 768
HEAD_DIM = 64
VIT_LN_EPS, IN_EPS, NORMAL_EPS = 1e-6, 1e-5, 1e-5
GRID = (64, 48)                     # sapiens_0.3b at 1024 x 768
RAW_C = 4
WORKSPACE_LIMIT = 1 << 30
KINDS = {"normal": 3, "depth": 1}

_PATCH = "backbone.patch_embed.projection."
_LAYER = (("ln1.weight", "h"), ("ln1.bias", "h"), ("attn.qkv.weight", "3hh"), ("attn.qkv.bias", "3h"),
          ("attn.proj.weight", "hh"), ("attn.proj.bias", "h"), ("ln2.weight", "h"), ("ln2.bias", "h"),
          ("ffn.layers.0.0.weight", "ih"), ("ffn.layers.0.0.bias", "i"), ("ffn.layers.1.weight", "hi"),
          ("ffn.layers.1.bias", "h"))


def _refuse(key, why):
    return ValueError(f"sapiens weights: {key!r}: {why}")


class SapiensWeights:
    """The frozen parameters of one network (normal or depth) in fp32 on the CPU, under the release's keys
    (``backbone.*``, ``decode_head.*``).  ``grid``: the token grid (rows, columns) ``pos_embed`` was learned for; the
    network's input is 16 grid[0] x 16 grid[1].  Read from the shapes: ``hidden``, ``heads`` (of 64), ``intermediate``,
    ``layers``, ``deconv`` / ``conv`` (the head's widths), ``deconv_affine`` / ``conv_affine`` and ``out_channels``."""

    def __init__(self, tensors: dict, grid=GRID, heads=None):
        self.grid = (int(grid[0]), int(grid[1]))
        if min(self.grid) < 1:
            raise ValueError(f"sapiens weights: grid = {grid!r}: both sides at least 1")
        self.in_size = (PATCH * self.grid[0], PATCH * self.grid[1])
        self.tensors = self._walk({k: v for k, v in tensors.items() if torch.is_tensor(v)}, heads)
        self._packs, self._converted = {}, (None, None)

    # ---- the state-dict walk ------------------------------------------------------------------------------------------
    def _walk(self, sd, heads):
        from . import _lib
        lim = _lib.SAPIENS
        keep = {}

        def take(key, shape=None, dims=None):
            if key not in sd:
                raise ValueError(f"sapiens weights: the state dict misses {key!r}")
            t = sd[key].detach().to(device="cpu", dtype=torch.float32).contiguous().clone()
            if (shape is not None and tuple(t.shape) != tuple(shape)) or (dims is not None and t.dim() != dims):
                want = f"expected {tuple(shape)}" if shape is not None else f"expected {dims} dimensions"
                raise _refuse(key, f"has shape {tuple(t.shape)}, {want}")
            keep[key] = t
            return t

        pw = take(_PATCH + "weight", dims=4)
        hidden = int(pw.shape[0])
        if tuple(pw.shape[1:]) != (3, PATCH, PATCH):
            raise _refuse(_PATCH + "weight", f"has shape {tuple(pw.shape)}, expected ({hidden}, 3, {PATCH}, {PATCH})")
        if hidden > 1024 or hidden % HEAD_DIM:
            raise _refuse(_PATCH + "weight", f"hidden = {hidden} is not supported: a multiple of {HEAD_DIM}, at most 1024 (the "
                          "larger Sapiens sizes: the LayerNorm kernel holds a row in one wave)")
        self.hidden, self.heads = hidden, hidden // HEAD_DIM
        if heads is not None and hidden != int(heads) * HEAD_DIM:
            raise ValueError(f"sapiens weights: heads = {heads}: hidden / heads must be {HEAD_DIM}, hidden is {hidden}")
        take(_PATCH + "bias", (hidden,))
        pos = take("backbone.pos_embed", dims=3)
        T = self.grid[0] * self.grid[1]
        if tuple(pos.shape) != (1, T, hidden):
            extra = " (one longer: a class token, which this network does not have)" if pos.shape[1] == T + 1 else ""
            raise _refuse("backbone.pos_embed", f"has shape {tuple(pos.shape)}, expected (1, {T}, {hidden}) for grid = "
                          f"{self.grid}{extra}")
        if T > lim["INSTAG_SAPIENS_MAX_TOKENS"]:
            raise ValueError(f"sapiens weights: grid = {self.grid}: {T} tokens, at most {lim['INSTAG_SAPIENS_MAX_TOKENS']}")

        # backbone.layers.{i}.*: every tensor known, the indices 0 .. layers - 1
        known, found = dict(_LAYER), {}
        for key in sd:
            m = re.fullmatch(r"backbone\.layers\.(\d+)\.(.+)", key)
            if m:
                if m.group(2) not in known:
                    raise _refuse(key, "an unknown tensor under backbone.layers (layer scale and other variants are not "
                                  "supported)")
                found.setdefault(int(m.group(1)), set()).add(m.group(2))
        self.layers = len(found)
        if not found or sorted(found) != list(range(self.layers)) or self.layers > lim["INSTAG_SAPIENS_MAX_LAYERS"]:
            raise ValueError(f"sapiens weights: backbone.layers: indices {sorted(found)}, expected 0 .. n - 1 with 1 <= n <= "
                             f"{lim['INSTAG_SAPIENS_MAX_LAYERS']}")
        inter = take("backbone.layers.0.ffn.layers.0.0.weight", dims=2).shape[0]
        self.intermediate = int(inter)
        if inter % 32 or not 32 <= inter <= 65536:
            raise _refuse("backbone.layers.0.ffn.layers.0.0.weight", f"intermediate = {inter} must be a multiple of 32")
        dim = {"h": (hidden,), "3h": (3 * hidden,), "i": (inter,), "hh": (hidden, hidden), "3hh": (3 * hidden, hidden),
               "ih": (inter, hidden), "hi": (hidden, inter)}
        for l in range(self.layers):
            for name, shape in _LAYER:
                take(f"backbone.layers.{l}.{name}", dim[shape])
        take("backbone.ln1.weight", (hidden,))
        take("backbone.ln1.bias", (hidden,))

        # decode_head.{deconv,conv}_layers.{index}.*, in index order: a 4-d weight opens a stage, a 1-d weight behind it
        # is its InstanceNorm's gain
        def stages(prefix, transposed):
            groups = {}
            for key in sd:
                m = re.fullmatch(re.escape(prefix) + r"(\d+)\.(.+)", key)
                if m:
                    groups.setdefault(int(m.group(1)), {})[m.group(2)] = key
            widths, affine, names = [], [], []
            cin = widths_in[0]
            for idx in sorted(groups):
                g = groups[idx]
                for name, key in g.items():
                    if name not in ("weight", "bias"):
                        raise _refuse(key, "not a tensor of a convolution or an InstanceNorm without running statistics")
                w = sd[g["weight"]] if "weight" in g else None
                if w is None:
                    raise ValueError(f"sapiens weights: the state dict misses {prefix}{idx}.weight")
                if w.dim() == 4:
                    k = 4 if transposed else 1
                    if tuple(w.shape[2:]) != (k, k):
                        raise _refuse(g["weight"], f"a kernel of {tuple(w.shape[2:])}, only {k} x {k} is supported")
                    ci, co = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
                    if ci != cin:
                        raise _refuse(g["weight"], f"takes {ci} channels, the stage in front of it gives {cin}")
                    if co % 32 or not 32 <= co <= lim["INSTAG_SAPIENS_MAX_WIDTH"]:
                        raise _refuse(g["weight"], f"a width of {co}: a multiple of 32, at most {lim['INSTAG_SAPIENS_MAX_WIDTH']}")
                    take(g["weight"])
                    if transposed and "bias" in g:
                        raise _refuse(g["bias"], "the transposed convolutions have no bias")
                    if not transposed:
                        take(prefix + f"{idx}.bias", (co,))
                    widths.append(int(co))
                    affine.append(False)
                    names.append(prefix + str(idx))
                    cin = int(co)
                elif w.dim() == 1 and widths and not affine[-1]:
                    take(g["weight"], (cin,))
                    take(prefix + f"{idx}.bias", (cin,))
                    affine[-1] = prefix + str(idx)
                else:
                    raise _refuse(g["weight"], f"has shape {tuple(w.shape)}: neither a convolution nor the norm behind one")
            if len(widths) > lim["INSTAG_SAPIENS_MAX_HEAD"]:
                raise ValueError(f"sapiens weights: {prefix}*: {len(widths)} stages, at most {lim['INSTAG_SAPIENS_MAX_HEAD']}")
            widths_in[0] = cin
            return widths, affine, names

        widths_in = [hidden]
        self.deconv, self.deconv_affine, self._deconv_keys = stages("decode_head.deconv_layers.", True)
        if not self.deconv:
            raise ValueError("sapiens weights: the state dict misses decode_head.deconv_layers.*")
        self.conv, self.conv_affine, self._conv_keys = stages("decode_head.conv_layers.", False)
        seg = take("decode_head.conv_seg.weight", dims=4)
        if tuple(seg.shape[1:]) != (widths_in[0], 1, 1) or seg.shape[0] not in (1, 3):
            raise _refuse("decode_head.conv_seg.weight", f"has shape {tuple(seg.shape)}, expected (3 or 1, {widths_in[0]}, 1, 1)")
        self.out_channels = int(seg.shape[0])
        take("decode_head.conv_seg.bias", (self.out_channels,))
        return keep

    @property
    def kind(self) -> str:
        return "normal" if self.out_channels == 3 else "depth"

    @property
    def map_size(self):
        """(h, w) of the network's output map."""
        return self.grid[0] << len(self.deconv), self.grid[1] << len(self.deconv)

    @classmethod
    def from_state_dict(cls, sd, grid=GRID, heads=None):
        """``sd``: the release's keys, or an mmengine checkpoint ``{"meta": ..., "state_dict": ...}`` itself.  Keys outside
        the backbone and the head's three parts are ignored; a missing key, an unknown tensor under ``backbone.layers``, a
        kernel, a width, a ``pos_embed`` or a ``heads`` the kernels are not written for raise ValueError naming it."""
        if "state_dict" in sd and not torch.is_tensor(sd["state_dict"]):
            sd = sd["state_dict"]
        return cls(dict(sd), grid, heads)

    @classmethod
    def load(cls, path, grid=GRID):
        """``path``: a ``*_torchscript.pt2`` archive (read through ``torch.jit.load``), or a file ``torch.load`` reads: a
        plain state dict or an mmengine checkpoint."""
        path = str(path)
        try:
            sd = torch.jit.load(path, map_location="cpu").state_dict()
        except RuntimeError:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        return cls.from_state_dict(sd, grid)

    @classmethod
    def random(cls, hidden=1024, layers=24, intermediate=4096, grid=GRID, deconv=(512, 256, 128, 64), conv=(64, 64),
               kind="normal", affine=False, seed=0, head_gain=1.0):
        """Seeded stand-ins under the release's keys (tests, benches).  Matrices are drawn with a gain over
        1 / sqrt(fan-in): 1.5 for q and k so that the attention is far from uniform, 1.4 in front of the GELU, ``head_gain``
        in the head, 1 elsewhere; LayerNorm and InstanceNorm gains are 1 +- 0.2, every bias, shift and position 0.1 wide
        (positions 0.5)."""
        g = torch.Generator().manual_seed(seed)
        sd = {}

        def mat(*shape, fan_in, gain=1.0):
            return torch.randn(*shape, generator=g) * (gain / fan_in ** 0.5)

        def vec(n, centre=0.0, width=0.1):
            return centre + width * torch.randn(n, generator=g)

        sd[_PATCH + "weight"], sd[_PATCH + "bias"] = mat(hidden, 3, PATCH, PATCH, fan_in=PATCH_K), vec(hidden)
        sd["backbone.pos_embed"] = 0.5 * torch.randn(1, grid[0] * grid[1], hidden, generator=g)
        for l in range(layers):
            p = f"backbone.layers.{l}."
            qkv = mat(3 * hidden, hidden, fan_in=hidden)
            qkv[:2 * hidden] *= 1.5
            sd.update({p + "ln1.weight": vec(hidden, 1.0, 0.2), p + "ln1.bias": vec(hidden), p + "attn.qkv.weight": qkv,
                       p + "attn.qkv.bias": vec(3 * hidden), p + "attn.proj.weight": mat(hidden, hidden, fan_in=hidden),
                       p + "attn.proj.bias": vec(hidden), p + "ln2.weight": vec(hidden, 1.0, 0.2), p + "ln2.bias": vec(hidden),
                       p + "ffn.layers.0.0.weight": mat(intermediate, hidden, fan_in=hidden, gain=1.4),
                       p + "ffn.layers.0.0.bias": vec(intermediate),
                       p + "ffn.layers.1.weight": mat(hidden, intermediate, fan_in=intermediate),
                       p + "ffn.layers.1.bias": vec(hidden)})
        sd["backbone.ln1.weight"], sd["backbone.ln1.bias"] = vec(hidden, 1.0, 0.2), vec(hidden)
        cin = hidden
        for j, c in enumerate(deconv):
            sd[f"decode_head.deconv_layers.{3 * j}.weight"] = mat(cin, c, 4, 4, fan_in=4 * cin, gain=head_gain)
            if affine:
                sd[f"decode_head.deconv_layers.{3 * j + 1}.weight"] = vec(c, 1.0, 0.2)
                sd[f"decode_head.deconv_layers.{3 * j + 1}.bias"] = vec(c)
            cin = c
        for j, c in enumerate(conv):
            sd[f"decode_head.conv_layers.{3 * j}.weight"] = mat(c, cin, 1, 1, fan_in=cin, gain=head_gain)
            sd[f"decode_head.conv_layers.{3 * j}.bias"] = vec(c)
            if affine:
                sd[f"decode_head.conv_layers.{3 * j + 1}.weight"] = vec(c, 1.0, 0.2)
                sd[f"decode_head.conv_layers.{3 * j + 1}.bias"] = vec(c)
            cin = c
        sd["decode_head.conv_seg.weight"] = mat(KINDS[kind], cin, 1, 1, fan_in=cin, gain=head_gain)
        sd["decode_head.conv_seg.bias"] = vec(KINDS[kind])
        return cls(sd, grid)

    def state_dict(self) -> dict:
        """The release's keys -> clones of the tensors."""
        return {k: t.clone() for k, t in self.tensors.items()}

    def to(self, device=None, dtype=None) -> dict:
        """key -> tensor of ``device`` / ``dtype`` for the torch statement; the last conversion is kept."""
        key = (torch.device(device) if device is not None else None, dtype)
        if self._converted[0] != key:
            self._converted = (key, {k: t.to(device=device, dtype=dtype) for k, t in self.tensors.items()})
        return self._converted[1]

    def head_stages(self):
        """[(kind, weight key, bias key or None, norm prefix or None)] of the head, in order."""
        out = [("deconv", k + ".weight", None, a or None) for k, a in zip(self._deconv_keys, self.deconv_affine)]
        return out + [("conv", k + ".weight", k + ".bias", a or None) for k, a in zip(self._conv_keys, self.conv_affine)]

    def fill_dims(self, s):
        """The dimensions of struct instag_sapiens_weights ``s`` (what the workspace's size depends on)."""
        s.hidden, s.heads, s.intermediate, s.layers = self.hidden, self.heads, self.intermediate, self.layers
        s.in_h, s.in_w = self.in_size
        s.n_deconv, s.n_conv, s.out_channels = len(self.deconv), len(self.conv), self.out_channels
        for j, c in enumerate(self.deconv):
            s.deconv_c[j] = c
        for j, c in enumerate(self.conv):
            s.conv_c[j] = c
        for c in range(3):
            s.mean[c], s.std[c] = MEAN[c], STD[c]
        return s

    def device_pack(self, device):
        """-> (struct instag_sapiens_weights, the device tensors it points to), every matrix as csrc/sapiens.hip reads it
        (include/instag_sapiens.h): [K][N]; a transposed convolution as its four phases' tap matrices; ``conv_seg`` with
        its 3 or 1 columns padded to 4."""
        from . import _lib
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key in self._packs:
            return self._packs[key]
        t, keep = self.tensors, []

        def put(x):
            x = x.to(dtype=torch.float32).contiguous().to(device)
            keep.append(x)
            return x.data_ptr()

        s = self.fill_dims(_lib.SapiensStruct())
        s.patch_w, s.patch_b = put(t[_PATCH + "weight"].reshape(self.hidden, PATCH_K).t()), put(t[_PATCH + "bias"])
        s.pos_embed = put(t["backbone.pos_embed"][0])
        s.enc_ln_g, s.enc_ln_b = put(t["backbone.ln1.weight"]), put(t["backbone.ln1.bias"])
        s.zeros = put(torch.zeros(_lib.SAPIENS["INSTAG_SAPIENS_MAX_WIDTH"]))
        for l in range(self.layers):
            p = f"backbone.layers.{l}."
            s.ln1_g[l], s.ln1_b[l] = put(t[p + "ln1.weight"]), put(t[p + "ln1.bias"])
            s.qkv_w[l], s.qkv_b[l] = put(t[p + "attn.qkv.weight"].t()), put(t[p + "attn.qkv.bias"])
            s.out_w[l], s.out_b[l] = put(t[p + "attn.proj.weight"].t()), put(t[p + "attn.proj.bias"])
            s.ln2_g[l], s.ln2_b[l] = put(t[p + "ln2.weight"]), put(t[p + "ln2.bias"])
            s.ff1_w[l], s.ff1_b[l] = put(t[p + "ffn.layers.0.0.weight"].t()), put(t[p + "ffn.layers.0.0.bias"])
            s.ff2_w[l], s.ff2_b[l] = put(t[p + "ffn.layers.1.weight"].t()), put(t[p + "ffn.layers.1.bias"])
        jd = jc = 0
        for kind, wk, bk, norm in self.head_stages():
            g, b = (put(t[norm + ".weight"]), put(t[norm + ".bias"])) if norm else (None, None)
            if kind == "deconv":
                s.deconv_w[jd], s.deconv_g[jd], s.deconv_b[jd] = put(pack_deconv(t[wk])), g, b
                jd += 1
            else:
                s.conv_w[jc], s.conv_bias[jc] = put(t[wk][:, :, 0, 0].t()), put(t[bk])
                s.conv_g[jc], s.conv_beta[jc] = g, b
                jc += 1
        seg = torch.zeros(t["decode_head.conv_seg.weight"].shape[1], RAW_C)
        seg[:, :self.out_channels] = t["decode_head.conv_seg.weight"][:, :, 0, 0].t()
        bias = torch.zeros(RAW_C)
        bias[:self.out_channels] = t["decode_head.conv_seg.bias"]
        s.seg_w, s.seg_b = put(seg), put(bias)
        self._packs[key] = (s, keep)
        return self._packs[key]


def pack_deconv(weight: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(4, 2, 1)'s weight [cin, cout, 4, 4] -> [py][px][v][(u, cin)][cout] = W[cin][cout][3 - py - 2 v]
    [3 - px - 2 u]: per output phase (py, px) and vertical tap v the matrix of the horizontal tap pair u = 0, 1."""
    cin, cout = weight.shape[:2]
    out = weight.new_empty(2, 2, 2, 2, cin, cout)
    for py in range(2):
        for px in range(2):
            for v in range(2):
                for u in range(2):
                    out[py, px, v, u] = weight[:, :, 3 - py - 2 * v, 3 - px - 2 * u]
    return out.reshape(2, 2, 2, 2 * cin, cout).contiguous()


# ---- plain-torch statements --------------------------------------------------------------------------------------------
def _resize_taps(S: int, D: int, device):
    """Per destination pixel of an axis resized from S to D: (first index, second index, weight of the second in 1/2048).
    The pixel's centre (d + 1/2) S / D - 1/2 as the exact fraction num / (2 D); its floor is the first index, the
    remainder in 1/2048 rounded half up the weight; below 0 and from S - 1 on the index is clamped and the weight 0."""
    d = torch.arange(D, dtype=torch.int64, device=device)
    num, den = (2 * d + 1) * S - D, 2 * D
    s = torch.div(num, den, rounding_mode="floor")
    w1 = torch.div((num - s * den) * 2048 + D, den, rounding_mode="floor")
    edge = (num < 0) | (s >= S - 1)
    i0 = torch.where(num < 0, torch.zeros_like(s), torch.where(s >= S - 1, torch.full_like(s, S - 1), s))
    return i0, torch.where(edge, i0, s + 1), torch.where(edge, torch.zeros_like(w1), w1)


def resize_u8_torch(frames_u8, size):
    """uint8 [B,H,W,3] -> uint8 [B,h,w,3], ``size`` = (h, w): this project's rule for the bilinear resize of an 8-bit image.
    Half-pixel centres, clamped indices, per-axis weights rounded to 1/2048 (``_resize_taps``), the weighted sum of the
    four pixels taken exactly on integers and rounded half up: (sum + 2^21) >> 22.  It follows what
    ``cv2.resize(INTER_LINEAR)`` is known to do on 8-bit images but is not checked against OpenCV, which is not a
    dependency; a frame of the network's own size passes unchanged."""
    x, H, W = check_frames("resize_u8", frames_u8, sides=False)
    h, w = int(size[0]), int(size[1])
    p = x.to(torch.int64)
    y0, y1, wy = _resize_taps(H, h, x.device)
    x0, x1, wx = _resize_taps(W, w, x.device)
    wx, wy = wx.view(1, 1, w, 1), wy.view(1, h, 1, 1)

    def across(rows):
        return (2048 - wx) * rows[:, :, x0] + wx * rows[:, :, x1]

    s = (2048 - wy) * across(p[:, y0]) + wy * across(p[:, y1])
    return ((s + (1 << 21)) >> 22).to(torch.uint8)


def patch_rows_torch(frames_u8, size, dtype=torch.float32):
    """uint8 [B,H,W,3] -> [B, T, 768] of ``dtype``: the frames resized to ``size``, normalised as (x - MEAN) / STD, padded
    with two zeros on every side (Conv2d's padding) and cut into 16 x 16 patches, row k = channel * 256 + ky * 16 + kx."""
    r = resize_u8_torch(frames_u8, size).permute(0, 3, 1, 2).to(dtype)
    mean = torch.tensor(MEAN, dtype=dtype, device=r.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype, device=r.device).view(1, 3, 1, 1)
    x = F.pad((r - mean) / std, (PATCH_PAD,) * 4)
    return F.unfold(x, PATCH, stride=PATCH).transpose(1, 2).contiguous()


def _tap(taps, name, v):
    if taps is not None:
        taps.append((name, v))
    return v


def vit_torch(weights: SapiensWeights, rows, taps=None):
    """Patch rows [B,T,768] -> features [B,T,hidden] in the rows' dtype on their device.  ``taps``: a list that receives
    (name, tensor) of every stage."""
    w = weights.to(rows.device, rows.dtype)
    hid, heads = weights.hidden, weights.heads
    B, T, _ = rows.shape
    h = F.linear(rows, w[_PATCH + "weight"].reshape(hid, PATCH_K), w[_PATCH + "bias"]) + w["backbone.pos_embed"]
    _tap(taps, "tokens", h)
    for l in range(weights.layers):
        p = f"backbone.layers.{l}."
        y = F.layer_norm(h, (hid,), w[p + "ln1.weight"], w[p + "ln1.bias"], VIT_LN_EPS)
        q, k, v = (t.view(B, T, heads, HEAD_DIM).transpose(1, 2)
                   for t in F.linear(y, w[p + "attn.qkv.weight"], w[p + "attn.qkv.bias"]).chunk(3, dim=2))
        probs = torch.softmax((q * HEAD_DIM ** -0.5) @ k.transpose(2, 3), dim=-1)
        ctx = (probs @ v).transpose(1, 2).reshape(B, T, hid)
        h = _tap(taps, f"layer{l}.attention", h + F.linear(ctx, w[p + "attn.proj.weight"], w[p + "attn.proj.bias"]))
        y = F.layer_norm(h, (hid,), w[p + "ln2.weight"], w[p + "ln2.bias"], VIT_LN_EPS)
        y = F.gelu(F.linear(y, w[p + "ffn.layers.0.0.weight"], w[p + "ffn.layers.0.0.bias"]))
        h = _tap(taps, f"layer{l}.feed_forward", h + F.linear(y, w[p + "ffn.layers.1.weight"], w[p + "ffn.layers.1.bias"]))
    return _tap(taps, "features", F.layer_norm(h, (hid,), w["backbone.ln1.weight"], w["backbone.ln1.bias"], VIT_LN_EPS))


def head_torch(weights: SapiensWeights, features, taps=None):
    """Features [B,T,hidden] -> raw [B,C,h,w]: the map [B,hidden,grid], the transposed convolutions, the 1 x 1
    convolutions (each with InstanceNorm and SiLU) and ``conv_seg``."""
    w = weights.to(features.device, features.dtype)
    B = features.shape[0]
    x = features.view(B, weights.grid[0], weights.grid[1], weights.hidden).permute(0, 3, 1, 2)
    count = {"deconv": 0, "conv": 0}
    for kind, wk, bk, norm in weights.head_stages():
        if kind == "deconv":
            x = F.conv_transpose2d(x, w[wk], stride=2, padding=1)
        else:
            x = F.conv2d(x, w[wk], w[bk])
        x = F.instance_norm(x, weight=w[norm + ".weight"] if norm else None, bias=w[norm + ".bias"] if norm else None,
                            eps=IN_EPS)
        x = _tap(taps, f"{kind}{count[kind]}", F.silu(x))
        count[kind] += 1
    return _tap(taps, "raw", F.conv2d(x, w["decode_head.conv_seg.weight"], w["decode_head.conv_seg.bias"]))


def _bilinear_taps(S: int, D: int, dtype, device):
    """``F.interpolate(mode="bilinear", align_corners=False)``'s rule per destination pixel: the source position
    max((d + 1/2) S / D - 1/2, 0), its floor and the next index (clamped), and the weight of the second."""
    src = ((torch.arange(D, dtype=dtype, device=device) + 0.5) * (torch.tensor(S, dtype=dtype) / D).to(device) - 0.5).clamp(min=0)
    i0 = src.floor().to(torch.int64).clamp(max=S - 1)
    return i0, (i0 + 1).clamp(max=S - 1), src - i0.to(dtype)


def finish_torch(raw, H: int, W: int):
    """raw [B,C,h,w] -> [B,3,H,W] (C = 3: n / (|n| + 1e-5) per pixel) or [B,H,W] (C = 1): bilinear to H x W without
    antialiasing, written out as the four reads and two weights per pixel."""
    B, Cn, h, w = raw.shape
    y0, y1, ly = _bilinear_taps(h, H, raw.dtype, raw.device)
    x0, x1, lx = _bilinear_taps(w, W, raw.dtype, raw.device)
    ly, lx = ly.view(1, 1, H, 1), lx.view(1, 1, 1, W)

    def across(rows):
        return (1 - lx) * rows[:, :, :, x0] + lx * rows[:, :, :, x1]

    out = (1 - ly) * across(raw[:, :, y0]) + ly * across(raw[:, :, y1])
    if Cn == 3:
        return out / (out.pow(2).sum(dim=1, keepdim=True).sqrt() + NORMAL_EPS)
    return out[:, 0]


def _check_kind(weights, kind):
    if kind is not None and kind not in KINDS:
        raise ValueError(f"sapiens: kind 'normal' or 'depth', got {kind!r}")
    if kind is not None and KINDS[kind] != weights.out_channels:
        raise ValueError(f"sapiens: kind {kind!r} has {KINDS[kind]} channels, the weights' conv_seg gives "
                         f"{weights.out_channels}")


def sapiens_torch(weights: SapiensWeights, frames_u8, kind=None, dtype=torch.float32, taps=None):
    """The whole chain on uint8 frames [B,H,W,3] in ``dtype`` on the frames' device -> [B,3,H,W] (normal) or [B,H,W]
    (depth).  ``kind``: checked against the weights where given.  ``taps``: a list that receives (name, tensor) of every
    stage, "out" the last."""
    _check_kind(weights, kind)
    x, H, W = check_frames("sapiens", frames_u8, sides=False)
    rows = patch_rows_torch(x, weights.in_size, dtype)
    raw = head_torch(weights, vit_torch(weights, rows, taps), taps)
    return _tap(taps, "out", finish_torch(raw, H, W))


def macs_per_frame(weights: SapiensWeights, H: int = 0, W: int = 0) -> int:
    """Multiply-accumulates of one frame from the layer table (the products only; the resizes to and from H x W have
    none): the projection, per layer 4 h^2 + 2 h i per token and 2 T h for its scores and its context, the head's
    transposed convolutions (4 taps per output pixel), 1 x 1 convolutions and ``conv_seg``."""
    T, hid = weights.grid[0] * weights.grid[1], weights.hidden
    total = T * PATCH_K * hid + weights.layers * T * (4 * hid * hid + 2 * hid * weights.intermediate + 2 * T * hid)
    px, cin = T, hid
    for c in weights.deconv:
        px *= 4
        total += px * 4 * cin * c
        cin = c
    for c in weights.conv:
        total += px * cin * c
        cin = c
    return total + px * cin * weights.out_channels


# ---- HIP operator -------------------------------------------------------------------------------------------------------
class GeometryNet(FrameOperator):
    """One Sapiens network over uint8 frames [N,H,W,3] on ``device`` (convnet.FrameOperator), on torch's current stream;
    inference only.  On the GPU the frames go through csrc/sapiens.hip in chunks of at most ``max_batch`` with the one
    kept workspace; on a CPU device every output is the torch statement.  The workspace is 16.5 MB a frame for the
    features plus the larger of the backbone's 135 MB and the head's two largest maps: with a head of
    (512, 256, 128, 64) + (64, 64) 434 MB a frame at 1024 x 768, so two frames a chunk.  The default ``max_batch`` is the largest whose
    workspace stays within 1 GiB, or 1 where a single frame already exceeds that (wider heads do).  ``tile``: 0, or
    1..3 to pin the GEMM tile (tests)."""

    NAME = "sapiens"

    def __init__(self, weights: SapiensWeights, device="cuda", kind="normal", max_batch=None, tile: int = 0):
        if kind not in KINDS:
            raise ValueError(f"GeometryNet: kind 'normal' or 'depth', got {kind!r}")
        _check_kind(weights, kind)
        self.kind, self.tile = kind, int(tile)
        super().__init__(weights, device, max_batch)
        if self.max_batch is None:
            self.max_batch = self.default_max_batch(weights)

    @staticmethod
    def workspace_bytes(weights: SapiensWeights, batch: int = 1) -> int:
        """Bytes of the workspace for ``batch`` frames (from the dimensions alone: no device copy, no GPU)."""
        from . import _lib
        s = weights.fill_dims(_lib.SapiensStruct())
        return _lib.workspace_bytes(_lib.lib().instag_sapiens_workspace_bytes(C.byref(s), int(batch)))

    @classmethod
    def default_max_batch(cls, weights: SapiensWeights) -> int:
        return max(1, min(4096, (WORKSPACE_LIMIT - 4096) // cls.workspace_bytes(weights, 1)))

    def _frames(self, frames_u8):
        x, H, W = check_frames(self.NAME, frames_u8, sides=False)
        return x.to(self.device).contiguous(), H, W

    def _torch(self, x, taps):
        """The CPU path, ``max_batch`` frames at a time -> the statement's taps of all frames, by name."""
        stages = {}
        for s in range(0, x.shape[0], self.max_batch):
            one = []
            sapiens_torch(self.weights, x[s:s + self.max_batch], self.kind, taps=one)
            for name, v in one:
                stages.setdefault(name, []).append(v)
        stages = {name: torch.cat(v) for name, v in stages.items()}
        if taps is not None:
            taps += [(name, v) for name, v in stages.items() if name != "out"]
        return stages

    @torch.no_grad()
    def _run(self, frames_u8, mode=0, taps=None):
        """-> (out [N,C,H,W], raw [N,h,w,4], features [N,T,hidden]) of the GPU entry point; ``mode`` 1: features only."""
        from . import _lib
        x, H, W = self._frames(frames_u8)
        wt, B = self.weights, int(x.shape[0])
        h, w = wt.map_size
        T = wt.grid[0] * wt.grid[1]
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)      # noqa: E731
        out = new(B, wt.out_channels, H, W) if mode == 0 else None
        raw = new(B, h, w, RAW_C) if mode == 0 else None
        feats = new(B, T, wt.hidden)
        if B == 0:
            return out, raw, feats
        ws = C.byref(self._struct)
        nbytes = _lib.workspace_bytes(self._L.instag_sapiens_workspace_bytes(ws, min(B, self.max_batch)))
        flat = None if taps is None else self._taps_buffer(self._L.instag_sapiens_taps_floats(ws, B), B)
        part = lambda t, c: None if t is None else _lib.ptr(t[c])                                # noqa: E731
        self._each_chunk(B, nbytes, lambda c, m, p, size: self._L.instag_sapiens_forward(
            ws, _lib.ptr(x[c]), m, H, W, mode, part(out, c), part(raw, c), _lib.ptr(feats[c]), p, size, self.tile,
            _lib.ptr(flat), _lib.current_stream()), "sapiens_forward")
        if taps is not None:
            stages = [("tokens", (B, T, wt.hidden))]
            stages += [(f"layer{l}.{part}", (B, T, wt.hidden)) for l in range(wt.layers) for part in ("attention", "feed_forward")]
            stages += [("features", (B, T, wt.hidden))]
            hh, ww = wt.grid
            for j, c in enumerate(wt.deconv):
                hh, ww = 2 * hh, 2 * ww
                stages.append((f"deconv{j}", (B, hh, ww, c)))
            stages += [(f"conv{j}", (B, h, w, c)) for j, c in enumerate(wt.conv)] + [("raw", (B, h, w, RAW_C))]
            for name, v in self._cut(flat, stages):
                if v.dim() == 4:
                    v = (v[..., :wt.out_channels] if name == "raw" else v).permute(0, 3, 1, 2)
                taps.append((name, v))
        return out, raw, feats

    def _finished(self, out):
        return out if self.kind == "normal" else out[:, 0]

    @torch.no_grad()
    def predict(self, frames_u8, taps=None):
        """uint8 [N,H,W,3] -> fp32 [N,3,H,W] (normal) or [N,H,W] (depth) at the frames' own size: what
        ``FrameStore.append(normal=, depth=)`` takes.  ``taps``: a list that receives (name, tensor) of every stage as
        ``sapiens_torch``'s does, but for the output (debug: one chunk only, N <= max_batch)."""
        if self.device.type != "cuda":
            return self._torch(self._frames(frames_u8)[0], taps)["out"]
        return self._finished(self._run(frames_u8, 0, taps)[0])

    @torch.no_grad()
    def raw(self, frames_u8):
        """-> [N,C,h,w]: the network's output map in front of the resize."""
        if self.device.type != "cuda":
            return self._torch(self._frames(frames_u8)[0], None)["raw"]
        return self._run(frames_u8)[1][..., :self.weights.out_channels].permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def features(self, frames_u8):
        """-> [N, grid[0] grid[1], hidden]: the backbone's output, token-major (the backbone alone runs)."""
        if self.device.type != "cuda":
            return self._torch(self._frames(frames_u8)[0], None)["features"]
        return self._run(frames_u8, 1)[2]

    @torch.no_grad()
    def head(self, features, H: int, W: int):
        """Features [N,T,hidden] on the GPU -> the finished output at H x W (the head and the finish alone: benches)."""
        from . import _lib
        wt = self.weights
        f = features.to(device=self.device, dtype=torch.float32).contiguous()
        B = int(f.shape[0])
        if self.device.type != "cuda":
            return finish_torch(head_torch(wt, f), H, W)
        if tuple(f.shape[1:]) != (wt.grid[0] * wt.grid[1], wt.hidden):
            raise ValueError(f"GeometryNet.head: features [N, {wt.grid[0] * wt.grid[1]}, {wt.hidden}], got {tuple(f.shape)}")
        out = torch.empty(B, wt.out_channels, H, W, dtype=torch.float32, device=self.device)
        ws = C.byref(self._struct)
        nbytes = _lib.workspace_bytes(self._L.instag_sapiens_workspace_bytes(ws, max(1, min(B, self.max_batch))))
        self._each_chunk(B, nbytes, lambda c, m, p, size: self._L.instag_sapiens_forward(
            ws, None, m, H, W, 2, _lib.ptr(out[c]), None, _lib.ptr(f[c]), p, size, self.tile, None,
            _lib.current_stream()), "sapiens_forward")
        return self._finished(out)


# ---- the stages alone (tests, benches) ------------------------------------------------------------------------------------
def _gpu_fp32(who, t, dims):
    if not torch.is_tensor(t) or t.dim() != dims or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"{who}: a fp32 tensor of {dims} dimensions on the GPU")
    return t.contiguous()


def patch_rows(frames_u8, size) -> torch.Tensor:
    """``patch_rows_torch`` in fp32 through the kernel: uint8 [B,H,W,3] on the GPU -> [B,T,768]."""
    from . import _lib
    x, H, W = check_frames("patch_rows", frames_u8, sides=False)
    if not x.is_cuda:
        raise ValueError("patch_rows: frames on the GPU")
    x, (h, w) = x.contiguous(), (int(size[0]), int(size[1]))
    T = ((h - 12) // 16 + 1) * ((w - 12) // 16 + 1) if min(h, w) >= 12 else 0
    rows = torch.empty(x.shape[0], max(T, 0), PATCH_K, dtype=torch.float32, device=x.device)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    with torch.cuda.device(x.device):
        _lib.check_arg(_lib.lib().instag_sapiens_patch_rows(_lib.ptr(x), x.shape[0], H, W, h, w, mean, std, _lib.ptr(rows),
                                                            _lib.current_stream()), "sapiens_patch_rows")
    return rows


def attention(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """The backbone's attention alone: qkv [B,T,3 * 64 heads] (q | k | v), fp32 on the GPU -> ctx [B,T,64 heads]."""
    from . import _lib
    qkv = _gpu_fp32("attention", qkv, 3)
    B, T, _ = qkv.shape
    if qkv.shape[2] != 3 * HEAD_DIM * int(heads):
        raise ValueError(f"attention: qkv [B, T, {3 * HEAD_DIM * int(heads)}], got {tuple(qkv.shape)}")
    ctx = torch.empty(B, T, HEAD_DIM * int(heads), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        _lib.check_arg(_lib.lib().instag_sapiens_attention(_lib.ptr(qkv), _lib.ptr(ctx), B, T, int(heads),
                                                           _lib.current_stream()), "sapiens_attention")
    return ctx


def deconv(x: torch.Tensor, weight: torch.Tensor, tile: int = 0) -> torch.Tensor:
    """ConvTranspose2d(4, 2, 1) alone: x [B,h,w,cin] (NHWC) and the module's weight [cin,cout,4,4], fp32 on the GPU ->
    [B,2h,2w,cout]."""
    from . import _lib
    x, weight = _gpu_fp32("deconv", x, 4), _gpu_fp32("deconv", weight, 4)
    B, h, w, cin = x.shape
    if tuple(weight.shape) != (cin, weight.shape[1], 4, 4):
        raise ValueError(f"deconv: weight [{cin}, cout, 4, 4], got {tuple(weight.shape)}")
    cout, L = int(weight.shape[1]), _lib.lib()
    packed = pack_deconv(weight)
    y = torch.empty(B, 2 * h, 2 * w, cout, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws = torch.empty(_lib.workspace_bytes(L.instag_sapiens_deconv_workspace_bytes(B, h, w, cin, cout)), dtype=torch.uint8,
                         device=x.device)
        _lib.check_arg(L.instag_sapiens_deconv(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(y), B, h, w, cin, cout, _lib.ptr(ws),
                                               ws.numel(), int(tile), _lib.current_stream()), "sapiens_deconv")
    return y


def instance_norm_silu(x: torch.Tensor, gamma=None, beta=None) -> torch.Tensor:
    """InstanceNorm (biased variance, eps 1e-5) + SiLU alone: x [B,h,w,C] (NHWC), fp32 on the GPU -> a new tensor."""
    from . import _lib
    y = _gpu_fp32("instance_norm_silu", x, 4).clone()
    B, h, w, Cn = y.shape
    L = _lib.lib()
    with torch.cuda.device(y.device):
        ws = torch.empty(_lib.workspace_bytes(L.instag_sapiens_norm_workspace_bytes(B, h, w, Cn)), dtype=torch.uint8,
                         device=y.device)
        _lib.check_arg(L.instag_sapiens_instance_norm_silu(_lib.ptr(y), B, h, w, Cn, _lib.ptr(gamma), _lib.ptr(beta),
                                                           _lib.ptr(ws), ws.numel(), _lib.current_stream()),
                       "sapiens_instance_norm_silu")
    return y


def finish(raw: torch.Tensor, channels: int, H: int, W: int) -> torch.Tensor:
    """The finish alone: raw [B,h,w,4] (NHWC, ``channels`` of them used), fp32 on the GPU -> [B,channels,H,W]."""
    from . import _lib
    raw = _gpu_fp32("finish", raw, 4)
    B, h, w, c4 = raw.shape
    if c4 != RAW_C:
        raise ValueError(f"finish: raw [B, h, w, {RAW_C}], got {tuple(raw.shape)}")
    out = torch.empty(B, int(channels), int(H), int(W), dtype=torch.float32, device=raw.device)
    with torch.cuda.device(raw.device):
        _lib.check_arg(_lib.lib().instag_sapiens_finish(_lib.ptr(raw), B, h, w, int(channels), int(H), int(W), _lib.ptr(out),
                                                        _lib.current_stream()), "sapiens_finish")
    return out


# ---- a directory ----------------------------------------------------------------------------------------------------------
def list_gt_frames(path, limit=None):
    """Numeric stems of gt_imgs/*.jpg, ascending (the reference's ``sort -V``), the first ``limit``."""
    stems = [os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(path, "gt_imgs", "*.jpg"))]
    ids = sorted(int(s) for s in stems if s.isdigit())
    return ids if limit is None else ids[:int(limit)]


def geometry_identity(path, normal_w, depth_w, device, limit=500, model_name="sapiens_0.3b", write=True, batch: int = 8):
    """The geometry priors of the identity directory ``path``: gt_imgs/<i>.jpg in ascending numeric order, the first
    ``limit``, through the normal network (``normal_w``) and the depth network (``depth_w``); either may be None, to run
    one network only.  ``write``: saves sapiens/normal/<model_name>/<i>.npy (fp32 [H,W,3]) and
    sapiens/depth/<model_name>/<i>.npy (fp32 [H,W]) exactly as ``dataset.read_identity`` reads them.
    -> (ids [N] int64 array, normal [N,3,H,W] or None, depth [N,H,W] or None) on ``device``: ``read_identity(...,
    priors=dict(ids=, normal=, depth=))`` takes them in place of the files."""
    from PIL import Image
    device = torch.device(device)
    ids = list_gt_frames(path, limit)
    nets = {kind: GeometryNet(w, device, kind) for kind, w in (("normal", normal_w), ("depth", depth_w)) if w is not None}
    out = {kind: [] for kind in nets}
    dirs = {kind: os.path.join(path, "sapiens", kind, model_name) for kind in nets}
    if write:
        for d in dirs.values():
            os.makedirs(d, exist_ok=True)
    size = None
    for s in range(0, len(ids), int(batch)):
        frames = []
        for i in ids[s:s + int(batch)]:
            img = Image.open(os.path.join(path, "gt_imgs", f"{i}.jpg"))
            if size is None:
                size = img.size
            elif img.size != size:
                raise ValueError(f"{path}: gt_imgs/{i}.jpg is {img.size}, the first frame {size}")
            frames.append(np.array(img.convert("RGB")))
        frames = torch.from_numpy(np.stack(frames))
        for kind, net in nets.items():
            pred = net.predict(frames)
            out[kind].append(pred)
            if write:
                host = pred.cpu().numpy()
                for i, one in zip(ids[s:s + int(batch)], host):
                    np.save(os.path.join(dirs[kind], f"{i}.npy"),
                            np.ascontiguousarray(one.transpose(1, 2, 0) if kind == "normal" else one))
    done = {kind: torch.cat(v) if v else None for kind, v in out.items()}
    return np.asarray(ids, dtype=np.int64), done.get("normal"), done.get("depth")
