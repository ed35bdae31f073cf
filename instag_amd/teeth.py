"""Teeth segmentation on the device: from ``ori_imgs/<i>.jpg`` to ``teeth_mask/<i>.npy`` (csrc/teeth.hip).

The reference makes the teeth masks with data_utils/easyportrait/create_teeth_mask.py: mmsegmentation's
``EncoderDecoder`` of local_configs/easyportrait_experiments_v2/fpn-fp/fpn-fp.py -- a ``ResNetV1c`` of depth 50
(mmseg/models/backbones/resnet.py, models/utils/res_layer.py), an ``FPN`` neck (models/necks/fpn.py) and an ``FPNHead``
(models/decode_heads/fpn_head.py) -- with the weights ``fpn-fp-512.pth``, in eval mode on the frame at its own size
(the test pipeline normalises and does not resize), and saves ``label == 7`` (teeth) as ``np.bool_ [H,W]``.  Here:

    w = FPNWeights.load("data_utils/easyportrait/fpn-fp-512.pth")  # the file a user of the reference already has
    teeth = teeth_identity(path, w, "cuda")                         # reads ori_imgs/*.jpg, writes teeth_mask/*.npy
    store.append(gt, torso, bc, parsing, teeth, ...)                # u8 [N,H,W] on the device, as it is

On the GPU the network, the bilinear upsample and the argmax run in csrc/teeth.hip (inference only, fp32, as the
reference runs it); ``fpn_torch``, ``upsample_torch``, ``labels_torch`` and ``teeth_torch`` are the plain-torch statement
of the same arithmetic (any dtype, CPU or GPU) that the tests compare against and a CPU device uses.  The project ships
no weights and fetches none.

The reference resizes the logits at stride 4 bilinearly (``align_corners=False``) to H x W, applies a softmax over the
classes and takes ``argmax`` (segmentors/encoder_decoder.py:71-80, 204-271).  The softmax is monotone: this project's
statement is the first-maximum argmax of the resized logits themselves.

Frames whose sides are not multiples of 32 (and at least 64) are not supported: a multiple of 32 makes every nearest
and bilinear x2 step of the network exact in its sizes.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import convnet
from .convnet import BN_EPS, first_argmax  # noqa: F401

SIZE = 512                                           # the size InsTaG's frames have
MEAN = (143.55267075, 132.96705975, 126.94924335)    # fpn-fp.py: img_norm_cfg, RGB, on the 0..255 scale
STD = (60.2625333, 60.32740275, 59.30988645)
TEETH = 7                                            # create_teeth_mask.py:30
MIN_CLASSES, MAX_CLASSES = 8, 32
STAGE_BLOCKS = (3, 4, 6, 3)
WORKSPACE_BUDGET = 1 << 30                           # bytes the default max_batch may ask for at 512 x 512
SEG = "decode_head.conv_seg"


def _layers():
    # (convolution, its BatchNorm or None, bias?, cin, cout, kernel, stride)
    s = "backbone.stem"
    out = [(f"{s}.0", f"{s}.1", False, 3, 32, 3, 2), (f"{s}.3", f"{s}.4", False, 32, 32, 3, 1),
           (f"{s}.6", f"{s}.7", False, 32, 64, 3, 1)]
    cin = 64
    for stage, blocks in enumerate(STAGE_BLOCKS, start=1):
        planes = 32 << stage
        for b in range(blocks):
            p = f"backbone.layer{stage}.{b}"
            stride = 2 if b == 0 and stage > 1 else 1
            out += [(f"{p}.conv1", f"{p}.bn1", False, cin, planes, 1, 1),
                    (f"{p}.conv2", f"{p}.bn2", False, planes, planes, 3, stride),
                    (f"{p}.conv3", f"{p}.bn3", False, planes, 4 * planes, 1, 1)]
            if b == 0:
                out.append((f"{p}.downsample.0", f"{p}.downsample.1", False, cin, 4 * planes, 1, stride))
            cin = 4 * planes
    out += [(f"neck.lateral_convs.{i}.conv", None, True, 256 << i, 256, 1, 1) for i in range(4)]
    out += [(f"neck.fpn_convs.{i}.conv", None, True, 256, 256, 3, 1) for i in range(4)]
    for i in range(4):
        for k in range(max(1, i)):
            h = f"decode_head.scale_heads.{i}.{2 * k}"
            out.append((f"{h}.conv", f"{h}.bn", False, 256 if k == 0 else 128, 128, 3, 1))
    out.append((SEG, None, True, 128, None, 1, 1))              # cout = C, read from the checkpoint
    return tuple(out)


# (convolution, its BatchNorm or None, has a bias, cin, cout, kernel, stride) in the order of struct instag_teeth_weights
LAYERS = _layers()
INDEX = {name: i for i, (name, *_) in enumerate(LAYERS)}


def macs_per_frame(H: int = SIZE, W: int = SIZE, classes: int = MIN_CLASSES) -> int:
    """Multiply-accumulates of the 71 convolutions of one H x W frame."""
    pix = lambda s: (H // s) * (W // s)
    total = 0
    for name, _, _, cin, cout, k, stride in LAYERS:
        cout = classes if cout is None else cout
        if name.startswith("backbone.stem"):
            out = pix(2)
        elif name.startswith("backbone.layer"):
            stage, b = int(name.split(".")[1][5:]), int(name.split(".")[2])
            s_out = 2 << stage
            # conv1 of a stage's first block still runs at the stage's input resolution
            out = pix(s_out // 2) if b == 0 and stage > 1 and name.endswith("conv1") else pix(s_out)
        elif name.startswith("neck."):
            out = pix(4 << int(name.split(".")[2]))
        elif name.startswith("decode_head.scale_heads"):
            i, k2 = int(name.split(".")[2]), int(name.split(".")[3])
            out = pix((4 << i) >> (k2 // 2))                     # every conv of a level runs behind k upsamples
        else:
            out = pix(4)
        total += cin * cout * k * k * out
    return total


# ---- weights ----------------------------------------------------------------------------------------------------------
class FPNWeights(convnet.ConvWeights):
    """The frozen parameters of the fpn-fp segmentor: per layer of ``LAYERS`` the convolution's weight, its bias where
    it has one (the neck and ``conv_seg``: a ConvModule has a bias exactly when it has no norm) and, where it has one,
    BatchNorm's gamma, beta, running mean and running variance (convnet.ConvWeights; ``from_state_dict`` takes the keys
    of fpn-fp-512.pth's state dict or the mmcv checkpoint itself).  ``classes`` is the number of rows of ``conv_seg``.
    On the device the first stem convolution's K = 27 is padded with zero rows to 32."""

    TABLE, LABEL, STRUCT, STEM_K = LAYERS, "FPN weights", "TeethWeights", 32

    def _prepare(self, layers):
        seg = layers[INDEX[SEG]]["weight"]
        if seg.dim() != 4 or not MIN_CLASSES <= int(seg.shape[0]) <= MAX_CLASSES:
            raise ValueError(f"FPN weights: {SEG}.weight has shape {tuple(seg.shape)}, expected (C, 128, 1, 1) with "
                             f"{MIN_CLASSES} <= C <= {MAX_CLASSES}")
        self.classes = int(seg.shape[0])

    @classmethod
    def random(cls, seed: int = 0, classes: int = MIN_CLASSES) -> "FPNWeights":
        """Seeded stand-ins with the scale of trained ones (tests, benches; convnet.draw_layer), so that the fold is
        exercised and about half of every stage's units are active.  ``conv3`` of every bottleneck is scaled by a
        further 1/2 so that the trunk's magnitude stays of order one through the sixteen blocks; the neck's
        convolutions, which no norm follows, by 0.7; every class row of ``conv_seg`` sums to zero over its inputs --
        they are all positive, and an uncentred row turns their common mean into a per-class offset that lets two or
        three classes win everywhere."""
        g = torch.Generator().manual_seed(seed)
        layers = {}
        lat, fpn = INDEX["neck.lateral_convs.0.conv"], INDEX["neck.fpn_convs.0.conv"]
        # drawn in the order the modules run: each level's lateral convolution, then its output convolution
        order = list(range(lat)) + [j + i for i in range(4) for j in (lat, fpn)] + list(range(fpn + 4, len(LAYERS)))
        for l in order:
            name = LAYERS[l][0]
            gain = 0.5 if name.endswith(".conv3") else 0.7 if name.startswith("neck.") else 1.0
            layers[l] = convnet.draw_layer(g, LAYERS[l], gain=gain, centre=name == SEG, classes=classes)
        return cls([layers[l] for l in range(len(LAYERS))])


# ---- plain-torch statement -------------------------------------------------------------------------------------------
def normalise(frames_u8, dtype=torch.float32):
    """u8 [B,H,W,3] -> [B,3,H,W] of ``dtype``: mmcv's ``Normalize``, (u8 - MEAN) / STD per channel, in ``dtype``."""
    return convnet.normalise("teeth", frames_u8, MEAN, STD, False, dtype)


def fpn_torch(weights: FPNWeights, x, taps=None):
    """Backbone, neck and head in eval mode up to ``conv_seg`` for normalised ``x`` [B,3,H,W] -> logits
    [B,C,H/4,W/4] (resnet.py:267-307, 659-674; fpn.py:163-213; fpn_head.py:55-69), BatchNorm not folded.  ``taps``: a
    list that receives the three stem outputs, the sixteen bottleneck outputs, the four neck outputs and the seven
    head convolutions' outputs (after the ReLU where there is one)."""
    p = weights.to(x.device, x.dtype)

    def conv(name, t):
        _, bn, _, _, _, k, stride = LAYERS[INDEX[name]]
        lay = p[name]
        y = F.conv2d(t, lay["weight"], lay.get("bias"), stride=stride, padding=k // 2)
        if bn:
            y = F.batch_norm(y, lay["mean"], lay["var"], lay["gamma"], lay["beta"], training=False, eps=BN_EPS)
        return y

    def tap(t):
        if taps is not None:
            taps.append(t)
        return t

    t = x
    for i in (0, 3, 6):
        t = tap(F.relu(conv(f"backbone.stem.{i}", t)))
    t = F.max_pool2d(t, kernel_size=3, stride=2, padding=1)
    feats = []
    for stage, blocks in enumerate(STAGE_BLOCKS, start=1):
        for b in range(blocks):
            pre = f"backbone.layer{stage}.{b}"
            out = conv(f"{pre}.conv3", F.relu(conv(f"{pre}.conv2", F.relu(conv(f"{pre}.conv1", t)))))
            identity = conv(f"{pre}.downsample.0", t) if b == 0 else t
            t = tap(F.relu(out + identity))
        feats.append(t)

    lat = [conv(f"neck.lateral_convs.{i}.conv", f) for i, f in enumerate(feats)]
    for i in (3, 2, 1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
    outs = [tap(conv(f"neck.fpn_convs.{i}.conv", l)) for i, l in enumerate(lat)]

    total = None
    for i in range(4):
        t = outs[i]
        for k in range(max(1, i)):
            t = tap(F.relu(conv(f"decode_head.scale_heads.{i}.{2 * k}.conv", t)))
            if i > 0:
                t = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
        # (fpn_head.py:62-66 resizes to the sum's size: the identity, the sides being multiples of 32)
        total = t if total is None else total + t
    return conv(SEG, total)


def upsample_torch(logits4, H: int, W: int):
    """Bilinear, ``align_corners=False``, to [B,C,H,W] (encoder_decoder.py:71-80)."""
    return F.interpolate(logits4, (H, W), mode="bilinear", align_corners=False)


def labels_torch(logits4, H: int, W: int):
    """Logits at 1/4 resolution -> labels u8 [B,H,W]: the bilinear upsample and the first-maximum argmax (the softmax in
    between is monotone and is not applied)."""
    return first_argmax(upsample_torch(logits4, H, W))


@torch.no_grad()
def teeth_torch(weights: FPNWeights, frames_u8, dtype=torch.float32):
    """The chain from u8 frames [B,H,W,3] to the teeth mask u8 [B,H,W] (1 = teeth) in plain torch, on the frames'
    device."""
    x, H, W = convnet.check_frames("teeth", frames_u8)
    labels = labels_torch(fpn_torch(weights, normalise(x, dtype)), H, W)
    return (labels == TEETH).to(torch.uint8)


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class TeethSegmenter(convnet.FrameOperator):
    """``mask(frames u8 [B,H,W,3]) -> u8 [B,H,W]`` (1 = teeth), ``labels -> u8 [B,H,W]`` and ``logits ->
    [B,C,H/4,W/4]`` on ``device`` through csrc/teeth.hip, in chunks of at most ``max_batch`` (convnet.FrameOperator).
    ``max_batch=None``: the largest batch, at most 8, whose workspace at 512 x 512 (100 MiB per frame: the stride-4 maps
    of 256 channels are 16 MiB each) stays within 1 GiB."""

    NAME = "teeth"
    net_torch, normalise_torch, labels_torch = staticmethod(fpn_torch), staticmethod(normalise), staticmethod(labels_torch)

    def __init__(self, weights: FPNWeights, device="cuda", max_batch=None):
        super().__init__(weights, device, max_batch)
        if max_batch is None and self.device.type == "cuda":
            per_frame = int(self._L.instag_teeth_workspace_bytes(1, SIZE, SIZE))
            max_batch = max(1, min(8, WORKSPACE_BUDGET // per_frame))
        self.max_batch = int(8 if max_batch is None else max_batch)

    def _workspace_bytes(self, batch, H, W):
        return self._L.instag_teeth_workspace_bytes(batch, H, W)

    def _run(self, frames_u8, want):
        from . import _lib
        x, H, W = convnet.check_frames(self.NAME, frames_u8)
        x = x.to(self.device).contiguous()
        B, Cn = int(x.shape[0]), self.weights.classes
        outs = self._empty(want, logits=(B, Cn, H // 4, W // 4), labels=(B, H, W), mask=(B, H, W))
        self._chunks(x, H, W, lambda c, m, ws, nbytes: self._L.instag_teeth_forward(
            C.byref(self._struct), _lib.ptr(x[c]), m, H, W, Cn, *(_lib.ptr(None if t is None else t[c]) for t in outs),
            ws, nbytes, _lib.current_stream()), "teeth_forward")
        return outs

    @torch.no_grad()
    def mask(self, frames_u8):
        if self.device.type != "cuda":
            return teeth_torch(self.weights, torch.as_tensor(frames_u8).to(self.device))
        return self._run(frames_u8, ("mask",))[2]


def teeth_labels(logits4, H: int, W: int, want_mask: bool = False):
    """The final stage alone on the device: logits fp32 [B,C,H/4,W/4] (cuda) -> labels u8 [B,H,W] (and the mask u8
    [B,H,W] of ``label == 7``): the bilinear upsample and the first-maximum argmax, one kernel."""
    from . import _lib
    logits4 = logits4.detach().to(dtype=torch.float32).contiguous()
    if logits4.dim() != 4 or H % 4 or W % 4 or tuple(logits4.shape[2:]) != (H // 4, W // 4) \
            or not MIN_CLASSES <= int(logits4.shape[1]) <= MAX_CLASSES:
        raise ValueError(f"teeth: logits [B,C,H/4,W/4] with {MIN_CLASSES} <= C <= {MAX_CLASSES}, got "
                         f"{tuple(logits4.shape)} for {H} x {W}")
    B, Cn = int(logits4.shape[0]), int(logits4.shape[1])
    labels = torch.empty(B, H, W, dtype=torch.uint8, device=logits4.device)
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=logits4.device) if want_mask else None
    with torch.cuda.device(logits4.device):
        rc = _lib.lib().instag_teeth_labels(_lib.ptr(logits4), B, H, W, Cn, _lib.ptr(labels), _lib.ptr(mask),
                                            _lib.current_stream())
    _lib.check_arg(rc, "teeth_labels")
    return (labels, mask) if want_mask else labels


# ---- a directory --------------------------------------------------------------------------------------------------------
def teeth_identity(path, weights: FPNWeights, device="cuda", write: bool = True, batch: int = 8, decoder=None):
    """ori_imgs/<i>.jpg of ``path`` (ascending numeric order) -> teeth masks u8 [N,H,W] (1 = teeth) on ``device``, what
    ``FrameStore.append(teeth=...)`` takes, H x W the frames' own size (create_teeth_mask.py does not resize).
    ``write``: also teeth_mask/<i>.npy as ``np.bool_ [H,W]``, the file ``dataset.decode_images`` reads.  ``decoder``: a
    ``jpeg_decode.JpegDecoder`` that decodes the files on the device (``convnet.frame_batches``)."""
    seg = TeethSegmenter(weights, torch.device(device), max_batch=batch)
    out = []
    if write:
        os.makedirs(os.path.join(path, "teeth_mask"), exist_ok=True)
    for ids, frames, _ in convnet.frame_batches(path, batch, decoder=decoder):
        mask = seg.mask(frames)
        out.append(mask)
        if write:
            for i, host in zip(ids, mask.cpu().numpy()):
                np.save(os.path.join(path, "teeth_mask", f"{i}.npy"), host.astype(np.bool_))
    return torch.cat(out, dim=0)
