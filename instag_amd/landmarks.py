"""Face landmarks on the device: from ``ori_imgs/<i>.jpg`` and one face box per frame to ``ori_imgs/<i>.lms``
(csrc/landmarks.hip).

The reference makes these files with the ``face_alignment`` package (data_utils/process.py:54-85:
``FaceAlignment(LandmarksType._2D, flip_input=False).get_landmarks(image)``, the 68 points saved with
``np.savetxt(..., '%f')``).  That package runs a face detector (S3FD) and then FAN-2D-4 on a crop around each detected
box.  Here is the second half: the crop, the network and the decode, for boxes that are given -- as the package itself
takes them through ``detected_faces=`` -- or that a ``face_detect.FaceDetector``, the first half, finds.

    w = FANWeights.load("2DFAN4-11f355bf06.pth.tar")                 # a file a user of the package has; none shipped or fetched
    detector = FaceDetector(S3FDWeights.load("s3fd-619a316812.pth"), "cuda")       # face_detect.py
    lms = landmarks_identity("data/May", w, "cuda", detector=detector)    # reads ori_imgs/*.jpg, writes ori_imgs/*.lms

On the GPU the crop, the network and the decode run in csrc/landmarks.hip (inference only, fp32); ``crop_torch``,
``fan_torch``, ``decode_torch`` and ``landmarks_torch`` are the plain-torch statement of the same arithmetic (any dtype,
CPU or GPU) that the tests compare against and a CPU device runs.  The project ships no weights and fetches none.

What is said here about the package -- the network's structure and module names, the keys of its state dict, the crop,
the transform and the decode -- is written from knowledge of the package, not read from it: neither ``face_alignment``
nor a FAN checkpoint was at hand, and no test compares with a ``face_alignment`` run.  What pins the definition is the
statements below, a golden made by a second, independently written ``nn.Module`` restatement
(tests/golden/make_golden_landmarks.py) and the host tests (tests/test_landmarks_host.py).

The network, ``FAN(num_modules=4)`` of the package's models.py, under its module names:

    conv1 (7 x 7, stride 2, pad 3, bias) -> bn1 -> ReLU; conv2 = ConvBlock(64, 128); avg_pool2d(2);
    conv3 = ConvBlock(128, 128); conv4 = ConvBlock(128, 256); then per stack i of 4:
      m{i} = HourGlass(depth 4, 256) with blocks b1_l, b2_l, b3_l (l = 4 .. 1) and b2_plus_1:
             up1 = b1(x); low = b3(inner(b2(avg_pool2d(x, 2)))); up1 + nearest_x2(low)
      top_m_{i} = ConvBlock(256, 256); conv_last{i} (1 x 1, bias) -> bn_end{i} -> ReLU; l{i} (1 x 1, 256 -> 68, bias):
      the stack's heatmaps; for i < 3: previous = previous + bl{i}(ll) + al{i}(heatmaps), both 1 x 1 with bias.
    ConvBlock(cin, cout) is pre-activation: o1 = conv1(relu(bn1(x))) (3 x 3, cin -> cout / 2), o2 = conv2(relu(bn2(o1)))
    (-> cout / 4), o3 = conv3(relu(bn3(o2))) (-> cout / 4), none with a bias; cat(o1, o2, o3) + residual, the residual
    x or, where cin != cout, downsample = bn -> relu -> 1 x 1 convolution without a bias.

The input is the RGB crop divided by 255 (no mean, no deviation); there is no flipped pass.

Around the network, for a box (x1, y1, x2, y2), in fp64 (the package builds a 3 x 3 matrix and inverts it in fp32,
which this closed form does not reproduce to the last ulp):

    center = (x2 - (x2 - x1) / 2, y2 - (y2 - y1) / 2 - 0.12 (y2 - y1)),  scale = (x2 - x1 + y2 - y1) / 195
    transform(p, center, scale, res, invert=True) = trunc(p h / res + center - h / 2),  h = 200 scale
    crop: ul = transform((1, 1), 256), br = transform((256, 256), 256); a zero image of (br - ul) receives the part of
    the frame that overlaps it, by the package's 1-based index arithmetic; it is resized to S x S (S = 256).
    decode: the first maximum of each S/4 x S/4 heatmap; strictly inside the map, +-0.25 along x and y by the sign of
    the neighbour difference (none for a zero difference); minus 0.5 in 1-based coordinates; transform(., res = S/4,
    invert=True), truncation included -- so the landmarks are whole numbers.

The package resizes with ``cv2.resize(INTER_LINEAR)`` on uint8.  OpenCV is not a dependency, so the resize is this
project's rule and is not checked against OpenCV: half-pixel-centre bilinear with the source indices clamped, in exact
integer arithmetic -- the source position of output index o among n pixels is ((2 o + 1) n - S) / (2 S), its fraction
becomes an integer weight out of 512 (rounded half up) per axis, and the weighted sum is rounded half up to uint8.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import convnet
from .convnet import BN_EPS

SIZE = 256                                           # the package's crop
N_POINTS, N_STACKS, DEPTH, TRUNK = 68, 4, 4, 256
MIN_SIDE, MAX_SIDE, SIDE_MULTIPLE = 64, 512, 64
MAX_COORD = 1 << 20                                  # a box coordinate beyond this is refused like a NaN
MAX_STATEMENT_CROP = 1 << 26                         # pixels of the (br - ul) image ``crop_torch`` is willing to build
WORKSPACE_BUDGET = 1 << 30
MOUTH = slice(48, 68)
# the parser's classes (parsing.py) that make up a face: skin, brows, eyes, glasses, nose, mouth, lips
FACE_CLASSES = (1, 2, 3, 4, 5, 6, 10, 11, 12, 13)


def _block(p, cin, cout):
    rows = [(f"{p}.conv1", f"{p}.bn1", False, cin, cout // 2, 3, 1), (f"{p}.conv2", f"{p}.bn2", False, cout // 2, cout // 4, 3, 1),
            (f"{p}.conv3", f"{p}.bn3", False, cout // 4, cout // 4, 3, 1)]
    if cin != cout:
        rows.append((f"{p}.downsample.2", f"{p}.downsample.0", False, cin, cout, 1, 1))
    return rows


def _layers():
    # (convolution, its BatchNorm or None, bias?, cin, cout, kernel, stride); in a block the BatchNorm stands in FRONT
    out = [("conv1", "bn1", True, 3, 64, 7, 2)] + _block("conv2", 64, 128) + _block("conv3", 128, 128) + _block("conv4", 128, 256)
    for i in range(N_STACKS):
        for l in range(DEPTH, 0, -1):
            out += _block(f"m{i}.b1_{l}", TRUNK, TRUNK) + _block(f"m{i}.b2_{l}", TRUNK, TRUNK)
        out += _block(f"m{i}.b2_plus_1", TRUNK, TRUNK)
        for l in range(1, DEPTH + 1):
            out += _block(f"m{i}.b3_{l}", TRUNK, TRUNK)
        out += _block(f"top_m_{i}", TRUNK, TRUNK)
        out += [(f"conv_last{i}", f"bn_end{i}", True, TRUNK, TRUNK, 1, 1), (f"l{i}", None, True, TRUNK, N_POINTS, 1, 1)]
        if i < N_STACKS - 1:
            out += [(f"bl{i}", None, True, TRUNK, TRUNK, 1, 1), (f"al{i}", None, True, N_POINTS, TRUNK, 1, 1)]
    return tuple(out)


# in the order of struct instag_landmarks_weights
LAYERS = _layers()
INDEX = {name: i for i, (name, *_) in enumerate(LAYERS)}
PRE = frozenset(i for i, (name, bn, *_) in enumerate(LAYERS) if bn and name != "conv1" and not name.startswith("conv_last"))


def macs_per_face(S: int = SIZE) -> int:
    """Multiply-accumulates of the 194 convolutions of one S x S crop, from the table."""
    total = 0
    for name, _, _, cin, cout, k, _ in LAYERS:
        head = name.split(".")[0]
        if head in ("conv1", "conv2"):
            side = S // 2
        elif head.startswith("m"):
            kind, l = name.split(".")[1].rsplit("_", 1)          # b1 runs at the level's own side, the others at half
            side = (S // 4) >> (DEPTH - int(l) + (0 if kind == "b1" else 1))
        else:
            side = S // 4
        total += cin * cout * k * k * side * side
    return total


# ---- weights ----------------------------------------------------------------------------------------------------------
class FANWeights(convnet.ConvWeights):
    """The frozen parameters of FAN-2D-4 under the package's key names (``conv2.bn1.weight``, ``m0.b1_4.conv1.weight``,
    ``conv4.downsample.0.running_mean``, ``conv4.downsample.2.weight``, ``top_m_0...``, ``conv_last0``, ``bn_end0``,
    ``l0``, ``bl0``, ``al0``, ...).  ``from_state_dict`` / ``load`` take the state dict of a ``2DFAN4-*.pth.tar`` of
    face_alignment <= 1.2 and, through ``torch.jit.load(...).state_dict()``, the TorchScript archive of later releases.
    The fold is this network's: a scale and shift BEHIND the convolution only for ``conv1`` + ``bn1`` and ``conv_last`` +
    ``bn_end`` (and the bias as shift for ``l``, ``bl``, ``al``); for every block convolution and every ``downsample`` a
    per-input-channel scale and shift in FRONT of it, which the kernel applies with the ReLU in its gather."""

    TABLE, LABEL, STRUCT, PRE = LAYERS, "FAN weights", "LandmarksWeights", PRE

    @classmethod
    def random(cls, seed: int = 0, gain: float = 0.5) -> "FANWeights":
        """Seeded stand-ins (tests, benches; convnet.draw_layer): ``gain`` scales the block convolutions and the
        downsamples -- at 0.5 the heatmap scale grows about x10 per stack and stays in range --, the other layers
        have gain 1.  A block's BatchNorm is drawn behind its convolution, over the convolution's inputs."""
        g = torch.Generator().manual_seed(seed)
        layers = []
        for l, row in enumerate(LAYERS):
            if l not in PRE:
                layers.append(convnet.draw_layer(g, row))
                continue
            name, _, bias, cin, cout, k, stride = row
            lay = convnet.draw_layer(g, (name, None, bias, cin, cout, k, stride), gain=gain)
            lay.update(gamma=torch.rand(cin, generator=g) + 0.5, beta=torch.randn(cin, generator=g) * 0.2,
                       mean=torch.randn(cin, generator=g) * 0.2, var=torch.rand(cin, generator=g) + 0.5)
            layers.append(lay)
        return cls(layers)

    @classmethod
    def from_state_dict(cls, sd):
        """``sd``: the package's keys (a ``{"state_dict": ...}`` wrapper and a ``module.`` prefix are taken off).
        ``num_batches_tracked`` is accepted and not read; a missing key raises a ValueError naming it, a misshapen one
        names the layer and the field."""
        if "state_dict" in sd and not torch.is_tensor(sd["state_dict"]):
            sd = sd["state_dict"]
        if sd and all(k.startswith("module.") for k in sd):
            sd = {k[len("module."):]: v for k, v in sd.items()}
        return super().from_state_dict(sd)

    @classmethod
    def load(cls, path):
        """A pickled state dict (``2DFAN4-*.pth.tar``) or a TorchScript archive (``2DFAN4-*.zip``)."""
        try:
            sd = torch.jit.load(path, map_location="cpu").state_dict()
        except RuntimeError:
            sd = torch.load(path, map_location="cpu")
        return cls.from_state_dict(sd)

    def folded(self, dtype=torch.float64):
        """Per layer (bias-free convolution weight, scale, shift, pre_scale, pre_shift), folded in fp64: behind the
        convolution as convnet.ConvWeights.folded; for a layer of ``PRE`` scale = 1, shift = 0 and, over its inputs,
        pre_scale = gamma / sqrt(var + eps), pre_shift = beta - mean pre_scale.  None where there is no pre-activation."""
        out = []
        for l, lay in enumerate(self.layers):
            d = {f: t.double() for f, t in lay.items()}
            zero = torch.zeros(d["weight"].shape[0], dtype=torch.float64)
            bn = d["gamma"] / torch.sqrt(d["var"] + BN_EPS) if "gamma" in d else None
            if l in PRE:
                row = (d["weight"], torch.ones_like(zero), zero, bn, d["beta"] - d["mean"] * bn)
            else:
                scale = torch.ones_like(zero) if bn is None else bn
                row = (d["weight"], scale, (d.get("bias", zero) - d.get("mean", zero)) * scale + d.get("beta", zero), None, None)
            out.append(tuple(None if t is None else t.to(dtype) for t in row))
        return out

    def device_pack(self, device):
        """The C struct for ``device``: every convolution as [K = (cin, ky, kx)][cout], the stem's K padded with zero rows
        to 160 and ``al``'s to 96."""
        from . import _lib
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        pack = self._packs.get(key)
        if pack is not None:
            return pack
        keep, s = [], _lib.LandmarksWeights()
        for l, (w, scale, shift, ps, pb) in enumerate(self.folded(torch.float32)):
            wk = w.reshape(w.shape[0], -1).t()
            rows = -(-wk.shape[0] // 32) * 32
            wk = torch.cat([wk, torch.zeros(rows - wk.shape[0], wk.shape[1])], dim=0)
            ts = [None if t is None else t.contiguous().to(device) for t in (wk, scale, shift, ps, pb)]
            keep += ts
            s.w[l], s.scale[l], s.shift[l], s.pre_scale[l], s.pre_shift[l] = [None if t is None else t.data_ptr() for t in ts]
        pack = self._packs[key] = (s, keep)
        return pack


# ---- plain-torch statement: the network --------------------------------------------------------------------------------
def normalise(crops_u8, dtype=torch.float32):
    """u8 [B,S,S,3] -> [B,3,S,S] of ``dtype``: u8 / 255."""
    x = convnet.check_frames("landmarks", crops_u8, sides=False)[0]
    return x.permute(0, 3, 1, 2).to(dtype) / 255


def check_side(S: int):
    if not (MIN_SIDE <= S <= MAX_SIDE and S % SIDE_MULTIPLE == 0):
        raise ValueError(f"landmarks: crops of side S, a multiple of {SIDE_MULTIPLE} in [{MIN_SIDE}, {MAX_SIDE}], got {S}")


def fan_torch(weights: FANWeights, x, all_stacks: bool = False):
    """FAN in eval mode for ``x`` [B,3,S,S] (the crop / 255) -> the last stack's heatmaps [B,68,S/4,S/4], or all four as
    [B,4,68,S/4,S/4]; BatchNorm not folded."""
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError(f"landmarks: x [B,3,S,S], got {tuple(x.shape)}")
    check_side(int(x.shape[2]))
    p = weights.to(x.device, x.dtype)

    def bn(lay, t):
        return F.batch_norm(t, lay["mean"], lay["var"], lay["gamma"], lay["beta"], training=False, eps=BN_EPS)

    def conv(name, t):
        lay, k, stride = p[name], *LAYERS[INDEX[name]][5:7]
        if INDEX[name] in PRE:
            return F.conv2d(F.relu(bn(lay, t)), lay["weight"], None, stride=stride, padding=k // 2)
        y = F.conv2d(t, lay["weight"], lay.get("bias"), stride=stride, padding=k // 2)
        return bn(lay, y) if "gamma" in lay else y

    def block(name, t):
        o1 = conv(f"{name}.conv1", t)
        o2 = conv(f"{name}.conv2", o1)
        o3 = conv(f"{name}.conv3", o2)
        residual = conv(f"{name}.downsample.2", t) if f"{name}.downsample.2" in INDEX else t
        return torch.cat((o1, o2, o3), dim=1) + residual

    def hourglass(i, l, t):
        up1 = block(f"m{i}.b1_{l}", t)
        low = block(f"m{i}.b2_{l}", F.avg_pool2d(t, 2))
        low = hourglass(i, l - 1, low) if l > 1 else block(f"m{i}.b2_plus_{l}", low)
        low = block(f"m{i}.b3_{l}", low)
        return up1 + F.interpolate(low, scale_factor=2, mode="nearest")

    t = F.relu(conv("conv1", x))
    t = F.avg_pool2d(block("conv2", t), 2)
    previous = block("conv4", block("conv3", t))
    outs = []
    for i in range(N_STACKS):
        ll = block(f"top_m_{i}", hourglass(i, DEPTH, previous))
        ll = F.relu(conv(f"conv_last{i}", ll))
        outs.append(conv(f"l{i}", ll))
        if i < N_STACKS - 1:
            previous = previous + conv(f"bl{i}", ll) + conv(f"al{i}", outs[-1])
    return torch.stack(outs, dim=1) if all_stacks else outs[-1]


# ---- plain-torch statement: around the network -----------------------------------------------------------------------
def check_boxes(boxes, n=None):
    """-> float32 [B,4] on the CPU; a [4] box serves all ``n`` frames."""
    b = torch.as_tensor(boxes).detach().to("cpu", torch.float32)
    if b.dim() == 1 and b.shape[0] == 4 and n is not None:
        b = b[None].expand(n, 4)
    if b.dim() != 2 or b.shape[1] != 4 or (n is not None and b.shape[0] != n):
        raise ValueError(f"landmarks: boxes [N,4] (or [4]) = (x1, y1, x2, y2), one row per frame, got {tuple(b.shape)}")
    return b.contiguous()


def usable(boxes):
    """[B] bool: every coordinate finite and at most ``MAX_COORD`` in magnitude."""
    return (boxes.abs() <= MAX_COORD).all(dim=1)


def center_scale(boxes):
    """float boxes [B,4] -> (cx, cy, h) in fp64, each [B], h = 200 scale."""
    x1, y1, x2, y2 = boxes.double().unbind(dim=1)
    w, hg = x2 - x1, y2 - y1
    return x2 - w / 2.0, y2 - hg / 2.0 - 0.12 * hg, 200.0 * ((w + hg) / 195.0)


def inverse(p, c, h, res):
    """transform(p, center, scale, res, invert=True) along one axis, fp64, truncated toward zero."""
    return (p * h / float(res) + c - h / 2.0).trunc()


def _resize_axis(n: int, S: int):
    """One axis of the integer resize: per output index the two clamped source indices and the second's weight of 512."""
    num = (2 * torch.arange(S, dtype=torch.int64) + 1) * n - S
    fl = torch.div(num, 2 * S, rounding_mode="floor")
    w1 = torch.div((num - fl * 2 * S) * 512 + S, 2 * S, rounding_mode="floor")
    return fl.clamp(0, n - 1), (fl + 1).clamp(0, n - 1), w1


def resize_torch(img_u8, S: int):
    """u8 [h,w,3] -> u8 [S,S,3]: this project's rule (module docstring), exact integers."""
    h, w = int(img_u8.shape[0]), int(img_u8.shape[1])
    y0, y1, wy = _resize_axis(h, S)
    x0, x1, wx = _resize_axis(w, S)
    v = img_u8.to(torch.int64)
    wy, wx = wy.view(S, 1, 1), wx.view(1, S, 1)
    top = v[y0][:, x0] * (512 - wx) + v[y0][:, x1] * wx
    bot = v[y1][:, x0] * (512 - wx) + v[y1][:, x1] * wx
    return ((top * (512 - wy) + bot * wy + (1 << 17)) >> 18).to(torch.uint8)


def crop_torch(frames_u8, boxes, S: int = SIZE, frame_index=None):
    """u8 frames [N,H,W,3] and boxes [B,4] (box b belongs to frame ``frame_index[b]``, default b) -> crops u8 [B,S,S,3]
    on the CPU.  The (br - ul) image is built by the package's 1-based index arithmetic as it stands, a range that comes
    out empty copying nothing; a box that is not ``usable`` or whose image has no pixel gives a zero crop."""
    x = convnet.check_frames("landmarks", frames_u8, sides=False)[0].cpu()
    boxes = check_boxes(boxes, None if frame_index is not None else int(x.shape[0]))
    ht, wd = int(x.shape[1]), int(x.shape[2])
    cx, cy, h = center_scale(boxes)
    ok = usable(boxes)
    out = torch.zeros(boxes.shape[0], S, S, 3, dtype=torch.uint8)
    for b in range(boxes.shape[0]):
        f = b if frame_index is None else int(frame_index[b])
        if not bool(ok[b]) or not 0 <= f < x.shape[0]:
            continue
        ul = [int(inverse(1.0, c[b], h[b], 256)) for c in (cx, cy)]
        br = [int(inverse(256.0, c[b], h[b], 256)) for c in (cx, cy)]
        if br[0] - ul[0] < 1 or br[1] - ul[1] < 1:
            continue
        if (br[0] - ul[0]) * (br[1] - ul[1]) > MAX_STATEMENT_CROP:
            raise ValueError(f"landmarks: the statement does not build a crop of {br[0] - ul[0]} x {br[1] - ul[1]} pixels")
        new = torch.zeros(br[1] - ul[1], br[0] - ul[0], 3, dtype=torch.uint8)
        new_x = (max(1, -ul[0] + 1), min(br[0], wd) - ul[0])
        new_y = (max(1, -ul[1] + 1), min(br[1], ht) - ul[1])
        old_x = (max(1, ul[0] + 1), min(br[0], wd))
        old_y = (max(1, ul[1] + 1), min(br[1], ht))
        if old_x[1] >= old_x[0] and old_y[1] >= old_y[0]:
            new[new_y[0] - 1:new_y[1], new_x[0] - 1:new_x[1]] = x[f, old_y[0] - 1:old_y[1], old_x[0] - 1:old_x[1]]
        out[b] = resize_torch(new, S)
    return out


def decode_torch(heatmaps, boxes):
    """Heatmaps [B,68,R,R] (any float dtype) and boxes [B,4] -> landmarks float32 [B,68,2] = (x, y) on the heatmaps'
    device, whole numbers; NaN for a box that is not ``usable``."""
    B, P, R, _ = heatmaps.shape
    boxes = check_boxes(boxes, B)
    flat = heatmaps.reshape(B, P, R * R)
    n = torch.arange(R * R, device=flat.device)
    arg = torch.where(flat == flat.max(dim=2, keepdim=True).values, n, R * R).min(dim=2).values.clamp(max=R * R - 1)
    py, px = arg // R, arg % R
    inside = (px > 0) & (px < R - 1) & (py > 0) & (py < R - 1)

    def at(dy, dx):
        return flat.gather(2, ((py + dy).clamp(0, R - 1) * R + (px + dx).clamp(0, R - 1))[..., None])[..., 0]

    sx = torch.sign(at(0, 1) - at(0, -1)).double() * inside
    sy = torch.sign(at(1, 0) - at(-1, 0)).double() * inside
    cx, cy, h = (t.to(flat.device)[:, None] for t in center_scale(boxes))
    x = inverse((px + 1).double() + 0.25 * sx - 0.5, cx, h, R)
    y = inverse((py + 1).double() + 0.25 * sy - 0.5, cy, h, R)
    out = torch.stack((x, y), dim=-1).float()
    out[~usable(boxes).to(out.device)] = float("nan")
    return out


@torch.no_grad()
def landmarks_torch(weights: FANWeights, frames_u8, boxes, dtype=torch.float32, S: int = SIZE):
    """The chain from u8 frames [N,H,W,3] and boxes [N,4] to landmarks float32 [N,68,2] in plain torch, the network on
    the frames' device in ``dtype`` (the crop is integer work on the CPU)."""
    frames = torch.as_tensor(frames_u8)
    boxes = check_boxes(boxes, int(frames.shape[0]))
    crops = crop_torch(frames, boxes, S).to(frames.device)
    return decode_torch(fan_torch(weights, normalise(crops, dtype)), boxes)


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class LandmarkNet(convnet.FrameOperator):
    """``heatmaps(crops u8 [B,S,S,3], all_stacks=False) -> [B,68,S/4,S/4]`` fp32 (or the four stacks,
    [B,4,68,S/4,S/4]) for S a multiple of 64 in [64, 512] -- the network is fully convolutional; the package runs it at
    256 -- and ``landmarks(frames u8 [N,H,W,3], boxes [N,4] or [4]) -> float32 [N,68,2]`` on ``device`` through
    csrc/landmarks.hip, in chunks of at most ``max_batch`` faces with one kept workspace (convnet.FrameOperator); a CPU
    device runs the statements.  ``max_batch=None``: the largest batch, at most 32, whose workspace at S = 256 (31 MiB
    per face) stays within 1 GiB: the convolutions of the hourglass's low levels are short on positions, and a launch
    over more faces costs them little more.  A frame whose box has a NaN gets NaN landmarks and costs nothing."""

    NAME = "landmarks"

    def __init__(self, weights: FANWeights, device="cuda", max_batch=None):
        super().__init__(weights, device, max_batch)
        if max_batch is None and self.device.type == "cuda":
            max_batch = max(1, min(32, WORKSPACE_BUDGET // int(self._L.instag_landmarks_workspace_bytes(1, SIZE))))
        self.max_batch = int(32 if max_batch is None else max_batch)
        if self.device.type == "cuda":
            from . import _lib
            if self.max_batch > _lib.LANDMARKS["INSTAG_LANDMARKS_MAX_BATCH"]:
                raise ValueError(f"LandmarkNet: max_batch at most {_lib.LANDMARKS['INSTAG_LANDMARKS_MAX_BATCH']}")

    def _workspace_bytes(self, batch, S, _):
        return self._L.instag_landmarks_workspace_bytes(batch, S)

    @torch.no_grad()
    def heatmaps(self, crops_u8, all_stacks: bool = False):
        x = convnet.check_frames(self.NAME, crops_u8, sides=False)[0]
        B, S = int(x.shape[0]), int(x.shape[1])
        if x.shape[2] != S:
            raise ValueError(f"landmarks: square crops [B,S,S,3], got {tuple(x.shape)}")
        check_side(S)
        x = x.to(self.device).contiguous()
        if self.device.type != "cuda":
            return fan_torch(self.weights, normalise(x), all_stacks)
        from . import _lib
        shape = (B, N_STACKS, N_POINTS, S // 4, S // 4) if all_stacks else (B, N_POINTS, S // 4, S // 4)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._chunks(x, S, S, lambda c, m, ws, nbytes: self._L.instag_landmarks_forward(
            C.byref(self._struct), _lib.ptr(x[c]), m, S, int(all_stacks), _lib.ptr(out[c]), ws, nbytes,
            _lib.current_stream()), "landmarks_forward")
        return out

    @torch.no_grad()
    def crop(self, frames_u8, boxes, S: int = SIZE, frame_index=None):
        """The crop alone: -> u8 [B,S,S,3] on the device (``crop_torch``'s arguments)."""
        x = convnet.check_frames(self.NAME, frames_u8, sides=False)[0]
        check_side(S)
        boxes = check_boxes(boxes, None if frame_index is not None else int(x.shape[0]))
        if self.device.type != "cuda":
            return crop_torch(x, boxes, S, frame_index).to(self.device)
        from . import _lib
        x, boxes = x.to(self.device).contiguous(), boxes.to(self.device)
        idx = None if frame_index is None else torch.as_tensor(frame_index).to(self.device, torch.int32).contiguous()
        B = int(boxes.shape[0])
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=self.device)
        step = _lib.LANDMARKS["INSTAG_LANDMARKS_MAX_BATCH"]
        with torch.cuda.device(self.device):
            for i in range(0, B, step):
                c = slice(i, min(B, i + step))
                # without an index box b reads frame b: the chunk's frames are passed with it
                frames, n = (x[c], c.stop - c.start) if idx is None else (x, int(x.shape[0]))
                _lib.check_arg(self._L.instag_landmarks_crop(
                    _lib.ptr(frames), n, int(x.shape[1]), int(x.shape[2]), _lib.ptr(boxes[c]),
                    _lib.ptr(None if idx is None else idx[c]), c.stop - c.start, S, _lib.ptr(out[c]),
                    _lib.current_stream()), "landmarks_crop")
        return out

    @torch.no_grad()
    def decode(self, heatmaps, boxes):
        """The decode alone: heatmaps fp32 [B,68,R,R] -> float32 [B,68,2] (``decode_torch``'s arguments)."""
        if heatmaps.dim() != 4 or heatmaps.shape[1] != N_POINTS or heatmaps.shape[2] != heatmaps.shape[3]:
            raise ValueError(f"landmarks: heatmaps [B,{N_POINTS},R,R], got {tuple(heatmaps.shape)}")
        B, R = int(heatmaps.shape[0]), int(heatmaps.shape[2])
        boxes = check_boxes(boxes, B)
        if self.device.type != "cuda":
            return decode_torch(heatmaps.to(self.device), boxes)
        from . import _lib
        hm = heatmaps.to(self.device, torch.float32).contiguous()
        out = torch.empty(B, N_POINTS, 2, dtype=torch.float32, device=self.device)
        if B:
            with torch.cuda.device(self.device):
                _lib.check_arg(self._L.instag_landmarks_decode(_lib.ptr(hm), _lib.ptr(boxes.to(self.device)), B, R,
                                                               _lib.ptr(out), _lib.current_stream()), "landmarks_decode")
        return out

    @torch.no_grad()
    def landmarks(self, frames_u8, boxes, S: int = SIZE):
        x = convnet.check_frames(self.NAME, frames_u8, sides=False)[0]
        N = int(x.shape[0])
        boxes = check_boxes(boxes, N)
        if self.device.type != "cuda":
            return landmarks_torch(self.weights, x.to(self.device), boxes, S=S)
        x = x.to(self.device).contiguous()
        out = torch.full((N, N_POINTS, 2), float("nan"), dtype=torch.float32, device=self.device)
        rows = torch.nonzero(usable(boxes))[:, 0]
        for i in range(0, int(rows.shape[0]), self.max_batch):
            r = rows[i:i + self.max_batch]
            crops = self.crop(x, boxes[r], S, frame_index=r)
            out[r.to(self.device)] = self.decode(self.heatmaps(crops), boxes[r])
        return out


def conv_torch(x, weight, scale, shift, pre=None, res=None, res2=None, relu=False):
    """The statement of ``conv_slice``: -> (raw, value) with raw = scale conv(pre(x)) + shift and value = act(raw + res +
    nearest_x2(res2)), ``res`` and ``res2`` already cut to the slice; ``pre`` = (pre_scale, pre_shift) over the inputs."""
    if pre is not None:
        x = F.relu(x * pre[0].view(1, -1, 1, 1) + pre[1].view(1, -1, 1, 1))
    raw = F.conv2d(x, weight, padding=weight.shape[-1] // 2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    v = raw
    if res is not None:
        v = v + res
    if res2 is not None:
        v = v + F.interpolate(res2, scale_factor=2, mode="nearest")
    return raw, F.relu(v) if relu else v


@torch.no_grad()
def conv_slice(x, weight, scale, shift, out, out_off=0, pre=None, res=None, res2=None, raw=False, relu=False, tile=0):
    """One convolution of the network's body alone on the device (``instag_landmarks_conv``; for the tests of the shared
    kernel's options): ``x`` fp32 [B,cin,H,W], ``weight`` [cout,cin,k,k] with k 1 or 3 -> channels ``out_off ..`` of
    ``out`` [B,out_ch,H,W], written in place; ``res`` [B,out_ch,H,W] and ``res2`` [B,out_ch,H/2,W/2] are read at the
    same channels.  -> the contiguous copy in front of the residuals [B,cout,H,W] where ``raw``, else None."""
    from . import _lib
    cout, cin, k, _ = weight.shape
    B, _, H, W = x.shape
    wk = weight.reshape(cout, -1).t().float()
    wk = torch.cat([wk, torch.zeros(-(-wk.shape[0] // 32) * 32 - wk.shape[0], cout, device=wk.device)]).contiguous().to(x.device)
    f = lambda t: None if t is None else t.to(x.device, torch.float32).contiguous()
    scale, shift, res, res2 = f(scale), f(shift), f(res), f(res2)
    ps, pb = (None, None) if pre is None else (f(pre[0]), f(pre[1]))
    if not (out.is_contiguous() and out.dtype == torch.float32 and out.dim() == 4 and tuple(out.shape[::3]) == (B, W)
            and out.shape[2] == H):
        raise ValueError(f"landmarks: out fp32 contiguous [B,out_ch,H,W], got {tuple(out.shape)}")
    for t, hw in ((res, (H, W)), (res2, (H // 2, W // 2))):
        if t is not None and tuple(t.shape) != (B, out.shape[1]) + hw:
            raise ValueError(f"landmarks: a residual of shape {tuple(t.shape)} for out {tuple(out.shape)}")
    keep = torch.empty(B, cout, H, W, dtype=torch.float32, device=x.device) if raw else None
    with torch.cuda.device(x.device):
        _lib.check_arg(_lib.lib().instag_landmarks_conv(
            _lib.ptr(f(x)), _lib.ptr(wk), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(ps), _lib.ptr(pb), _lib.ptr(res),
            _lib.ptr(res2), _lib.ptr(keep), _lib.ptr(out), B, cin, cout, H, W, k, int(out.shape[1]), int(out_off), int(relu),
            int(tile), _lib.current_stream()), "landmarks_conv")
    return keep


# ---- a directory, the stand-in for the detector, the metric -----------------------------------------------------------
def write_landmarks(path, lms):
    """One ``.lms`` file as the reference writes it (process.py:84: ``np.savetxt(..., '%f')``)."""
    np.savetxt(path, np.asarray(lms, dtype=np.float32), "%f")


def landmarks_identity(path, weights: FANWeights, device="cuda", boxes=None, write: bool = True, batch: int = 32,
                       detector=None, decoder=None):
    """ori_imgs/<i>.jpg of ``path`` (ascending numeric order) and ``boxes`` [N,4] (or [4]) in that order -> landmarks
    float32 [N,68,2] on ``device``.  Without boxes, ``detector`` (a ``face_detect.FaceDetector``) finds them: each
    batch's boxes are ``detector.first(frames)``, the face process.py takes.  ``write``: also ori_imgs/<i>.lms, what
    ``track.read_landmarks`` reads; a frame whose box row has a NaN gets no file (and a NaN row), as a frame without a
    detection gets none in the reference.  ``decoder``: a ``jpeg_decode.JpegDecoder`` that decodes the files on the device
    (``convnet.frame_batches``)."""
    from .prepare import list_frames
    if boxes is None and detector is None:
        raise ValueError("landmarks_identity: boxes [N,4], one per frame (the face detector is not part of this project)")
    if boxes is not None:
        boxes = check_boxes(boxes, len(list_frames(path)))
    net = LandmarkNet(weights, torch.device(device), max_batch=batch)
    out, at = [], 0
    for ids, frames, _ in convnet.frame_batches(path, batch, decoder=decoder):
        lms = net.landmarks(frames, detector.first(frames) if boxes is None else boxes[at:at + len(ids)])
        at += len(ids)
        out.append(lms)
        if write:
            for i, host in zip(ids, lms.cpu().numpy()):
                if not np.isnan(host).any():
                    write_landmarks(os.path.join(path, "ori_imgs", f"{i}.lms"), host)
    return torch.cat(out, dim=0)


def boxes_from_labels(labels_u8):
    """Parser labels u8 [N,H,W] (parsing.FaceParser.labels) -> boxes float32 [N,4] = (x1, y1, x2, y2): the bounding box
    of the pixels of the face classes (skin, brows, eyes, glasses, nose, mouth, lips), x2 and y2 one past the last
    pixel; a NaN row where a frame has none.  Plain torch, on the labels' device.

    **This project's rule, for a caller without S3FD weights: the reference's boxes come from the face detector, which is
    ``face_detect.FaceDetector`` (``landmarks_identity(detector=...)``); these do not, and nothing is claimed about how
    close the landmarks they lead to are to the reference's.**"""
    lab = torch.as_tensor(labels_u8)
    if lab.dim() != 3:
        raise ValueError(f"landmarks: labels [N,H,W], got {tuple(lab.shape)}")
    face = torch.zeros_like(lab, dtype=torch.bool)
    for c in FACE_CLASSES:
        face |= lab == c
    N, H, W = face.shape
    cols, rows = face.any(dim=1), face.any(dim=2)                                   # [N,W], [N,H]
    ix, iy = torch.arange(W, device=lab.device), torch.arange(H, device=lab.device)
    x1 = torch.where(cols, ix, W).min(dim=1).values
    x2 = torch.where(cols, ix, -1).max(dim=1).values + 1
    y1 = torch.where(rows, iy, H).min(dim=1).values
    y2 = torch.where(rows, iy, -1).max(dim=1).values + 1
    out = torch.stack((x1, y1, x2, y2), dim=1).float()
    out[~cols.any(dim=1)] = float("nan")
    return out


def lmd_torch(pred_lms, gt_lms, region: str = "mouth"):
    """The reference's landmark distance (metrics.py:81-90) per frame: [N,68,2] twice -> [N]; each set (the mouth's
    points 48..67, or all of ``region="face"``) minus its own mean, then the mean Euclidean distance."""
    if region not in ("mouth", "face"):
        raise ValueError(f"lmd: region 'mouth' or 'face', got {region!r}")
    p, g = (t[:, MOUTH] if region == "mouth" else t for t in (pred_lms, gt_lms))
    p, g = p - p.mean(dim=1, keepdim=True), g - g.mean(dim=1, keepdim=True)
    return ((p - g) ** 2).sum(dim=2).sqrt().mean(dim=1)
