"""Face detection on the device: from ``ori_imgs/<i>.jpg`` to one face box per frame, what the landmark network
(landmarks.py) crops by (csrc/face_detect.hip).

The reference makes ``ori_imgs/<i>.lms`` with the ``face_alignment`` package (data_utils/process.py:54-85), which runs
a face detector (S3FD) and then FAN-2D-4 on a crop around each detected box; its LMD meter (metrics.py:35-49) does the
same on every rendered and ground-truth frame.  Here is the first half: the network, the score, the box decode and
the non-maximum suppression.

    w = S3FDWeights.load("s3fd-619a316812.pth")                       # a file a user of the package has; none shipped or fetched
    det = FaceDetector(w, "cuda")
    boxes, count, overflow = det.detect(frames_u8)                    # [N,16,5], [N], [N]
    lms = landmarks_identity("data/May", fan, "cuda", detector=det)   # reads ori_imgs/*.jpg, writes ori_imgs/*.lms

On the GPU the network and the tail run in csrc/face_detect.hip (inference only, fp32 convolutions); ``s3fd_torch``,
``normalise_torch``, ``scores_torch``, ``candidates_torch``, ``nms_torch``, ``post_torch`` and ``detect_torch`` are the
plain-torch statement of the same arithmetic that the tests compare against and a CPU device runs.  The project ships
no weights and fetches none.

What is said here about the package -- the network's structure and module names, the keys of its state dict, the
input, the priors, the decode and the suppression -- is written from knowledge of the package, not read from it:
neither ``face_alignment`` nor an S3FD checkpoint was at hand, and no test compares with a ``face_alignment`` run.  What
pins the definition is the statements below, a golden made by a second, independently written restatement
(tests/golden/make_golden_face_detect.py, tests/face_detect_helpers.py) and the host tests
(tests/test_face_detect_host.py).

The network (the package's detection/sfd/net_s3fd.py), under its module names; every convolution has a bias and no
BatchNorm, a ReLU follows every trunk convolution and none of the heads, 3 x 3 is stride 1 and pad 1 unless said, a
pool is ``max_pool2d(2, 2)``:

    conv1_1 3 -> 64, conv1_2, pool; conv2_1 64 -> 128, conv2_2, pool; conv3_1 128 -> 256, conv3_2, conv3_3 (f3), pool;
    conv4_1 256 -> 512, conv4_2, conv4_3 (f4), pool; conv5_1..3 512 (f5), pool;
    fc6 512 -> 1024, 3 x 3 with PADDING 3 and no dilation (the map grows by 4 per axis: a quirk of the package's
    conversion, kept); fc7 1024 -> 1024, 1 x 1 (f7); conv6_1 1024 -> 256, 1 x 1; conv6_2 256 -> 512, 3 x 3, stride 2 (f6);
    conv7_1 512 -> 128, 1 x 1; conv7_2 128 -> 256, 3 x 3, stride 2 (f72);
    conv3_3_norm, conv4_3_norm, conv5_3_norm = L2Norm with one weight [C] (initially 10, 8, 5):
    x / (sqrt(sum_c x^2) + 1e-10) * weight[c];
    six levels f3n, f4n, f5n, f7, f6, f72, each with a ``*_mbox_conf`` and a ``*_mbox_loc`` head (3 x 3, cout 2 and 4);
    conv3_3_norm_mbox_conf has cout 4: background = the maximum of its first three channels, face = the fourth.

The input is the RGB frame with its channels flipped to BGR and (104, 117, 123) subtracted per BGR channel, no division,
at its own size.

The tail (detect.py, bbox.py, sfd_detector.py), per frame: level i = 0..5 has stride s = 4 * 2^i; the face probability p
is the two-way softmax of (background, face); a position is a candidate where p > 0.05; its prior is (s/2 + x s,
s/2 + y s, 4 s, 4 s); with the variances (0.1, 0.2), cx = px + loc0 * 0.1 * pw, cy likewise, w = pw * exp(0.2 * loc2),
h likewise, and the box is (cx - w/2, cy - h/2, cx + w/2, cy + h/2); NMS is greedy over the candidates in descending
score, areas (x2 - x1 + 1)(y2 - y1 + 1), the intersection with the same + 1, a later candidate surviving a kept one
where ovr <= 0.3; the kept boxes with score > 0.5 are the detections, in descending score.  process.py takes the first
face, the reference's LMD meter the last.

**This project's rules**, where the package leaves a choice or a bound is needed:

  * the score is 1 / (1 + exp(bg - face)) in fp64 on the fp32 logits, rounded to fp32 (the package calls an fp32
    softmax); it is compared as fp32 with float32(0.05), and with 0.5;
  * the box decode and every NMS quantity are fp64 on the fp32 ``loc`` and score, as numpy promotes them in the package;
    the returned boxes are rounded to fp32;
  * ties in score go to the lower candidate index, candidates being numbered by level, then y, then x (numpy's reversed
    ``argsort`` leaves this unspecified);
  * at most ``MAX_CANDIDATES`` = 4096 candidates per frame enter the sort: the first 4096 in candidate-index order; a
    frame that has more sets its ``overflow`` flag (trained weights leave a few hundred);
  * at most ``MAX_FACES`` = 16 detections per frame are returned, the highest-scoring ones; the per-frame count is the
    true number;
  * H and W are multiples of 32 in [64, 4096] (the reference's frames are 512 x 512).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import convnet

MAX_CANDIDATES, MAX_FACES, N_LEVELS = 4096, 16, 6
MEAN_BGR = (104.0, 117.0, 123.0)
CANDIDATE_THRESHOLD, FACE_THRESHOLD, NMS_THRESHOLD = 0.05, 0.5, 0.3
VARIANCES = (0.1, 0.2)
MAX_SIDE = 4096
WORKSPACE_BUDGET = 1 << 30

# (convolution, no BatchNorm, bias, cin, cout, kernel, stride); fc6 pads 3, every other 3 x 3 pads 1
TRUNK = (("conv1_1", None, True, 3, 64, 3, 1), ("conv1_2", None, True, 64, 64, 3, 1),
         ("conv2_1", None, True, 64, 128, 3, 1), ("conv2_2", None, True, 128, 128, 3, 1),
         ("conv3_1", None, True, 128, 256, 3, 1), ("conv3_2", None, True, 256, 256, 3, 1), ("conv3_3", None, True, 256, 256, 3, 1),
         ("conv4_1", None, True, 256, 512, 3, 1), ("conv4_2", None, True, 512, 512, 3, 1), ("conv4_3", None, True, 512, 512, 3, 1),
         ("conv5_1", None, True, 512, 512, 3, 1), ("conv5_2", None, True, 512, 512, 3, 1), ("conv5_3", None, True, 512, 512, 3, 1),
         ("fc6", None, True, 512, 1024, 3, 1), ("fc7", None, True, 1024, 1024, 1, 1),
         ("conv6_1", None, True, 1024, 256, 1, 1), ("conv6_2", None, True, 256, 512, 3, 2),
         ("conv7_1", None, True, 512, 128, 1, 1), ("conv7_2", None, True, 128, 256, 3, 2))
LEVELS = (("conv3_3_norm", 256), ("conv4_3_norm", 512), ("conv5_3_norm", 512), ("fc7", 1024), ("conv6_2", 512), ("conv7_2", 256))
NORMS = (("conv3_3_norm", 256, 10.0), ("conv4_3_norm", 512, 8.0), ("conv5_3_norm", 512, 5.0))
HEADS = tuple(row for l, (name, ch) in enumerate(LEVELS)
              for row in ((f"{name}_mbox_conf", None, True, ch, 4 if l == 0 else 2, 3, 1), (f"{name}_mbox_loc", None, True, ch, 4, 3, 1)))
# the 31 convolutions of the state dict; struct instag_face_detect_weights holds the trunk and one packed head per level
LAYERS = TRUNK + HEADS
INDEX = {name: i for i, (name, *_) in enumerate(LAYERS)}


def level_sides(n: int):
    """The sides of the six levels along an axis of ``n`` pixels (a multiple of 32): n/4, n/8, n/16, then n/32 + 4 behind
    fc6's padding of 3 and the two stride-2 convolutions, (g - 1) // 2 + 1 each."""
    g = n // 32 + 4
    g6 = (g - 1) // 2 + 1
    return (n // 4, n // 8, n // 16, g, g6, (g6 - 1) // 2 + 1)


def check_size(who, H, W):
    if H < convnet.MIN_SIDE or W < convnet.MIN_SIDE or H % 32 or W % 32 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{who}: H and W multiples of 32 in [{convnet.MIN_SIDE}, {MAX_SIDE}], got {H} x {W}")


def macs_per_frame(H: int, W: int) -> int:
    """Multiply-accumulates of the 31 convolutions of one H x W frame, from the table."""
    hs, ws = level_sides(H), level_sides(W)
    side = {"conv1": (H, W), "conv2": (H // 2, W // 2), "conv3": (hs[0], ws[0]), "conv4": (hs[1], ws[1]),
            "conv5": (hs[2], ws[2]), "fc6": (hs[3], ws[3]), "fc7": (hs[3], ws[3]), "conv6_1": (hs[3], ws[3]),
            "conv6_2": (hs[4], ws[4]), "conv7_1": (hs[4], ws[4]), "conv7_2": (hs[5], ws[5])}
    total = 0
    for name, _, _, cin, cout, k, _ in TRUNK:
        h, w = side[name] if name in side else side[name.split("_")[0]]
        total += cin * cout * k * k * h * w                                        # output positions
    for l in range(N_LEVELS):
        for _, _, _, cin, cout, k, _ in HEADS[2 * l:2 * l + 2]:
            total += cin * cout * k * k * hs[l] * ws[l]
    return total


# ---- weights ----------------------------------------------------------------------------------------------------------
class S3FDWeights(convnet.ConvWeights):
    """The frozen parameters of S3FD under the package's key names (``conv1_1.weight``, ``fc6.bias``,
    ``conv3_3_norm.weight``, ``conv3_3_norm_mbox_conf.weight``, ``fc7_mbox_loc.bias``, ...): the 31 convolutions of
    ``LAYERS`` and the three L2Norm vectors (``norms``: name -> [C])."""

    TABLE, LABEL, STRUCT = LAYERS, "S3FD weights", "FaceDetectWeights"

    def __init__(self, layers, norms):
        super().__init__(layers)
        self.norms = {}
        for name, ch, _ in NORMS:
            if name not in norms:
                raise ValueError(f"{self.LABEL}: the L2Norm weight of {name} is missing")
            t = norms[name].detach().float().contiguous().cpu()
            if tuple(t.shape) != (ch,):
                raise ValueError(f"{self.LABEL}: {name} weight has shape {tuple(t.shape)}, expected {(ch,)}")
            self.norms[name] = t

    @classmethod
    def random(cls, seed: int = 0, conf_shift: float = 0.0, conf_gain: float = 1.0) -> "S3FDWeights":
        """Seeded stand-ins (tests, benches; convnet.draw_layer).  conv1_1 has gain 1/64, which brings the frame's values
        of about a hundred to about one for the He-scaled trunk behind it; the L2Norm weights are their initial scales
        times a factor in [0.5, 1.5].  ``conf_shift`` is added to the background bias of every conf head (level 0: its
        three background channels): it steers how many positions pass 0.05 -- the larger, the fewer.  ``conf_gain``
        scales the conf heads' weights: the wider the logits are spread, the larger the share of the candidates that
        are detections."""
        g = torch.Generator().manual_seed(seed)
        layers = [convnet.draw_layer(g, row, gain=1.0 / 64 if row[0] == "conv1_1" else 1.0) for row in LAYERS]
        for l in range(N_LEVELS):
            layers[len(TRUNK) + 2 * l]["weight"] *= conf_gain
            layers[len(TRUNK) + 2 * l]["bias"][:3 if l == 0 else 1] += conf_shift
        norms = {name: init * (torch.rand(ch, generator=g) + 0.5) for name, ch, init in NORMS}
        return cls(layers, norms)

    @classmethod
    def _extras(cls, sd):
        norms = {}
        for name, _, _ in NORMS:
            if f"{name}.weight" not in sd:
                raise ValueError(f"{cls.LABEL}: the state dict misses {name + '.weight'!r}")
            norms[name] = sd[f"{name}.weight"]
        return dict(norms=norms)

    @classmethod
    def from_state_dict(cls, sd):
        """``sd``: the package's keys (a ``{"state_dict": ...}`` wrapper and a ``module.`` prefix are taken off).  A
        missing key raises a ValueError naming it, a misshapen one names the layer and the field."""
        if "state_dict" in sd and not torch.is_tensor(sd["state_dict"]):
            sd = sd["state_dict"]
        if sd and all(k.startswith("module.") for k in sd):
            sd = {k[len("module."):]: v for k, v in sd.items()}
        return super().from_state_dict(sd)

    def state_dict(self):
        out = super().state_dict()
        out.update({f"{name}.weight": t.clone() for name, t in self.norms.items()})
        return out

    def to(self, device=None, dtype=None):
        out = super().to(device, dtype)
        out.update({name: {"weight": t.to(device=device, dtype=dtype)} for name, t in self.norms.items()})
        return out

    def device_pack(self, device):
        """The C struct for ``device``: the 19 trunk convolutions and one packed head per level as [K][cout] with
        (1, bias); conv1_1's input channels reversed (it reads RGB frames) and its K = 27 padded with zero rows to 32."""
        from . import _lib
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        pack = self._packs.get(key)
        if pack is not None:
            return pack
        convs = [(lay["weight"], lay["bias"]) for lay in self.layers[:len(TRUNK)]]
        convs[0] = (convs[0][0].flip(1), convs[0][1])
        for l in range(N_LEVELS):
            conf, loc = self.layers[len(TRUNK) + 2 * l], self.layers[len(TRUNK) + 2 * l + 1]
            convs.append((torch.cat((conf["weight"], loc["weight"])), torch.cat((conf["bias"], loc["bias"]))))
        keep, s = [], _lib.FaceDetectWeights()
        for l, (w, bias) in enumerate(convs):
            wk = w.reshape(w.shape[0], -1).t()
            rows = -(-wk.shape[0] // 32) * 32
            wk = torch.cat([wk, torch.zeros(rows - wk.shape[0], wk.shape[1])], dim=0)
            ts = [t.contiguous().to(device) for t in (wk, torch.ones_like(bias), bias)]
            keep += ts
            s.w[l], s.scale[l], s.shift[l] = [t.data_ptr() for t in ts]
        for i, (name, _, _) in enumerate(NORMS):
            t = self.norms[name].to(device)
            keep.append(t)
            s.norm[i] = t.data_ptr()
        pack = self._packs[key] = (s, keep)
        return pack


# ---- plain-torch statement: the network --------------------------------------------------------------------------------
def normalise_torch(frames_u8, dtype=torch.float32):
    """u8 RGB [B,H,W,3] -> [B,3,H,W] of ``dtype``: BGR minus (104, 117, 123)."""
    x = convnet.check_frames("face_detect", frames_u8, sides=False)[0]
    mean = torch.tensor(MEAN_BGR, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    return x.flip(-1).permute(0, 3, 1, 2).to(dtype) - mean


def l2norm_torch(x, weight):
    """[B,C,h,w], [C] -> x / (sqrt(sum_c x^2) + 1e-10) * weight[c]."""
    return x / (x.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10) * weight.view(1, -1, 1, 1)


def s3fd_torch(weights: S3FDWeights, x):
    """S3FD for ``x`` [B,3,H,W] (``normalise_torch``) -> the 12 maps (conf, loc) of level 0, .., (conf, loc) of level 5:
    conf [B,2,h,w] (level 0: [B,4,h,w]), loc [B,4,h,w]."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"face_detect: x [B,3,H,W], got {tuple(x.shape)}")
    check_size("face_detect", int(x.shape[2]), int(x.shape[3]))
    p = weights.to(x.device, x.dtype)

    def conv(name, t, relu=True, padding=None):
        k, stride = LAYERS[INDEX[name]][5:7]
        y = F.conv2d(t, p[name]["weight"], p[name]["bias"], stride=stride, padding=k // 2 if padding is None else padding)
        return F.relu(y) if relu else y

    def stage(names, t):
        for name in names:
            t = conv(name, t)
        return t

    f3 = stage(("conv3_1", "conv3_2", "conv3_3"),
               F.max_pool2d(stage(("conv2_1", "conv2_2"), F.max_pool2d(stage(("conv1_1", "conv1_2"), x), 2, 2)), 2, 2))
    f4 = stage(("conv4_1", "conv4_2", "conv4_3"), F.max_pool2d(f3, 2, 2))
    f5 = stage(("conv5_1", "conv5_2", "conv5_3"), F.max_pool2d(f4, 2, 2))
    f7 = conv("fc7", conv("fc6", F.max_pool2d(f5, 2, 2), padding=3))
    f6 = conv("conv6_2", conv("conv6_1", f7))
    f72 = conv("conv7_2", conv("conv7_1", f6))
    feats = [l2norm_torch(f, p[name]["weight"]) for f, (name, _, _) in zip((f3, f4, f5), NORMS)] + [f7, f6, f72]
    out = []
    for (name, _), f in zip(LEVELS, feats):
        out += [conv(f"{name}_mbox_conf", f, relu=False), conv(f"{name}_mbox_loc", f, relu=False)]
    return out


# ---- plain-torch statement: the tail -----------------------------------------------------------------------------------
def check_maps(maps, H, W):
    """The 12 maps of ``s3fd_torch`` for H x W frames -> B."""
    check_size("face_detect", H, W)
    if len(maps) != 2 * N_LEVELS:
        raise ValueError(f"face_detect: maps: 12 tensors (conf, loc per level), got {len(maps)}")
    B, hs, ws = int(maps[0].shape[0]), level_sides(H), level_sides(W)
    for i, m in enumerate(maps):
        want = (B, (4 if i == 0 else 2) if i % 2 == 0 else 4, hs[i // 2], ws[i // 2])
        if tuple(m.shape) != want:
            raise ValueError(f"face_detect: maps[{i}] has shape {tuple(m.shape)}, expected {want} for {H} x {W} frames")
    return B


def scores_torch(maps):
    """The 12 maps -> per level the face probability float32 [B,h,w]: 1 / (1 + exp(bg - face)) in fp64, rounded; level 0's
    background is the maximum of its first three conf channels."""
    out = []
    for l in range(N_LEVELS):
        conf = maps[2 * l]
        bg = conf[:, :3].max(dim=1).values if l == 0 else conf[:, 0]
        out.append((1.0 / (1.0 + torch.exp(bg.double() - conf[:, -1].double()))).float())
    return out


def candidates_torch(maps, H: int, W: int):
    """The 12 maps -> per frame (index int64 [n], score float32 [n], boxes float64 [n,4], overflow): the positions with
    score > float32(0.05) in candidate-index order (level, y, x), at most ``MAX_CANDIDATES`` of them, decoded in fp64."""
    B = check_maps(maps, H, W)
    scores = scores_torch(maps)
    thr = torch.tensor(CANDIDATE_THRESHOLD, dtype=torch.float32)
    out = []
    for b in range(B):
        idx, sc, boxes, start = [], [], [], 0
        for l in range(N_LEVELS):
            s = float(4 << l)
            p = scores[l][b]
            ys, xs = torch.nonzero(p > thr.to(p.device), as_tuple=True)          # row-major: y, then x
            loc = maps[2 * l + 1][b][:, ys, xs].double()
            px, py, pw = s / 2 + xs.double() * s, s / 2 + ys.double() * s, 4 * s
            cx, cy = px + loc[0] * VARIANCES[0] * pw, py + loc[1] * VARIANCES[0] * pw
            w, h = pw * torch.exp(VARIANCES[1] * loc[2]), pw * torch.exp(VARIANCES[1] * loc[3])
            boxes.append(torch.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), dim=1))
            idx.append(start + ys * p.shape[1] + xs)
            sc.append(p[ys, xs])
            start += p.numel()
        idx, sc, boxes = torch.cat(idx), torch.cat(sc), torch.cat(boxes)
        out.append((idx[:MAX_CANDIDATES], sc[:MAX_CANDIDATES], boxes[:MAX_CANDIDATES], int(idx.shape[0]) > MAX_CANDIDATES))
    return out


def overlap_torch(box, others):
    """ovr of one fp64 box [4] with fp64 boxes [n,4], with the + 1 of pixel boxes."""
    area = lambda t: (t[..., 2] - t[..., 0] + 1) * (t[..., 3] - t[..., 1] + 1)
    w = (torch.minimum(box[2], others[:, 2]) - torch.maximum(box[0], others[:, 0]) + 1).clamp(min=0)
    h = (torch.minimum(box[3], others[:, 3]) - torch.maximum(box[1], others[:, 1]) + 1).clamp(min=0)
    inter = w * h
    return inter / (area(box) + area(others) - inter)


def nms_torch(boxes, scores):
    """fp64 boxes [n,4] and float32 scores [n] in candidate order -> the kept candidates' positions in [0, n), in
    descending score (ties: the lower position)."""
    order = torch.argsort(-scores.double(), stable=True)
    keep = []
    while order.numel():
        i = order[0]
        keep.append(int(i))
        rest = order[1:]
        order = rest[overlap_torch(boxes[i], boxes[rest]) <= NMS_THRESHOLD]
    return torch.tensor(keep, dtype=torch.int64)


def post_torch(maps, H: int, W: int, details: bool = False, on_cpu: bool = True):
    """The 12 maps -> (boxes float32 [B,16,5] = (x1, y1, x2, y2, score), NaN-padded; count int32 [B]; overflow bool [B])
    on the maps' device; ``details``: also per frame the candidate indices of ALL its detections, in order.  The work is
    done on the CPU unless ``on_cpu`` is False: then the same torch operations run on the maps' device (the benchmark's
    torch chain)."""
    B = check_maps(maps, H, W)
    cpu = [m.detach().cpu() if on_cpu else m.detach() for m in maps]
    boxes = torch.full((B, MAX_FACES, 5), float("nan"), dtype=torch.float32)
    count, overflow, found = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.bool), []
    for b, (idx, sc, bx, over) in enumerate(candidates_torch(cpu, H, W)):
        keep = nms_torch(bx, sc).to(sc.device)
        keep = keep[sc[keep] > FACE_THRESHOLD]
        n = min(int(keep.shape[0]), MAX_FACES)
        boxes[b, :n, :4] = bx[keep[:n]].float().cpu()
        boxes[b, :n, 4] = sc[keep[:n]].cpu()
        count[b], overflow[b] = int(keep.shape[0]), over
        found.append(idx[keep].cpu())
    dev = maps[0].device
    out = (boxes.to(dev), count.to(dev), overflow.to(dev))
    return out + (found,) if details else out


@torch.no_grad()
def detect_torch(weights: S3FDWeights, frames_u8, dtype=torch.float32):
    """u8 RGB frames [N,H,W,3] -> ``post_torch``'s triple, the network on the frames' device in ``dtype``."""
    x, H, W = convnet.check_frames("face_detect", frames_u8)
    check_size("face_detect", H, W)
    return post_torch(s3fd_torch(weights, normalise_torch(x, dtype)), H, W)


def pick(boxes, count, last: bool = False):
    """``detect``'s boxes and count -> float32 [N,4]: the first (highest-scoring) detection of each frame, or the last of
    those returned; a NaN row where a frame has none."""
    n = count.to(boxes.device).long().clamp(max=MAX_FACES)
    row = (n - 1).clamp(min=0) if last else torch.zeros_like(n)
    out = boxes[torch.arange(boxes.shape[0], device=boxes.device), row, :4].clone()
    out[n == 0] = float("nan")
    return out


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class FaceDetector(convnet.FrameOperator):
    """S3FD over u8 RGB frames [N,H,W,3] on ``device`` through csrc/face_detect.hip, in chunks of at most ``max_batch``
    frames with one kept workspace (convnet.FrameOperator); a CPU device runs the statements.

      ``maps(frames)``            the 12 maps of ``s3fd_torch`` (views of the six packed tensors the kernels write)
      ``post(maps, H, W)``        the tail on given logits
      ``detect(frames)``          (boxes float32 [N,16,5] = (x1, y1, x2, y2, score), NaN-padded; count int32 [N];
                                  overflow bool [N])
      ``first(frames)`` / ``last(frames)``    float32 [N,4], a NaN row where there is no detection: what
                                  ``LandmarkNet.landmarks`` and ``landmarks_identity`` take (process.py reads ``[0]``,
                                  the reference's LMD meter ``[-1]``)

    ``max_batch=None``: the largest batch whose workspace at 512 x 512 (144 MiB per frame: the two full-resolution
    64-channel maps are 128 MiB of it) stays within 1 GiB, which is 7."""

    NAME = "face_detect"
    logits = labels = None                               # a detector has maps and boxes, no per-pixel logits or labels

    def __init__(self, weights: S3FDWeights, device="cuda", max_batch=None):
        super().__init__(weights, device, max_batch)
        if self.device.type == "cuda":
            from . import _lib
            bound = _lib.FACE_DETECT["INSTAG_FACE_DETECT_MAX_BATCH"]
            if max_batch is None:
                max_batch = max(1, min(bound, WORKSPACE_BUDGET // int(self._L.instag_face_detect_workspace_bytes(1, 512, 512))))
            if max_batch > bound:
                raise ValueError(f"FaceDetector: max_batch at most {bound}")
        self.max_batch = int(7 if max_batch is None else max_batch)

    def _workspace_bytes(self, batch, H, W):
        return self._L.instag_face_detect_workspace_bytes(batch, H, W)

    def _frames(self, frames_u8):
        x, H, W = convnet.check_frames(self.NAME, frames_u8)
        check_size(self.NAME, H, W)
        return x.to(self.device).contiguous(), H, W

    def _packed(self, B, H, W):
        hs, ws = level_sides(H), level_sides(W)
        return [torch.empty(B, 8 if l == 0 else 6, hs[l], ws[l], dtype=torch.float32, device=self.device)
                for l in range(N_LEVELS)]

    @staticmethod
    def _pointers(packed, c=slice(None)):
        return (C.c_void_p * N_LEVELS)(*[t[c].data_ptr() for t in packed])

    @torch.no_grad()
    def maps(self, frames_u8):
        x, H, W = self._frames(frames_u8)
        if self.device.type != "cuda":
            return s3fd_torch(self.weights, normalise_torch(x))
        from . import _lib
        packed = self._packed(int(x.shape[0]), H, W)
        self._chunks(x, H, W, lambda c, m, ws, nbytes: self._L.instag_face_detect_forward(
            C.byref(self._struct), _lib.ptr(x[c]), m, H, W, self._pointers(packed, c), ws, nbytes,
            _lib.current_stream()), "face_detect_forward")
        return [v for l, t in enumerate(packed) for v in (t[:, :4 if l == 0 else 2], t[:, 4 if l == 0 else 2:])]

    def _outputs(self, B):
        return (torch.empty(B, MAX_FACES, 5, dtype=torch.float32, device=self.device),
                torch.empty(B, dtype=torch.int32, device=self.device), torch.empty(B, dtype=torch.uint8, device=self.device))

    @torch.no_grad()
    def post(self, maps, H: int, W: int):
        B = check_maps(maps, H, W)
        if self.device.type != "cuda":
            return post_torch([m.to(self.device) for m in maps], H, W)
        from . import _lib
        packed = [torch.cat((maps[2 * l].to(self.device, torch.float32), maps[2 * l + 1].to(self.device, torch.float32)),
                            dim=1).contiguous() for l in range(N_LEVELS)]
        boxes, count, overflow = self._outputs(B)
        step = _lib.FACE_DETECT["INSTAG_FACE_DETECT_MAX_BATCH"]
        with torch.cuda.device(self.device):
            for i in range(0, B, step):
                c = slice(i, min(B, i + step))
                _lib.check_arg(self._L.instag_face_detect_post(
                    self._pointers(packed, c), c.stop - c.start, H, W, _lib.ptr(boxes[c]), _lib.ptr(count[c]),
                    _lib.ptr(overflow[c]), _lib.current_stream()), "face_detect_post")
        return boxes, count, overflow.bool()

    @torch.no_grad()
    def detect(self, frames_u8):
        x, H, W = self._frames(frames_u8)
        if self.device.type != "cuda":
            return detect_torch(self.weights, x)
        from . import _lib
        boxes, count, overflow = self._outputs(int(x.shape[0]))
        self._chunks(x, H, W, lambda c, m, ws, nbytes: self._L.instag_face_detect(
            C.byref(self._struct), _lib.ptr(x[c]), m, H, W, _lib.ptr(boxes[c]), _lib.ptr(count[c]), _lib.ptr(overflow[c]),
            ws, nbytes, _lib.current_stream()), "face_detect")
        return boxes, count, overflow.bool()

    def first(self, frames_u8):
        boxes, count, _ = self.detect(frames_u8)
        return pick(boxes, count)

    def last(self, frames_u8):
        boxes, count, _ = self.detect(frames_u8)
        return pick(boxes, count, last=True)


def pool_device(x, border: int = 0):
    """The 2 x 2 max-pool kernel alone (for the tests): fp32 [B,C,h,w] on the device -> [B,C,h/2 + 2 border, w/2 + 2 border]."""
    from . import _lib
    B, Cn, h, w = x.shape
    x = x.float().contiguous()
    out = torch.empty(B, Cn, h // 2 + 2 * border, w // 2 + 2 * border, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check_arg(_lib.lib().instag_face_detect_pool(_lib.ptr(x), _lib.ptr(out), B * Cn, h, w, int(border),
                                                          _lib.current_stream()), "face_detect_pool")
    return out


def l2norm_device(x, weight):
    """The L2Norm kernel alone (for the tests): fp32 [B,C,h,w] and [C] on the device -> [B,C,h,w]."""
    from . import _lib
    B, Cn, h, w = x.shape
    x, weight = x.float().contiguous(), weight.to(x.device, torch.float32).contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check_arg(_lib.lib().instag_face_detect_l2norm(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(out), B, Cn, h * w,
                                                            _lib.current_stream()), "face_detect_l2norm")
    return out


# ---- a directory --------------------------------------------------------------------------------------------------------
def detect_identity(path, weights: S3FDWeights, device="cuda", batch: int = 7, decoder=None):
    """ori_imgs/<i>.jpg of ``path`` in ascending numeric order -> float32 [N,4] on ``device``: each frame's first box, a
    NaN row where a frame has no detection.  ``decoder``: a ``jpeg_decode.JpegDecoder`` that decodes the files on the device
    (``convnet.frame_batches``)."""
    det = FaceDetector(weights, torch.device(device), max_batch=batch)
    out = [det.first(frames) for _, frames, _ in convnet.frame_batches(path, batch, decoder=decoder)]
    return torch.cat(out, dim=0) if out else torch.zeros(0, 4, device=det.device)
