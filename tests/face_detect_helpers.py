"""Shared by the face detector's tests and tests/golden/make_golden_face_detect.py (golden G20).

G20 stores no weights (S3FD has 22 M of them): ``S3FDWeights.random(SEED)`` gives the state dict under the package's
keys; the generator loads it into the ``nn.Module`` below, the tests into ``S3FDWeights``.  The module is a second
statement of the network, written in the layout of the package's net_s3fd.py (one ``nn.Conv2d`` per name, an ``L2Norm``
module, ``F.max_pool2d``), and ``tail_loops`` / ``nms_loop`` a second statement of the tail: per position in Python floats,
the suppression as the package's numpy loop.  None of them shares code with instag_amd.face_detect.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import segnet_helpers as S
from tests.segnet_helpers import seeded_frames  # noqa: F401 (re-exported)

SEED = 20
G20_H, G20_W = 64, 96
FACTOR = S.FACTOR
MAX_CANDIDATES, MAX_FACES = 4096, 16
OFF = 10.0                                           # a background logit this far above the face's: p = 4.5e-5


E2E_SEED, E2E_SHIFT, E2E_GAIN = 70, 4.0, 2.0         # the end-to-end case, chosen on the CPU (flip_margins)
RISK = 10.0                                          # a decision is safe with this many times the operator's bar to spare


def weights(conf_shift: float = 0.0, seed: int = SEED, conf_gain: float = 1.0):
    from instag_amd.face_detect import S3FDWeights
    return S3FDWeights.random(seed, conf_shift=conf_shift, conf_gain=conf_gain)


# ---- the network, in the package's layout ------------------------------------------------------------------------------
class L2Norm(nn.Module):
    def __init__(self, n_channels, scale=1.0):
        super().__init__()
        self.eps = 1e-10
        self.weight = nn.Parameter(torch.full((n_channels,), float(scale)))

    def forward(self, x):
        norm = x.pow(2).sum(dim=1, keepdim=True).sqrt() + self.eps
        return x / norm * self.weight.view(1, -1, 1, 1)


class S3FDNet(nn.Module):
    def __init__(self):
        super().__init__()
        c = lambda i, o, k=3, s=1, p=1: nn.Conv2d(i, o, kernel_size=k, stride=s, padding=p)
        self.conv1_1, self.conv1_2 = c(3, 64), c(64, 64)
        self.conv2_1, self.conv2_2 = c(64, 128), c(128, 128)
        self.conv3_1, self.conv3_2, self.conv3_3 = c(128, 256), c(256, 256), c(256, 256)
        self.conv4_1, self.conv4_2, self.conv4_3 = c(256, 512), c(512, 512), c(512, 512)
        self.conv5_1, self.conv5_2, self.conv5_3 = c(512, 512), c(512, 512), c(512, 512)
        self.fc6 = c(512, 1024, 3, 1, 3)
        self.fc7 = c(1024, 1024, 1, 1, 0)
        self.conv6_1, self.conv6_2 = c(1024, 256, 1, 1, 0), c(256, 512, 3, 2, 1)
        self.conv7_1, self.conv7_2 = c(512, 128, 1, 1, 0), c(128, 256, 3, 2, 1)
        self.conv3_3_norm, self.conv4_3_norm, self.conv5_3_norm = L2Norm(256, 10), L2Norm(512, 8), L2Norm(512, 5)
        self.conv3_3_norm_mbox_conf, self.conv3_3_norm_mbox_loc = c(256, 4), c(256, 4)
        self.conv4_3_norm_mbox_conf, self.conv4_3_norm_mbox_loc = c(512, 2), c(512, 4)
        self.conv5_3_norm_mbox_conf, self.conv5_3_norm_mbox_loc = c(512, 2), c(512, 4)
        self.fc7_mbox_conf, self.fc7_mbox_loc = c(1024, 2), c(1024, 4)
        self.conv6_2_mbox_conf, self.conv6_2_mbox_loc = c(512, 2), c(512, 4)
        self.conv7_2_mbox_conf, self.conv7_2_mbox_loc = c(256, 2), c(256, 4)

    def forward(self, x):
        h = F.relu(self.conv1_1(x)); h = F.relu(self.conv1_2(h)); h = F.max_pool2d(h, 2, 2)
        h = F.relu(self.conv2_1(h)); h = F.relu(self.conv2_2(h)); h = F.max_pool2d(h, 2, 2)
        h = F.relu(self.conv3_1(h)); h = F.relu(self.conv3_2(h)); h = F.relu(self.conv3_3(h)); f3_3 = h
        h = F.max_pool2d(h, 2, 2)
        h = F.relu(self.conv4_1(h)); h = F.relu(self.conv4_2(h)); h = F.relu(self.conv4_3(h)); f4_3 = h
        h = F.max_pool2d(h, 2, 2)
        h = F.relu(self.conv5_1(h)); h = F.relu(self.conv5_2(h)); h = F.relu(self.conv5_3(h)); f5_3 = h
        h = F.max_pool2d(h, 2, 2)
        h = F.relu(self.fc6(h)); h = F.relu(self.fc7(h)); ffc7 = h
        h = F.relu(self.conv6_1(h)); h = F.relu(self.conv6_2(h)); f6_2 = h
        h = F.relu(self.conv7_1(h)); h = F.relu(self.conv7_2(h)); f7_2 = h
        f3_3, f4_3, f5_3 = self.conv3_3_norm(f3_3), self.conv4_3_norm(f4_3), self.conv5_3_norm(f5_3)
        return [self.conv3_3_norm_mbox_conf(f3_3), self.conv3_3_norm_mbox_loc(f3_3),
                self.conv4_3_norm_mbox_conf(f4_3), self.conv4_3_norm_mbox_loc(f4_3),
                self.conv5_3_norm_mbox_conf(f5_3), self.conv5_3_norm_mbox_loc(f5_3),
                self.fc7_mbox_conf(ffc7), self.fc7_mbox_loc(ffc7),
                self.conv6_2_mbox_conf(f6_2), self.conv6_2_mbox_loc(f6_2),
                self.conv7_2_mbox_conf(f7_2), self.conv7_2_mbox_loc(f7_2)]


def module(w=None, dtype=torch.float64):
    """The module in eval mode with ``w``'s (default: the seeded) state dict loaded strictly."""
    net = S3FDNet()
    net.load_state_dict((w or weights()).state_dict(), strict=True)
    return net.to(dtype).eval()


def bgr_input(frames_u8, dtype=torch.float64):
    """u8 RGB [B,H,W,3] -> the module's input: BGR minus (104, 117, 123), [B,3,H,W]."""
    x = torch.as_tensor(np.asarray(frames_u8)[..., ::-1].copy()).to(dtype)
    return (x - torch.tensor([104.0, 117.0, 123.0], dtype=dtype)).permute(0, 3, 1, 2)


# ---- the tail, position by position ------------------------------------------------------------------------------------
def nms_loop(dets, thresh):
    """The package's loop over [n,5] = (x1, y1, x2, y2, score) -> the kept rows, the order's ties to the lower row."""
    if len(dets) == 0:
        return []
    x1, y1, x2, y2, scores = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = np.lexsort((np.arange(len(dets)), -scores))
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        xx1, yy1 = np.maximum(x1[i], x1[order[1:]]), np.maximum(y1[i], y1[order[1:]])
        xx2, yy2 = np.minimum(x2[i], x2[order[1:]]), np.minimum(y2[i], y2[order[1:]])
        w, h = np.maximum(0.0, xx2 - xx1 + 1), np.maximum(0.0, yy2 - yy1 + 1)
        ovr = w * h / (areas[i] + areas[order[1:]] - w * h)
        inds = np.where(ovr <= thresh)[0]
        order = order[inds + 1]
    return keep


def tail_loops(maps, b: int = 0):
    """The 12 maps (arrays or tensors, [B,C,h,w]) -> frame ``b``'s candidates and detections as a dict: ``index`` int64
    [n], ``score`` float32 [n], ``boxes`` float64 [n,4] (at most 4096, in index order), ``overflow``, and of ALL the
    detections in order ``det_index``, ``det_score`` float32, ``det_boxes`` float64."""
    maps = [np.asarray(m[b].detach().cpu() if torch.is_tensor(m) else m[b]) for m in maps]
    index, score, boxes, start, seen = [], [], [], 0, 0
    thr = float(np.float32(0.05))
    for level in range(6):
        conf, loc = maps[2 * level], maps[2 * level + 1]
        stride = 4 * 2 ** level
        for y in range(conf.shape[1]):
            for x in range(conf.shape[2]):
                if level == 0:
                    bg, face = max(float(conf[0, y, x]), float(conf[1, y, x]), float(conf[2, y, x])), float(conf[3, y, x])
                else:
                    bg, face = float(conf[0, y, x]), float(conf[1, y, x])
                try:
                    p = float(np.float32(1.0 / (1.0 + math.exp(bg - face))))
                except OverflowError:
                    p = 0.0
                if p > thr:
                    seen += 1
                    if len(index) < MAX_CANDIDATES:
                        px, py, pw = stride / 2 + x * stride, stride / 2 + y * stride, 4 * stride
                        cx = px + float(loc[0, y, x]) * 0.1 * pw
                        cy = py + float(loc[1, y, x]) * 0.1 * pw
                        w = pw * math.exp(0.2 * float(loc[2, y, x]))
                        h = pw * math.exp(0.2 * float(loc[3, y, x]))
                        index.append(start + y * conf.shape[2] + x)
                        score.append(p)
                        boxes.append((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2))
        start += conf.shape[1] * conf.shape[2]
    index, score = np.asarray(index, dtype=np.int64), np.asarray(score, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    keep = nms_loop(np.concatenate((boxes, score.astype(np.float64)[:, None]), axis=1), 0.3)
    keep = np.asarray([k for k in keep if score[k] > 0.5], dtype=np.int64)
    return dict(index=index, score=score, boxes=boxes, overflow=seen > MAX_CANDIDATES, det_index=index[keep],
                det_score=score[keep], det_boxes=boxes[keep])


def overlaps(t):
    """Every overlap the greedy loop evaluates on ``tail_loops``' candidates and the gaps between consecutive sorted
    scores: what a flip-risk check needs.  -> (ovr values, sorted scores)."""
    dets = np.concatenate((t["boxes"], t["score"].astype(np.float64)[:, None]), axis=1)
    out = []
    if len(dets):
        x1, y1, x2, y2 = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3]
        areas = (x2 - x1 + 1) * (y2 - y1 + 1)
        order = np.lexsort((np.arange(len(dets)), -dets[:, 4]))
        while order.size > 0:
            i, rest = order[0], order[1:]
            w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
            h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
            ovr = w * h / (areas[i] + areas[rest] - w * h)
            out.append(ovr)
            order = rest[ovr <= 0.3]
    return (np.concatenate(out) if out else np.zeros(0)), np.sort(t["score"].astype(np.float64))[::-1]


def flip_margins(maps64, maps32, b):
    """What could flip a decision of frame ``b``'s tail under the error the map test allows the operator: name ->
    (smallest margin the fp64 statement shows, margin required).  The operator's logits may be off by FACTOR x e32 x
    the map's largest entry = FACTOR x (the fp32 statement's largest error in that map); ``err_conf`` / ``err_loc`` is the
    largest such error over the conf / loc maps.  A score moves by at most 1/4 per unit of (bg - face), two logits, so
    its scale is err_conf / 2: that holds for |p - 0.05|, for a detection's |p - 0.5| and for the gap between
    consecutive sorted scores.  A box edge moves by at most 0.1 pw + 0.1 w per unit of loc, a tenth to a fifth of the
    box's side, and ovr by at most the summed relative moves of the eight edges involved, so its scale is 2 err_loc.
    Required is RISK x FACTOR x that scale."""
    err = lambda which: max(float((a.double() - w).abs().max()) for a, w in zip(maps32[which::2], maps64[which::2]))
    need_p, need_ovr = RISK * FACTOR * err(0) / 2, RISK * FACTOR * 2 * err(1)
    t = tail_loops(maps64, b)
    ovr, ss = overlaps(t)
    sc, det = t["score"].astype(np.float64), t["det_score"].astype(np.float64)
    big = float("inf")
    return {"p - 0.05": (float(np.abs(sc - 0.05).min()) if len(sc) else big, need_p),
            "p - 0.5": (float(np.abs(det - 0.5).min()) if len(det) else big, need_p),
            "score gap": (float(np.min(-np.diff(ss))) if len(ss) > 1 else big, need_p),
            "ovr - 0.3": (float(np.abs(ovr - 0.3).min()) if len(ovr) else big, need_ovr)}


# ---- crafted logits ----------------------------------------------------------------------------------------------------
def level_sides(n):
    g = n // 32 + 4
    g6 = (g - 1) // 2 + 1
    return [n // 4, n // 8, n // 16, g, g6, (g6 - 1) // 2 + 1]


def blank_maps(B, H, W):
    """12 float32 maps for H x W frames with no candidate: every background logit ``OFF``, every other entry 0."""
    hs, ws, out = level_sides(H), level_sides(W), []
    for level in range(6):
        conf = torch.zeros(B, 4 if level == 0 else 2, hs[level], ws[level])
        conf[:, 0] = OFF
        out += [conf, torch.zeros(B, 4, hs[level], ws[level])]
    return out


def put(maps, b, level, y, x, diff, loc=(0.0, 0.0, 0.0, 0.0)):
    """Position (level, y, x) of frame ``b`` gets bg - face = ``diff`` (a float32) and the given loc."""
    conf = maps[2 * level]
    conf[b, :, y, x] = 0.0
    if level == 0:
        conf[b, 1, y, x] = float(diff)                # the maximum of the three is the middle one
        conf[b, 0, y, x] = float(diff) - 1.0
        conf[b, 2, y, x] = float(diff) - 3.0
    else:
        conf[b, 0, y, x] = float(diff)
    maps[2 * level + 1][b, :, y, x] = torch.tensor(loc, dtype=torch.float32)


def diff_for(p: float) -> np.float32:
    """The float32 ``bg - face`` whose score is nearest to ``p``."""
    return np.float32(math.log(1.0 / p - 1.0))


def score32(diff) -> np.float32:
    return np.float32(1.0 / (1.0 + math.exp(float(np.float32(diff)))))


def logits_for(target) -> tuple:
    """(bg, face) float32 whose fp64 score rounds to exactly the float32 ``target``: bg is the float32 nearest the
    wanted difference and the tiny face logit takes the remainder, which the fp64 subtraction keeps."""
    t = float(np.float32(target))
    want = math.log(1.0 / t - 1.0)
    bg = np.float32(want)
    face = np.float32(float(bg) - want)
    assert np.float32(1.0 / (1.0 + math.exp(float(bg) - float(face)))) == np.float32(target)
    return float(bg), float(face)


def put_pair(maps, b, level, y, x, bg, face):
    """Position (level, y, x) of frame ``b`` gets these two logits (level 0: the background through channel 1)."""
    conf = maps[2 * level]
    if level == 0:
        conf[b, :, y, x] = torch.tensor([bg - 1.0, bg, bg - 3.0, face])
    else:
        conf[b, :, y, x] = torch.tensor([bg, face])


# the first candidate index of each level of a 64 x 64 frame (sides 16, 8, 4, 6, 3, 2) and of a 512 x 512 one
START_64 = (0, 256, 320, 336, 372, 381)
START_512 = (0, 16384, 20480, 21504, 21904, 22004)
F05 = np.float32(0.05)


def tail_cases():
    """The crafted logits of the tail's tests: name -> (maps, H, W, expected), ``expected`` worked out by hand:
    ``count`` and ``overflow`` per frame and, where given, ``index`` (the candidate indices of all detections in
    order, per frame) and ``boxes`` (frame 0's first box in fp64)."""
    out = {}

    # one candidate at level 1 (stride 8, prior 32 x 32 around (4 + 8 x, 4 + 8 y)), position (2, 3): index 256 + 2 * 8 + 3
    m = blank_maps(1, 64, 64)
    put(m, 0, 1, 2, 3, -2.0, (0.5, -0.25, 5.0, -5.0))
    cx, cy, w, h = 28 + 0.5 * 0.1 * 32, 20 - 0.25 * 0.1 * 32, 32 * math.exp(1.0), 32 * math.exp(-1.0)
    out["single"] = (m, 64, 64, dict(count=[1], overflow=[False], index=[[275]], score=1.0 / (1.0 + math.exp(-2.0)),
                                     boxes=(cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)))

    # level 0's background is the maximum of three channels: (1, -1, 3) against 2.5 is p = 0.38, (-2, -1, -3) against 0 is
    # p = 0.73; with the first channel alone the first position would be the higher detection
    m = blank_maps(1, 64, 64)
    m[0][0, :, 1, 2] = torch.tensor([1.0, -1.0, 3.0, 2.5])
    m[0][0, :, 5, 9] = torch.tensor([-2.0, -1.0, -3.0, 0.0])
    out["maxout"] = (m, 64, 64, dict(count=[1], overflow=[False], index=[[5 * 16 + 9]]))

    # 0.5: p = 0.5 exactly (equal logits) and just below it are no detections, just above it is one; all at level 2
    m = blank_maps(1, 64, 64)
    put(m, 0, 2, 0, 0, 0.0)
    put(m, 0, 2, 0, 3, 1e-6)
    put(m, 0, 2, 3, 0, -1e-6)
    out["half"] = (m, 64, 64, dict(count=[1], overflow=[False], index=[[320 + 3 * 4]]))

    # ovr on both sides of 0.3: two 32 x 32 boxes of level 1, the second 17 px to the right (ovr = 16 * 33 / 1650 = 0.32,
    # suppressed) in frame 0 and 18.5 px (14.5 * 33 / 1699.5 = 0.28, kept) in frame 1
    m = blank_maps(2, 64, 64)
    for b, loc0 in ((0, 0.3125), (1, 0.78125)):
        put(m, b, 1, 1, 0, -3.0)
        put(m, b, 1, 1, 2, -2.0, (loc0, 0.0, 0.0, 0.0))
    out["overlap"] = (m, 64, 64, dict(count=[1, 2], overflow=[False, False], index=[[264], [264, 266]]))

    # equal scores: of two overlapping positions (8 px apart, ovr = 0.61) the lower index is kept; two that do not
    # overlap come out in index order, behind a higher score at a later index
    m = blank_maps(1, 64, 64)
    put(m, 0, 1, 0, 0, -1.0)
    put(m, 0, 1, 0, 1, -1.0)
    put(m, 0, 1, 7, 7, -1.0)
    put(m, 0, 2, 3, 3, -4.0)
    out["tie"] = (m, 64, 64, dict(count=[3], overflow=[False], index=[[335, 256, 319]]))

    out["empty"] = (blank_maps(2, 64, 64), 64, 64, dict(count=[0, 0], overflow=[False, False], index=[[], []]))

    # 20 detections: level-0 boxes (16 x 16) 12 px apart overlap by 5 * 17 / 493 = 0.17; the scores rise with k
    m = blank_maps(1, 64, 64)
    spots = [(y, x) for y in (0, 3, 6, 9, 12, 15) for x in (0, 3, 6, 9, 12, 15)][:20]
    for k, (y, x) in enumerate(spots):
        put(m, 0, 0, y, x, -1.0 - 0.1 * k)
    out["many"] = (m, 64, 64, dict(count=[20], overflow=[False], index=[[y * 16 + x for y, x in reversed(spots)]]))

    # the cap, on the 128 x 128 level 0 of a 512 x 512 frame: the first 32 rows are 4096 candidates with p = 0.6, and one
    # more position decides the overflow flag: p exactly float32(0.05) and the float32 below it are no candidates, the
    # float32 above it is the 4097th
    base = blank_maps(1, 512, 512)
    base[0][0, :, :32, :] = torch.tensor([-1.0, math.log(1 / 0.6 - 1), -3.0, 0.0]).view(4, 1, 1)
    for name, target, over in (("cap at 0.05", F05, False), ("cap below 0.05", np.nextafter(F05, np.float32(0)), False),
                               ("cap above 0.05", np.nextafter(F05, np.float32(1)), True)):
        m = [t.clone() for t in base]
        put_pair(m, 0, 3, 5, 5, *logits_for(target))
        out[name] = (m, 512, 512, dict(count=None, overflow=[over]))
    # every position of level 0 a candidate: the first 4096 enter, the detections lie in the first 32 rows
    m = [t.clone() for t in base]
    m[0][0, :, :, :] = torch.tensor([-1.0, math.log(1 / 0.6 - 1), -3.0, 0.0]).view(4, 1, 1)
    out["cap all"] = (m, 512, 512, dict(count=None, overflow=[True]))
    return out


def within_one_ulp(got, want64):
    """float32 ``got`` against the fp64 values rounded to float32: at most one float32 step apart."""
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))
