"""Shared by the landmark tests and tests/golden/make_golden_landmarks.py (golden G19).

G19 stores no weights (FAN-2D-4 has 24 M of them): ``FANWeights.random(SEED)`` gives the state dict under the package's
keys; the generator loads it into the ``nn.Module`` classes below, the tests into ``FANWeights``.  The classes are a
second statement of the network, written in the layout of the package's models.py (modules registered under its names,
BatchNorm modules, ``torch.cat``), and ``crop_loops`` / ``decode_loops`` a second statement of the arithmetic around it,
per pixel and per landmark in Python integers and floats.  None of them shares code with instag_amd.landmarks.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import segnet_helpers as S
from tests.segnet_helpers import seeded_frames  # noqa: F401 (re-exported)

SEED = 19
G19_S = 64
G19_H, G19_W = 96, 80
G19_BOX = (-10.0, 20.0, 50.0, 90.0)                  # crosses the frame's left edge; its crop also leaves through the top
FACTOR = S.FACTOR
MAX_LEFT_OUT = 0.05


# ---- the network, in the package's layout ------------------------------------------------------------------------------
def conv3x3(in_planes, out_planes):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=1, padding=1, bias=False)


class ConvBlock(nn.Module):
    def __init__(self, in_planes, out_planes):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.conv1 = conv3x3(in_planes, out_planes // 2)
        self.bn2 = nn.BatchNorm2d(out_planes // 2)
        self.conv2 = conv3x3(out_planes // 2, out_planes // 4)
        self.bn3 = nn.BatchNorm2d(out_planes // 4)
        self.conv3 = conv3x3(out_planes // 4, out_planes // 4)
        self.downsample = None
        if in_planes != out_planes:
            self.downsample = nn.Sequential(nn.BatchNorm2d(in_planes), nn.ReLU(True),
                                            nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=1, bias=False))

    def forward(self, x):
        residual = x
        out1 = self.conv1(F.relu(self.bn1(x), True))
        out2 = self.conv2(F.relu(self.bn2(out1), True))
        out3 = self.conv3(F.relu(self.bn3(out2), True))
        out3 = torch.cat((out1, out2, out3), 1)
        if self.downsample is not None:
            residual = self.downsample(residual)
        out3 += residual
        return out3


class HourGlass(nn.Module):
    def __init__(self, depth, num_features):
        super().__init__()
        self.depth, self.features = depth, num_features
        self._generate_network(depth)

    def _generate_network(self, level):
        self.add_module("b1_" + str(level), ConvBlock(self.features, self.features))
        self.add_module("b2_" + str(level), ConvBlock(self.features, self.features))
        if level > 1:
            self._generate_network(level - 1)
        else:
            self.add_module("b2_plus_" + str(level), ConvBlock(self.features, self.features))
        self.add_module("b3_" + str(level), ConvBlock(self.features, self.features))

    def _forward(self, level, inp):
        up1 = self._modules["b1_" + str(level)](inp)
        low1 = F.avg_pool2d(inp, 2, stride=2)
        low1 = self._modules["b2_" + str(level)](low1)
        if level > 1:
            low2 = self._forward(level - 1, low1)
        else:
            low2 = self._modules["b2_plus_" + str(level)](low1)
        low3 = self._modules["b3_" + str(level)](low2)
        up2 = F.interpolate(low3, scale_factor=2, mode="nearest")
        return up1 + up2

    def forward(self, x):
        return self._forward(self.depth, x)


class FAN(nn.Module):
    def __init__(self, num_modules=4):
        super().__init__()
        self.num_modules = num_modules
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)
        self.bn1 = nn.BatchNorm2d(64)
        self.conv2 = ConvBlock(64, 128)
        self.conv3 = ConvBlock(128, 128)
        self.conv4 = ConvBlock(128, 256)
        for m in range(num_modules):
            self.add_module("m" + str(m), HourGlass(4, 256))
            self.add_module("top_m_" + str(m), ConvBlock(256, 256))
            self.add_module("conv_last" + str(m), nn.Conv2d(256, 256, kernel_size=1, stride=1, padding=0))
            self.add_module("bn_end" + str(m), nn.BatchNorm2d(256))
            self.add_module("l" + str(m), nn.Conv2d(256, 68, kernel_size=1, stride=1, padding=0))
            if m < num_modules - 1:
                self.add_module("bl" + str(m), nn.Conv2d(256, 256, kernel_size=1, stride=1, padding=0))
                self.add_module("al" + str(m), nn.Conv2d(68, 256, kernel_size=1, stride=1, padding=0))

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)), True)
        x = F.avg_pool2d(self.conv2(x), 2, stride=2)
        x = self.conv3(x)
        x = self.conv4(x)
        previous = x
        outputs = []
        for i in range(self.num_modules):
            hg = self._modules["m" + str(i)](previous)
            ll = self._modules["top_m_" + str(i)](hg)
            ll = F.relu(self._modules["bn_end" + str(i)](self._modules["conv_last" + str(i)](ll)), True)
            tmp_out = self._modules["l" + str(i)](ll)
            outputs.append(tmp_out)
            if i < self.num_modules - 1:
                ll = self._modules["bl" + str(i)](ll)
                tmp_out_ = self._modules["al" + str(i)](tmp_out)
                previous = previous + ll + tmp_out_
        return outputs


def state_dict(seed: int = SEED):
    from instag_amd.landmarks import FANWeights
    return FANWeights.random(seed).state_dict()


def weights(seed: int = SEED):
    from instag_amd.landmarks import FANWeights
    return FANWeights.from_state_dict(state_dict(seed))


def module(seed: int = SEED, dtype=torch.float64):
    net = FAN(4).to(dtype)
    net.load_state_dict(state_dict(seed), strict=True)
    return net.eval()


# ---- around the network, in loops --------------------------------------------------------------------------------------
def _inverse(p, c, h, res):
    return math.trunc(p * h / res + c - h / 2.0)


def _center_scale(box):
    x1, y1, x2, y2 = (float(np.float32(v)) for v in box)
    return x2 - (x2 - x1) / 2.0, y2 - (y2 - y1) / 2.0 - 0.12 * (y2 - y1), 200.0 * ((x2 - x1 + y2 - y1) / 195.0)


def crop_loops(frame, box, S):
    """u8 [H,W,3] -> u8 [S,S,3], pixel by pixel in Python integers."""
    H, W = frame.shape[:2]
    cx, cy, h = _center_scale(box)
    ulx, uly = _inverse(1.0, cx, h, 256.0), _inverse(1.0, cy, h, 256.0)
    cw, ch = _inverse(256.0, cx, h, 256.0) - ulx, _inverse(256.0, cy, h, 256.0) - uly
    out = np.zeros((S, S, 3), dtype=np.uint8)
    if cw < 1 or ch < 1:
        return out

    def source(y, x, c):
        fy, fx = y + uly, x + ulx
        return int(frame[fy, fx, c]) if 0 <= fy < H and 0 <= fx < W else 0

    def axis(o, n):
        num = (2 * o + 1) * n - S
        fl = num // (2 * S)
        return min(max(fl, 0), n - 1), min(max(fl + 1, 0), n - 1), ((num - fl * 2 * S) * 512 + S) // (2 * S)

    for oy in range(S):
        y0, y1, wy = axis(oy, ch)
        for ox in range(S):
            x0, x1, wx = axis(ox, cw)
            for c in range(3):
                total = (512 - wy) * ((512 - wx) * source(y0, x0, c) + wx * source(y0, x1, c)) \
                    + wy * ((512 - wx) * source(y1, x0, c) + wx * source(y1, x1, c))
                out[oy, ox, c] = (total + (1 << 17)) >> 18
    return out


def decode_loops(heat, box):
    """[68,R,R] -> float32 [68,2], landmark by landmark as the package's loop goes."""
    P, R, _ = heat.shape
    cx, cy, h = _center_scale(box)
    out = np.zeros((P, 2), dtype=np.float32)
    for j in range(P):
        idx = int(np.argmax(heat[j].reshape(-1))) + 1                   # numpy's argmax is the first maximum
        px, py = (idx - 1) % R + 1, (idx - 1) // R + 1                  # 1-based
        x, y = float(px), float(py)
        pX, pY = px - 1, py - 1
        if 0 < pX < R - 1 and 0 < pY < R - 1:
            x += 0.25 * float(np.sign(heat[j, pY, pX + 1] - heat[j, pY, pX - 1]))
            y += 0.25 * float(np.sign(heat[j, pY + 1, pX] - heat[j, pY - 1, pX]))
        out[j] = (_inverse(x - 0.5, cx, h, float(R)), _inverse(y - 0.5, cy, h, float(R)))
    return out


# ---- the GPU tests' cases ----------------------------------------------------------------------------------------------
def seeded_crops(B: int, S_: int, seed: int = 0):
    """u8 [B,S,S,3]: ``seeded_frames``, every crop with its own phase."""
    return seeded_frames(B, S_, S_, seed)


def case(weights_, crops):
    """The fp64 statement's heatmaps of all four stacks [B,4,68,R,R], e32 and the scale per stack (e32 = the fp32 CPU
    statement's largest error relative to the stack's largest fp64 entry), and the flip-risk (face, landmark) pairs of
    the last stack: top-two margin, or a neighbour difference the decode's shift reads, below 2 x FACTOR x e32 x scale."""
    from instag_amd import landmarks as L
    with torch.no_grad():
        want = L.fan_torch(weights_, L.normalise(crops, torch.float64), all_stacks=True)
        got32 = L.fan_torch(weights_, L.normalise(crops, torch.float32), all_stacks=True)
    scale = [float(want[:, i].abs().max()) for i in range(4)]
    e32 = [float((got32[:, i].double() - want[:, i]).abs().max()) / scale[i] for i in range(4)]
    for e in e32:
        assert 1e-8 < e < 2e-5, e32
    last = want[:, 3]
    B, P, R, _ = last.shape
    flat = last.reshape(B, P, R * R)
    top = flat.topk(2, dim=2)
    bar = 2.0 * FACTOR * e32[3] * scale[3]
    risk = (top.values[..., 0] - top.values[..., 1]) < bar
    arg = top.indices[..., 0]
    py, px = arg // R, arg % R
    inside = (px > 0) & (px < R - 1) & (py > 0) & (py < R - 1)
    pad = F.pad(last, (1, 1, 1, 1))
    at = lambda dy, dx: pad.reshape(B, P, -1).gather(2, ((py + 1 + dy) * (R + 2) + px + 1 + dx)[..., None])[..., 0]
    risk |= inside & (((at(0, 1) - at(0, -1)).abs() < bar) | ((at(1, 0) - at(-1, 0)).abs() < bar))
    return dict(weights=weights_, crops=crops, want=want, e32=e32, scale=scale, risk=risk, arg=arg, arg32=got32[:, 3].reshape(B, P, -1).argmax(dim=2))


def check_heatmaps(name, got, c, record=None):
    """All four stacks within FACTOR x e32 of the fp64 statement, each relative to its own scale; prints first."""
    assert tuple(got.shape) == tuple(c["want"].shape) and got.dtype == torch.float32 and got.is_cuda
    errs = [float((got[:, i].double().cpu() - c["want"][:, i]).abs().max()) / c["scale"][i] for i in range(4)]
    for i in range(4):
        print(f"{name} stack {i}: operator {errs[i]:.3e} e32 {c['e32'][i]:.3e} bar {FACTOR * c['e32'][i]:.3e} "
              f"scale {c['scale'][i]:.3e}")
    if record is not None:
        record[name] = dict(operator=errs, e32=c["e32"], scale=c["scale"])
    for i in range(4):
        assert errs[i] <= FACTOR * c["e32"][i], (name, i, errs[i], c["e32"][i])
    return errs


# ---- crafted cases of the crop and the decode (host and GPU tests) -----------------------------------------------------
CROP_SIDE = 128                                      # the frames of the crop cases are 128 x 128, the crops 64 x 64
# name -> box.  With w + h = 78 the scale is 0.4 and the (br - ul) image has 80 pixels a side (79 where ul < 0: the
# truncation is toward zero), with 39 it has 40, with 62.4 it has 64 = S and the resize is the identity.
CROP_BOXES = {
    "inside_larger": (44.0, 50.0, 84.0, 88.0),       # ul = (24, 24), br = (104, 104)
    "inside_smaller": (54.0, 57.0, 74.0, 76.0),      # ul = (44, 44), br = (84, 84)
    "identity": (48.5, 53.1, 80.5, 83.5),            # ul = (32, 32), br = (96, 96)
    "left": (-16.0, 50.0, 24.0, 88.0),               # ul_x = trunc(-35.69) = -35, br_x = 44
    "right": (104.0, 50.0, 144.0, 88.0),             # ul_x = 84, br_x = 164 > 128
    "top": (44.0, -10.0, 84.0, 28.0),                # ul_y = trunc(-35.25) = -35, br_y = 44
    "bottom": (44.0, 110.0, 84.0, 148.0),            # ul_y = 84, br_y = 164
    "outside": (300.0, 300.0, 340.0, 338.0),
    "reversed": (84.0, 88.0, 44.0, 50.0),            # a negative scale: br - ul < 1, a zero crop
    "nan": (float("nan"), 50.0, 84.0, 88.0),
}


def crop_frames():
    """u8 [len(CROP_BOXES),128,128,3], every frame different, and the boxes float32 [.,4] in the dict's order."""
    frames = seeded_frames(len(CROP_BOXES), CROP_SIDE, CROP_SIDE, seed=SEED + 1)
    return frames, torch.tensor(list(CROP_BOXES.values()), dtype=torch.float32)


DECODE_R = 16
DECODE_BOXES = ((10.0, 0.0, 110.0, 95.0),            # scale 1: centre (60, 36.1), h = 200
                (-300.0, -280.0, -200.0, -185.0))    # scale 1 again, every coordinate negative
# landmark -> ((py, px) of the peak, sign of the x difference, sign of the y difference) the crafted maps give
DECODE_PEAKS = {0: ((0, 5), 1, 1), 1: ((15, 5), 1, 1), 2: ((5, 0), 1, 1), 3: ((5, 15), 1, 1),          # borders: no shift
                4: ((7, 7), 1, 1), 5: ((7, 7), 1, -1), 6: ((7, 7), -1, 1), 7: ((7, 7), -1, -1),
                8: ((7, 7), 0, 0), 9: ((3, 4), 1, -1)}                                                # 9: a tie with (9, 2)


def decode_heatmaps():
    """fp32 [2,68,16,16] in sixty-fourths: a low seeded floor, one peak of 10 per map (``DECODE_PEAKS`` for the first ten,
    seeded interior cells for the rest), neighbours of 5 and 3 that fix the signs of the differences."""
    g = torch.Generator().manual_seed(SEED + 2)
    R = DECODE_R
    hm = (torch.rand(2, 68, R, R, generator=g) * 64).floor() / 64
    for b in range(2):
        for j in range(68):
            if j in DECODE_PEAKS:
                (py, px), sx, sy = DECODE_PEAKS[j]
            else:
                py, px = (int(v) for v in torch.randint(1, R - 1, (2,), generator=g))
                sx, sy = (int(v) for v in torch.randint(-1, 2, (2,), generator=g))
            hm[b, j, py, px] = 10.0
            for (dy, dx), s in (((0, 1), sx), ((1, 0), sy)):
                hi, lo = (py + dy, px + dx), (py - dy, px - dx)
                for cell, v in ((hi, 5.0 if s > 0 else 3.0), (lo, 5.0 if s < 0 else 3.0)):
                    if 0 <= cell[0] < R and 0 <= cell[1] < R:
                        hm[b, j, cell[0], cell[1]] = v
        hm[b, 9, 9, 2] = 10.0                                                     # the tie: the first maximum is (3, 4)
    return hm, torch.tensor(DECODE_BOXES, dtype=torch.float32)
