"""Golden G21: the project's Sapiens statement pinned to a second statement that shares no code with it.

    python tests/golden/make_golden_sapiens.py        # writes tests/golden/g21_sapiens.npz (CPU)

The second statement is an ``nn.Module`` in the release's layout -- ``nn.Conv2d(3, hidden, 16, 16, padding=2)``, a learned
``pos_embed``, blocks of ``nn.LayerNorm`` / a Linear ``qkv`` with an explicit softmax / ``proj`` / an FFN of nested
Sequentials, ``nn.ConvTranspose2d(4, 2, 1, bias=False)``, ``nn.InstanceNorm2d``, ``nn.SiLU``, ``F.interpolate`` -- with the
8-bit resize as Python loops over exact fractions.  It loads the state dict of tests/sapiens_helpers.py's configuration
T (``strict=True``), so the key mapping is pinned too, and runs in fp64 on one seeded 40 x 56 frame, once with the
normal weights and once with the depth weights.

Stored: the expected outputs only (normal [3,40,56], depth [40,56], fp64) and the seeds; the frame and the weights are
the helper's.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


class Attention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, D = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.heads, D // self.heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        scores = q @ k.transpose(-2, -1) / (D // self.heads) ** 0.5
        scores = scores - scores.amax(dim=-1, keepdim=True)
        p = scores.exp()
        p = p / p.sum(dim=-1, keepdim=True)
        return self.proj((p @ v).transpose(1, 2).reshape(B, N, D))


class FFN(nn.Module):
    def __init__(self, dim, inner):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(dim, inner), nn.GELU()), nn.Linear(inner, dim))

    def forward(self, x):
        return self.layers(x)


class Block(nn.Module):
    def __init__(self, dim, heads, inner):
        super().__init__()
        self.ln1, self.attn = nn.LayerNorm(dim, eps=1e-6), Attention(dim, heads)
        self.ln2, self.ffn = nn.LayerNorm(dim, eps=1e-6), FFN(dim, inner)

    def forward(self, x):
        x = x + self.attn(self.ln1(x))
        return x + self.ffn(self.ln2(x))


class PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.projection = nn.Conv2d(3, dim, kernel_size=16, stride=16, padding=2)


class Backbone(nn.Module):
    def __init__(self, dim, depth, inner, grid):
        super().__init__()
        self.patch_embed = PatchEmbed(dim)
        self.pos_embed = nn.Parameter(torch.zeros(1, grid[0] * grid[1], dim))
        self.layers = nn.ModuleList(Block(dim, dim // 64, inner) for _ in range(depth))
        self.ln1 = nn.LayerNorm(dim, eps=1e-6)

    def forward(self, x):
        x = self.patch_embed.projection(x)
        B, D, gh, gw = x.shape
        x = x.flatten(2).transpose(1, 2) + self.pos_embed
        for layer in self.layers:
            x = layer(x)
        return self.ln1(x).transpose(1, 2).reshape(B, D, gh, gw)


class Head(nn.Module):
    def __init__(self, dim, deconv, conv, out, affine):
        super().__init__()
        d, cin = [], dim
        for c in deconv:
            d += [nn.ConvTranspose2d(cin, c, kernel_size=4, stride=2, padding=1, bias=False),
                  nn.InstanceNorm2d(c, eps=1e-5, affine=affine), nn.SiLU()]
            cin = c
        self.deconv_layers = nn.Sequential(*d)
        d = []
        for c in conv:
            d += [nn.Conv2d(cin, c, kernel_size=1), nn.InstanceNorm2d(c, eps=1e-5, affine=affine), nn.SiLU()]
            cin = c
        self.conv_layers = nn.Sequential(*d)
        self.conv_seg = nn.Conv2d(cin, out, kernel_size=1)

    def forward(self, x):
        return self.conv_seg(self.conv_layers(self.deconv_layers(x)))


class Net(nn.Module):
    def __init__(self, hidden, layers, intermediate, grid, deconv, conv, affine, out):
        super().__init__()
        self.backbone = Backbone(hidden, layers, intermediate, grid)
        self.decode_head = Head(hidden, deconv, conv, out, affine)

    def forward(self, x):
        return self.decode_head(self.backbone(x))


def loop_resize(frame, h, w):
    """uint8 [H,W,3] (numpy) -> float64 [h,w,3]: the 8-bit bilinear resize as DESIGN.md states it, pixel by pixel."""
    H, W = frame.shape[:2]

    def taps(d, src, dst):
        centre = (Fraction(d) + Fraction(1, 2)) * Fraction(src, dst) - Fraction(1, 2)
        if centre < 0:
            return 0, 0, 0
        first = int(centre // 1)
        if first >= src - 1:
            return src - 1, src - 1, 0
        return first, first + 1, int(((centre - first) * 2048 + Fraction(1, 2)) // 1)

    out = np.zeros((h, w, 3))
    for y in range(h):
        ya, yb, wy = taps(y, H, h)
        for x in range(w):
            xa, xb, wx = taps(x, W, w)
            for c in range(3):
                top = (2048 - wx) * int(frame[ya, xa, c]) + wx * int(frame[ya, xb, c])
                bottom = (2048 - wx) * int(frame[yb, xa, c]) + wx * int(frame[yb, xb, c])
                out[y, x, c] = ((2048 - wy) * top + wy * bottom + (1 << 21)) >> 22
    return out


def main():
    from instag_amd import sapiens as S
    from tests import sapiens_helpers as G

    cfg = G.CONFIGS["T"]
    H, W = G.G21_FRAME
    frame = G.frames_of(1, H, W, G.G21_FRAME_SEED)
    in_h, in_w = 16 * cfg["grid"][0], 16 * cfg["grid"][1]
    small = loop_resize(frame[0].numpy(), in_h, in_w)
    x = torch.from_numpy((small - np.array([123.5, 116.5, 103.5])) / np.array([58.5, 57.0, 57.5])).permute(2, 0, 1)[None]
    stored = {}
    for kind, out in (("normal", 3), ("depth", 1)):
        w = G.weights("T", kind)
        net = Net(out=out, **cfg).double().eval()
        net.load_state_dict({k: v.double() for k, v in w.state_dict().items()}, strict=True)
        with torch.no_grad():
            y = F.interpolate(net(x), size=(H, W), mode="bilinear", align_corners=False)
            if kind == "normal":
                y = y / (torch.linalg.norm(y, dim=1, keepdim=True) + 1e-5)
        y = y[0] if kind == "normal" else y[0, 0]
        ours64 = S.sapiens_torch(w, frame, kind, dtype=torch.float64)[0]
        ours32 = S.sapiens_torch(w, frame, kind)[0].double()
        scale = float(y.abs().max())
        print(f"{kind}: max|y| {scale:.4f}  statement fp64 {float((ours64 - y).abs().max()) / scale:.3e}  "
              f"fp32 {float((ours32 - y).abs().max()) / scale:.3e}")
        stored[kind] = y.numpy()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g21_sapiens.npz"), normal=stored["normal"],
                        depth=stored["depth"], weights_seed=np.int64(G.G21_SEED), frame_seed=np.int64(G.G21_FRAME_SEED))


if __name__ == "__main__":
    main()
