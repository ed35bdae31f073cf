"""Shared by the Sapiens tests and tests/golden/make_golden_sapiens.py: the two tiny configurations with their seeded
weights under the package's keys, seeded frames, the fp64 reference of every stage with the fp32 CPU statement's own
error beside it, a slow loop statement of the patch rows, and the cases of the stage tests."""
import functools
from fractions import Fraction

import torch

from instag_amd import sapiens as S
from tests.hubert_helpers import AttentionCase

E32_WINDOW = (1e-8, 1e-4)
G21_SEED, G21_FRAME_SEED, G21_FRAME = 21, 12, (40, 56)

# T: input 64 x 48 (grid 4 x 3), output map 64 x 48, norms without gain and shift.
# U: input 80 x 48 (grid 5 x 3), output map 10 x 6, norms with gain and shift.
CONFIGS = {
    "T": dict(hidden=128, layers=2, intermediate=256, grid=(4, 3), deconv=(64, 32, 32, 32), conv=(32,), affine=False),
    "U": dict(hidden=64, layers=1, intermediate=128, grid=(5, 3), deconv=(32,), conv=(32, 32), affine=True),
}
# The gains: 1 in the head.  Behind every InstanceNorm a stage is of order 1 whatever its weights' size, so the head's
# gain only has to keep conv_seg's output of order 1 beside its bias of 0.1; test_sapiens_host.py checks every stage's e32.
HEAD_GAIN = 1.0


@functools.lru_cache(maxsize=None)
def weights(name: str, kind: str = "normal", seed: int = G21_SEED) -> S.SapiensWeights:
    return S.SapiensWeights.random(kind=kind, seed=seed, head_gain=HEAD_GAIN, **CONFIGS[name])


def frames_of(B: int, H: int, W: int, seed: int) -> torch.Tensor:
    """uint8 [B,H,W,3]: a smooth seeded image (a few waves per channel) plus noise of +-20, clipped."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, H).view(1, H, 1, 1)
    x = torch.linspace(0, 1, W).view(1, 1, W, 1)
    f, p = 1 + 4 * torch.rand(2, B, 1, 1, 3, generator=g), 6.28 * torch.rand(2, B, 1, 1, 3, generator=g)
    img = 128 + 70 * torch.sin(6.28 * f[0] * y + p[0]) * torch.cos(6.28 * f[1] * x + p[1])
    img = img + 40 * (torch.rand(B, H, W, 3, generator=g) - 0.5)
    return img.round().clamp(0, 255).to(torch.uint8)


def relative(a: torch.Tensor, want: torch.Tensor):
    """(max|a - want| / max|want|, max|want|), in fp64."""
    scale = float(want.abs().max())
    return float((a.double().cpu() - want).abs().max()) / scale, scale


class Case:
    """Frames with the fp64 reference of every stage (computed once and left unchanged) and the fp32 CPU statement's."""

    def __init__(self, w: S.SapiensWeights, frames: torch.Tensor):
        self.w, self.frames = w, frames
        taps64, taps32 = [], []
        self.want = S.sapiens_torch(w, frames, dtype=torch.float64, taps=taps64)
        self.got32 = S.sapiens_torch(w, frames, dtype=torch.float32, taps=taps32).double()
        self.taps, self.taps32 = dict(taps64), {k: v.double() for k, v in taps32}

    def e32(self, stage="out", rows=slice(None)):
        """max|fp32 statement on the CPU - fp64| / max|fp64| of ``stage`` over the frames ``rows``, and that scale."""
        e, scale = relative(self.taps32[stage][rows], self.taps[stage][rows])
        assert E32_WINDOW[0] < e < E32_WINDOW[1], (stage, e)
        return e, scale


@functools.lru_cache(maxsize=None)
def case(name: str, kind: str, B: int, H: int, W: int) -> Case:
    return Case(weights(name, kind), frames_of(B, H, W, seed=1000 * H + W))


# ---- the front end, slowly ----------------------------------------------------------------------------------------------
def slow_resize(frame, size):
    """One uint8 frame [H,W,3] -> nested lists [h][w][3] of ints: the rule of ``resize_u8_torch`` walked pixel by pixel
    on exact fractions."""
    H, W = frame.shape[:2]
    h, w = size
    px = frame.tolist()

    def taps(d, S_, D):
        c = Fraction(2 * d + 1, 2) * Fraction(S_, D) - Fraction(1, 2)
        if c < 0:
            return 0, 0, 0
        i = c.numerator // c.denominator
        if i >= S_ - 1:
            return S_ - 1, S_ - 1, 0
        wt = (c - i) * 2048 + Fraction(1, 2)
        return i, i + 1, wt.numerator // wt.denominator

    out = []
    for y in range(h):
        y0, y1, wy = taps(y, H, h)
        row = []
        for x in range(w):
            x0, x1, wx = taps(x, W, w)
            row.append([((2048 - wy) * ((2048 - wx) * px[y0][x0][c] + wx * px[y0][x1][c])
                         + wy * ((2048 - wx) * px[y1][x0][c] + wx * px[y1][x1][c]) + 2 ** 21) // 2 ** 22 for c in range(3)])
        out.append(row)
    return out


def slow_patch_rows(frames, size, dtype=torch.float32):
    """[B,H,W,3] uint8 -> [B,T,768] of ``dtype``: token (gy, gx)'s entry (c, ky, kx) is the normalised resized pixel
    (16 gy + ky - 2, 16 gx + kx - 2), 0 outside the image -- filled entry by entry."""
    h, w = size
    gh, gw = (h - 12) // 16 + 1, (w - 12) // 16 + 1
    mean, std = torch.tensor(S.MEAN, dtype=dtype), torch.tensor(S.STD, dtype=dtype)
    out = torch.zeros(frames.shape[0], gh * gw, 768, dtype=dtype)
    for b in range(frames.shape[0]):
        small = torch.tensor(slow_resize(frames[b], size), dtype=dtype)             # [h,w,3]
        norm = (small - mean) / std
        for gy in range(gh):
            for gx in range(gw):
                for ky in range(16):
                    y = 16 * gy + ky - 2
                    if not 0 <= y < h:
                        continue
                    for kx in range(16):
                        x = 16 * gx + kx - 2
                        if 0 <= x < w:
                            out[b, gy * gw + gx, ky * 16 + kx::256] = norm[y, x]
    return out


PATCH_ROWS_CASES = [((32, 32), (64, 48)), ((100, 70), (64, 48)), ((50, 38), (80, 48))]


# ---- the attention alone: the HuBERT tests' cases at this network's lengths ---------------------------------------------
ATTENTION_SHAPES = [(1, 1, 1), (63, 2, 1), (65, 1, 2), (1025, 2, 1), (3072, 1, 1)]


@functools.lru_cache(maxsize=None)
def attention_case(T: int, heads: int, B: int) -> AttentionCase:
    return AttentionCase(T, heads, B, seed=3000 * T + 10 * heads + B)


class CraftedAttention(AttentionCase):
    """The crafted rows of tests/hubert_helpers.py (CRAFTED: rising, first, equal, huge, spike) at a length that is a
    whole number of key tiles, which that class does not take: the spike sits on the first key of the last tile,
    ``T - 64``.  One segment, one head; the rest of the case (q, k ~ N(0, 2), v ~ N(0.5, 1), the fp64 and fp32 CPU
    results, ``e32``) is the base class's."""

    def __init__(self, T: int, seed: int):
        from tests.hubert_helpers import CRAFTED
        assert T % 64 == 0 and T > 192
        g = torch.Generator().manual_seed(seed)
        q, k = (2.0 ** 0.5 * torch.randn(1, T, 1, 64, generator=g) for _ in range(2))
        v = 0.5 + torch.randn(1, T, 1, 64, generator=g)
        c = torch.arange(T, dtype=torch.float32)
        self.spike_key = T - 64
        k[0, :, 0, 0] = c / T
        k[0, :, 0, 1] = (c == 0).float()
        k[0, :, 0, 2] = torch.where(torch.rand(T, generator=g) < 0.5, -1.0, 1.0)
        k[0, :, 0, 3] = (c == self.spike_key).float()
        for name, axis, gain in (("rising", 0, 240.0), ("first", 1, 80.0), ("equal", None, 0.0), ("huge", 2, 800.0),
                                 ("spike", 3, 80.0)):
            q[0, CRAFTED[name], 0] = 0.0
            if axis is not None:
                q[0, CRAFTED[name], 0, axis] = gain
        self.rows = dict(CRAFTED)
        self.T, self.heads, self.B = T, 1, 1
        self.qkv = torch.cat([t.reshape(1, T, 64) for t in (q, k, v)], dim=2).contiguous()
        self.scores = self._scores(torch.float64)
        self.want = self._ctx(torch.float64)
        self.got32 = self._ctx(torch.float32).double()


@functools.lru_cache(maxsize=None)
def crafted_attention(T: int = 3072) -> CraftedAttention:
    return CraftedAttention(T, seed=7 * T)


# ---- the transposed convolution alone -------------------------------------------------------------------------------------
IMPULSES = [(0, 0), (0, 4), (2, 0), (2, 4), (0, 2), (1, 2)]        # the four corners, an edge and the centre of 3 x 5
DECONV_SHAPES = [(4, 3, 32, 32), (33, 17, 96, 64)]                 # h, w, cin, cout


class DeconvCase:
    """x [B,cin,h,w] and a weight [cin,cout,4,4] in fp32 with conv_transpose2d(stride 2, padding 1) in fp64 and in fp32."""

    def __init__(self, x, weight):
        self.x, self.weight = x, weight
        self.want = torch.nn.functional.conv_transpose2d(x.double(), weight.double(), stride=2, padding=1)
        self.got32 = torch.nn.functional.conv_transpose2d(x, weight, stride=2, padding=1).double()

    def e32(self):
        e, scale = relative(self.got32, self.want)
        assert E32_WINDOW[0] < e < E32_WINDOW[1], e
        return e, scale


@functools.lru_cache(maxsize=None)
def deconv_case(h: int, w: int, cin: int, cout: int, B: int = 2) -> DeconvCase:
    g = torch.Generator().manual_seed(100 * h + w)
    return DeconvCase(torch.randn(B, cin, h, w, generator=g), torch.randn(cin, cout, 4, 4, generator=g) / (4 * cin) ** 0.5)


@functools.lru_cache(maxsize=None)
def impulse_case() -> DeconvCase:
    """One frame per position of IMPULSES: channel 0 is 1 there, everything else 0; weights with sixteen distinct taps."""
    g = torch.Generator().manual_seed(5)
    x = torch.zeros(len(IMPULSES), 32, 3, 5)
    for b, (y, xx) in enumerate(IMPULSES):
        x[b, 0, y, xx] = 1.0
    weight = torch.randn(32, 32, 4, 4, generator=g)
    weight[0] = (1.0 + torch.arange(16.0).view(1, 4, 4)) * (1.0 + 0.01 * torch.arange(32.0).view(32, 1, 1))
    return DeconvCase(x, weight)


# ---- InstanceNorm + SiLU alone --------------------------------------------------------------------------------------------
NORM_MAPS = [(3, 4), (6, 8), (64, 48)]                             # 12, 48 and 3072 elements
CONSTANT_CHANNEL, OFFSET_CHANNEL, NORM_CHANNELS = 5, 9, 32


class NormCase:
    """x [B,C,h,w] in fp32: channel 5 constant (7.25), channel 9 with a mean of 100 beside a spread of 1; gamma / beta or
    None; instance_norm (eps 1e-5) + SiLU in fp64 and in fp32 on the CPU."""

    def __init__(self, h, w, affine, B=3):
        g = torch.Generator().manual_seed(10 * h + w + affine)
        x = 0.3 + 1.5 * torch.randn(B, NORM_CHANNELS, h, w, generator=g)
        x[:, CONSTANT_CHANNEL] = 7.25
        x[:, OFFSET_CHANNEL] = 100.0 + torch.randn(B, h, w, generator=g)
        self.x = x
        self.gamma = 1.0 + 0.2 * torch.randn(NORM_CHANNELS, generator=g) if affine else None
        self.beta = 0.1 * torch.randn(NORM_CHANNELS, generator=g) if affine else None
        self.want = self._run(torch.float64)
        self.got32 = self._run(torch.float32).double()

    def _run(self, dtype):
        cast = lambda t: None if t is None else t.to(dtype)          # noqa: E731
        return torch.nn.functional.silu(torch.nn.functional.instance_norm(self.x.to(dtype), weight=cast(self.gamma),
                                                                           bias=cast(self.beta), eps=S.IN_EPS))

    def e32(self, channels=slice(None)):
        e, scale = relative(self.got32[:, channels], self.want[:, channels])
        assert E32_WINDOW[0] < e < E32_WINDOW[1], e
        return e, scale


@functools.lru_cache(maxsize=None)
def norm_case(h: int, w: int, affine: bool) -> NormCase:
    return NormCase(h, w, affine)
