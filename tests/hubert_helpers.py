"""Shared by the HuBERT tests and tests/golden/make_golden_hubert.py: the two small configs and the seeded audio of the
wav2vec tests, a slow restatement of the clip rule, the fp64 references of the network and of the
attention alone with the conditions the tests put on their own inputs, and the crafted attention rows."""
import functools

import torch

from instag_amd.hubert import HubertWeights, hubert_torch, normalise_utterance
from instag_amd.wav2vec import frames_of
from tests.wav2vec_helpers import CONFIGS, O, S, seeded_audio  # noqa: F401

G17_SEED, G17_AUDIO_SEED = 17, 71
E32_WINDOW = (1e-8, 1e-4)


@functools.lru_cache(maxsize=None)
def weights(name: str, seed: int = G17_SEED) -> HubertWeights:
    return HubertWeights.random(CONFIGS[name], seed)


def slow_clips(values: torch.Tensor, clip_rows: int = 1000):
    """The clip rule as the issue words it, walked with a cursor and with every row counted one by one ->
    ([(the clip's input values, rows it gives)], expected rows).  A row is a window of 400 samples and the windows start
    320 samples apart, so ``clip_rows`` rows need 400 + 320 (clip_rows - 1) samples and the clip behind them starts
    320 clip_rows samples further on.  As long as that many samples lie between the cursor and the end of the audio a
    clip is cut at the cursor -- short of its full length where the audio ends first -- and the cursor moves on; what
    lies behind the cursor at the end is one more clip if it holds a window.  The audio as a whole is expected to give
    (L - 80) // 320 rows."""
    L = int(values.shape[0])
    hop, full = 320 * clip_rows, 400 + 320 * (clip_rows - 1)
    pieces, cursor = [], 0
    while L - cursor >= hop:
        pieces.append(values[cursor:min(cursor + full, L)])
        cursor += hop
    if L - cursor >= 400:
        pieces.append(values[cursor:])

    def windows(piece):
        return sum(1 for first in range(0, piece.shape[0], 320) if first + 400 <= piece.shape[0])

    return [(piece, windows(piece)) for piece in pieces], (L - 80) // 320


class Case:
    """Input values with their fp64 reference (computed once per case and left unchanged)."""

    def __init__(self, w: HubertWeights, values: torch.Tensor):
        self.w, self.values = w, values
        taps = []
        self.want = hubert_torch(w, values.double(), taps)
        self.taps = taps
        self.got32 = hubert_torch(w, values.float()).double()
        self.T = frames_of(values.shape[1])

    def e32(self, rows=slice(None)):
        """max|fp32 statement on the CPU - fp64| / max|fp64| over the segments ``rows``, and that scale."""
        scale = float(self.want[rows].abs().max())
        e = float((self.got32[rows] - self.want[rows]).abs().max()) / scale
        assert E32_WINDOW[0] < e < E32_WINDOW[1], e
        return e, scale

    def check_inputs(self):
        """The conditions under which a wrong softmax scale or a dead stage cannot hide, on the fp64 reference."""
        T, want = self.T, self.want
        if T > 2:       # a softmax row of T <= 2 entries cannot exceed 2 / T >= 1
            for name, p in self.taps:
                if name.endswith("attn_probs"):
                    assert float(p.amax(dim=-1).max()) > 2.0 / T, (name, float(p.amax(dim=-1).max()), T)
        assert float(want.std(dim=-1).min()) > 0.05 * float(want.abs().max())
        for b in range(self.values.shape[0]):
            self.e32(slice(b, b + 1))


def values_of(B: int, n: int, seed: int) -> torch.Tensor:
    """[B,n] fp32 input values: each seeded segment normalised as an utterance of its own."""
    return torch.stack([normalise_utterance(r) for r in seeded_audio(B, n, seed=seed)])


@functools.lru_cache(maxsize=None)
def case(name: str, n: int, B: int = 2) -> Case:
    return Case(weights(name), values_of(B, n, seed=n))


# ---- the attention alone ---------------------------------------------------------------------------------------------
# crafted query rows (name -> row index); the keys carry the patterns on their first four dimensions
CRAFTED = {"rising": 3, "first": 70, "equal": 101, "huge": 131, "spike": 190}


class AttentionCase:
    """qkv [B,T,3 * 64 heads] fp32 with softmax(q k^T / 8) v in fp64 and in fp32 on the CPU.  q and k are N(0, 2) so that
    the scores have a standard deviation near 2; v is N(0.5, 1) so that a row of equal scores (the mean of v) is not
    near zero.  ``crafted``: the rows of CRAFTED of segment 0, head 0 get (with c the key and s its score)
      rising: s = 30 c / T, the maximum at the LAST key, every tile's maximum above the one before it;
      first:  s = 10 at key 0 and 0 elsewhere;
      equal:  s = 0 everywhere;
      huge:   s = +-100, an exponent without the running maximum overflows;
      spike:  s = 10 at the first key of the last, partial tile of 64, 64 (T // 64), and 0 elsewhere."""

    def __init__(self, T: int, heads: int, B: int, seed: int, crafted: bool = False):
        g = torch.Generator().manual_seed(seed)
        H = 64 * heads
        q, k = (2.0 ** 0.5 * torch.randn(B, T, heads, 64, generator=g) for _ in range(2))
        v = 0.5 + torch.randn(B, T, heads, 64, generator=g)
        self.rows = {}
        if crafted:
            assert T > max(CRAFTED.values()) and T % 64
            c = torch.arange(T, dtype=torch.float32)
            self.spike_key = 64 * (T // 64)
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
        self.T, self.heads, self.B = T, heads, B
        self.qkv = torch.cat([t.reshape(B, T, H) for t in (q, k, v)], dim=2).contiguous()
        self.scores = self._scores(torch.float64)
        self.want = self._ctx(torch.float64)
        self.got32 = self._ctx(torch.float32).double()

    def _scores(self, dtype):
        q, k, _ = (t.to(dtype).view(self.B, self.T, self.heads, 64).transpose(1, 2) for t in self.qkv.chunk(3, dim=2))
        return (q * 0.125) @ k.transpose(2, 3)

    def _ctx(self, dtype):
        v = self.qkv.chunk(3, dim=2)[2].to(dtype).view(self.B, self.T, self.heads, 64).transpose(1, 2)
        probs = torch.softmax(self._scores(dtype), dim=-1)
        return (probs @ v).transpose(1, 2).reshape(self.B, self.T, 64 * self.heads)

    def e32(self):
        """max|fp32 on the CPU - fp64| / max|fp64| and that scale.  One key: the softmax is 1 and the output is v in
        any precision, so e32 is 0 and the operator has to be exact."""
        scale = float(self.want.abs().max())
        e = float((self.got32 - self.want).abs().max()) / scale
        if self.T == 1:
            assert e == 0.0
        else:
            assert E32_WINDOW[0] < e < E32_WINDOW[1], e
        return e, scale

    def check_inputs(self):
        T, probs = self.T, torch.softmax(self.scores, dim=-1)
        if T > 2:
            assert float(probs.amax(dim=-1).max()) > 2.0 / T
        assert float(self.want.abs().amax(dim=-1).min()) > 0.05 * float(self.want.abs().max())     # no dead row
        self.e32()
        if self.rows:
            s = self.scores[0, 0]
            r = self.rows
            assert int(s[r["rising"]].argmax()) == T - 1 and bool((s[r["rising"]].diff() > 0).all())
            tile_max = [float(s[r["rising"], a:a + 64].max()) for a in range(0, T, 64)]
            assert all(b > a + 1.0 for a, b in zip(tile_max, tile_max[1:])), tile_max
            assert int(s[r["first"]].argmax()) == 0 and float(probs[0, 0, r["first"], 0]) > 0.9
            assert float(s[r["equal"]].abs().max()) == 0.0
            assert 99.0 < float(s[r["huge"]].max()) < 101.0 and -101.0 < float(s[r["huge"]].min()) < -99.0
            assert int(s[r["spike"]].argmax()) == self.spike_key and self.spike_key + 64 > T > self.spike_key
            assert float(probs[0, 0, r["spike"], self.spike_key]) > 0.9


@functools.lru_cache(maxsize=None)
def features_wav():
    """The wav of the features test on the GPU with the Case of each of its clips -> (wav [330000], [Case])."""
    from instag_amd.hubert import clip_plan
    wav = seeded_audio(1, 330000, seed=7)[0]
    plan, expected = clip_plan(330000)
    assert plan == [(0, 320080), (320000, 10000)] and expected == 1031
    values = normalise_utterance(wav)
    return wav, [Case(weights("S"), values[None, start:start + length]) for start, length in plan]


ATTENTION_SHAPES = [(T, heads, B) for T in (1, 2, 63, 64, 65, 128, 129, 200, 1000) for heads in (1, 3) for B in (1, 2)]


@functools.lru_cache(maxsize=None)
def attention_case(T: int, heads: int, B: int, crafted: bool = False) -> AttentionCase:
    return AttentionCase(T, heads, B, seed=1000 * T + 10 * heads + B, crafted=crafted)
