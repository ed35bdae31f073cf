"""Shared by the wav2vec tests and tests/golden/make_golden_wav2vec.py: the two small configs, seeded audio, a slow
restatement of the streaming rule and the fp64 reference with the conditions the tests put on their own inputs."""
import functools

import torch

from instag_amd.wav2vec import Wav2Vec2Dims, Wav2Vec2Weights, frames_of, wav2vec2_torch

# both with the real convolution kernels and strides
S = Wav2Vec2Dims(conv_dim=64, hidden=128, heads=2, intermediate=256, layers=2, pos_kernel=128, pos_groups=2, vocab=44)
# N and K edge tiles everywhere, an odd head count
O = Wav2Vec2Dims(conv_dim=96, hidden=192, heads=3, intermediate=352, layers=1, pos_kernel=32, pos_groups=3, vocab=44)
CONFIGS = {"S": S, "O": O}
G16_SEED, G16_AUDIO_SEED = 16, 61


@functools.lru_cache(maxsize=None)
def weights(name: str, seed: int = 16) -> Wav2Vec2Weights:
    return Wav2Vec2Weights.random(CONFIGS[name], seed)


def seeded_audio(B: int, n: int, seed: int = 0) -> torch.Tensor:
    """[B,n] fp32 in about [-1, 1]: three sinusoids plus noise with a silent stretch in the middle, segment b louder than
    segment b - 1 by a factor of 3 and shifted off zero, so that the segments' means and variances differ."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    out = []
    for b in range(B):
        f = 80.0 + 900.0 * torch.rand(3, generator=g, dtype=torch.float64)
        ph = 6.283185307179586 * torch.rand(3, generator=g, dtype=torch.float64)
        x = sum(a * torch.sin(6.283185307179586 * fi * t + pi) for a, fi, pi in zip((0.5, 0.3, 0.2), f, ph))
        x = x + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
        if n >= 8:
            x[3 * n // 8: n // 2] = 0.0
        out.append((x * 0.3 * 3.0 ** b / 3.0 ** (B - 1) + 0.02 * (b + 1)))
    return torch.stack(out).float()


def slow_runs(audio: torch.Tensor):
    """The streaming rule with the list kept, as the issue words it -> [(the run's samples, left, right)]: chunks of 320
    (the last may be shorter); the list starts with ten zero chunks; every audio chunk is appended; whenever the list
    holds 70 chunks the network runs on their concatenation and only the last 20 are kept; at the end it runs once more on
    what the list holds.  A run of T rows keeps [10, min(T, T - 9)), the final one [10, T) (empty when T <= 10)."""
    held = [torch.zeros(320, dtype=audio.dtype) for _ in range(10)]
    runs = []

    def run(final):
        seg = torch.cat(held)
        T = (seg.numel() - 400) // 320 + 1
        right = T if final else min(T, T - 9)
        runs.append((seg, 10, max(right, 10)))

    for start in range(0, audio.numel(), 320):
        held.append(audio[start:start + 320])
        if len(held) == 70:
            run(False)
            del held[:50]
    run(True)
    return runs


class Case:
    """Segments with their fp64 reference (computed once per case and left unchanged)."""

    def __init__(self, w: Wav2Vec2Weights, audio: torch.Tensor):
        self.w, self.audio = w, audio
        taps = []
        self.want = wav2vec2_torch(w, audio.double(), taps)
        self.taps = taps
        self.got32 = wav2vec2_torch(w, audio.float()).double()
        self.T = frames_of(audio.shape[1])

    def e32(self, rows=slice(None)):
        """max|fp32 statement on the CPU - fp64| / max|fp64| over the segments ``rows``, and that scale."""
        scale = float(self.want[rows].abs().max())
        e = float((self.got32[rows] - self.want[rows]).abs().max()) / scale
        assert 1e-8 < e < 1e-4, e
        return e, scale

    def check_inputs(self):
        """The conditions under which a wrong softmax scale or a dead stage cannot hide, on the fp64 reference."""
        T, want = self.T, self.want
        if T > 2:       # a softmax row of T <= 2 entries cannot exceed 2 / T >= 1
            for name, p in self.taps:
                if name.endswith("attn_probs"):
                    assert float(p.amax(dim=-1).max()) > 2.0 / T, (name, float(p.amax(dim=-1).max()), T)
        assert float(want.std(dim=-1).min()) > 0.05 * float(want.abs().max())
        if self.audio.shape[0] > 1:
            var = self.audio.double().var(dim=1, unbiased=False)
            ratio = var[1:] / var[:-1]
            assert float(torch.minimum(ratio, 1.0 / ratio).max()) <= 0.5, var


@functools.lru_cache(maxsize=None)
def case(name: str, n: int, B: int = 2) -> Case:
    return Case(weights(name), seeded_audio(B, n, seed=n))
