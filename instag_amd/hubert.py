"""From a wav to the audio features of a 'hubert' head: the HuBERT encoder and the clip rule around it.

What data_utils/hubert.py of the reference does: the 16 kHz audio is normalised as a whole (zero mean, unit variance:
the processor of ``facebook/hubert-large-ls960-ft``), cut into clips of 1000 rows (320,080 samples) that do not overlap
in their rows, each clip goes through ``HubertModel`` alone, the last hidden states are joined to [E, 1024], and pairs
of rows are what it saves as aud_hu.npy.

    w = HubertWeights.load("hubert-large-ls960-ft/")                # the directory a user of the reference already has
    feats = hubert_features(load_wav16k("aud.wav"), w, "cuda")      # fp32 [E // 2, 2, 1024]
    store, meta = open_identity("data/May", "train", "cuda", audio_extractor="hubert", audio_features=feats)

The network is the wav2vec 2.0 "large" one of wav2vec.py (stable layer norm, layer-norm feature extractor) without the
CTC head: the output is the encoder's last LayerNorm.  On the GPU it runs in csrc/hubert.hip (fp32, inference only),
whose attention streams the keys, so that a clip's 1000 rows need no 1000 x 1000 scores anywhere; ``hubert_torch`` is
the plain-torch statement of the same arithmetic (any dtype, CPU or GPU) that the tests compare against and a CPU
device runs.  ``HubertEncoder`` is wav2vec.SegmentEncoder with this file's entry points, statement and clip length.
The project ships no weights and fetches none.
"""
from __future__ import annotations

import numpy as np
import torch

from .wav2vec import NORM_EPS, _REQUIRED, EncoderWeights, SegmentEncoder, encoder_torch, frames_of

KERNEL, STRIDE, CLIP_ROWS = 400, 320, 1000               # hubert.py: one row per 320 samples behind the first 400
CLIP_SAMPLES = STRIDE * (CLIP_ROWS - 1) + KERNEL           # 320,080


class HubertWeights(EncoderWeights):
    """The parameters of a ``HubertModel``: keys without the ``hubert.`` prefix, no ``lm_head.*`` (a fine-tuned
    checkpoint's is ignored, as ``masked_spec_embed`` is) and no part for ``vocab``.  The config rules are the wav2vec
    ones and, of HuBERT's own fields, a LayerNorm in the feature projection and no batch norm in the positional
    convolution (transformers' defaults)."""
    PREFIX, HEAD, WHAT = "hubert.", False, "hubert"
    REQUIRED = _REQUIRED + (("feat_proj_layer_norm", True, True), ("conv_pos_batch_norm", False, False))

    def state_dict(self, prefix: str = "", weight_norm: str = "parametrizations") -> dict:
        """The keys of a ``HubertModel`` (``prefix="hubert."``: of a ``HubertForCTC`` without its head)."""
        return super().state_dict(prefix, weight_norm)


def hubert_torch(weights: HubertWeights, input_values, taps=None):
    """``HubertModel(input_values).last_hidden_state`` in eval mode, input values [B,n] -> [B,T,hidden], in their dtype
    on their device; no attention mask and no normalisation: that is the whole utterance's (``normalise_utterance``).
    ``taps``: a list that receives (name, tensor) of every stage as ``wav2vec2_torch``'s does, "hidden" the last."""
    x = torch.as_tensor(input_values)
    if x.dim() != 2 or x.shape[1] < KERNEL:
        raise ValueError(f"hubert: input values [B, n >= {KERNEL}], got {tuple(x.shape)}")
    out = encoder_torch(weights, x, taps)
    if taps is not None:
        taps.append(("hidden", out))
    return out


def normalise_utterance(x) -> torch.Tensor:
    """(x - mean) / sqrt(var + 1e-7) with the population variance over the whole wav [L], what
    ``Wav2Vec2Processor(do_normalize=True)`` does before the reference cuts clips; summed in fp64 -> fp32."""
    x = torch.as_tensor(x)
    if x.dim() != 1 or x.numel() < 1:
        raise ValueError(f"normalise_utterance: samples [L >= 1], got {tuple(x.shape)}")
    x = x.double()
    return ((x - x.mean()) / torch.sqrt(x.var(unbiased=False) + NORM_EPS)).float()


class HubertEncoder(SegmentEncoder):
    """``hidden(input_values [B,n]) -> [B,T,hidden]`` through csrc/hubert.hip (wav2vec.SegmentEncoder); the default
    ``max_batch`` is sized for clips of 320,080 samples (4 at the real size: about 240 MB a clip, most of it the first
    two convolution buffers)."""
    ENTRY, STATEMENT, OUTPUT, DROPPED, SAMPLES = "hubert", staticmethod(hubert_torch), "hidden", "hidden", CLIP_SAMPLES
    INPUT = "input values"

    def hidden(self, input_values, taps=None):
        """``taps``: a list that receives (name, tensor) of every stage as ``hubert_torch``'s does, but for the
        attention probabilities and the output (debug: one chunk only, B <= max_batch)."""
        return self._encode(input_values, taps)


default_max_batch = HubertEncoder.default_max_batch


def attention(qkv: torch.Tensor, heads: int, out=None) -> torch.Tensor:
    """The operator's attention alone (csrc/hubert.hip): qkv [B,T,3 * 64 heads] (q | k | v), fp32 on the GPU ->
    ctx [B,T,64 heads] = softmax(q k^T / 8) v per (segment, head), written to ``out`` where one is given."""
    from . import _lib
    if qkv.dim() != 3 or qkv.shape[2] != 3 * 64 * int(heads) or qkv.dtype != torch.float32 or not qkv.is_cuda:
        raise ValueError(f"attention: fp32 qkv [B, T, {3 * 64 * int(heads)}] on the GPU, got {tuple(qkv.shape)} {qkv.dtype}")
    qkv = qkv.contiguous()
    B, T, _ = qkv.shape
    ctx = torch.empty(B, T, 64 * int(heads), dtype=torch.float32, device=qkv.device) if out is None else out
    if tuple(ctx.shape) != (B, T, 64 * int(heads)) or ctx.dtype != torch.float32 or ctx.device != qkv.device \
            or not ctx.is_contiguous():
        raise ValueError(f"attention: out is contiguous fp32 [{B}, {T}, {64 * int(heads)}] beside qkv, got {tuple(ctx.shape)}")
    with torch.cuda.device(qkv.device):
        _lib.check_arg(_lib.lib().instag_hubert_attention(_lib.ptr(qkv), _lib.ptr(ctx), B, T, int(heads),
                                                          _lib.current_stream()), "hubert_attention")
    return ctx


# ---- the clip rule and the features ---------------------------------------------------------------------------------
def clip_plan(n_samples: int, clip_rows: int = CLIP_ROWS):
    """The reference's loop over ``n_samples`` of audio as arithmetic -> ([(start, length)], expected_rows): with
    clip = 320 clip_rows and q = n_samples // clip, clip i < q is [clip i, min(L, clip i + clip + 80)) (``clip_rows`` rows,
    fewer where the audio ends inside the 80), then the remainder [clip q, L) if it holds the 400 samples of one row.
    expected_rows = (L - 80) // 320, and the clips' rows add up to exactly that for every L >= 400 (asserted): the
    reference's pad / truncate branch is never taken.  L < 400 raises ValueError (the reference crashes there)."""
    L, clip_rows = int(n_samples), int(clip_rows)
    if clip_rows < 2:                                        # (a clip of one row is shorter than the 400 samples of a row)
        raise ValueError(f"clip_plan: clip_rows >= 2, got {clip_rows}")
    if L < KERNEL:
        raise ValueError(f"clip_plan: at least {KERNEL} samples (one row), got {L}")
    clip = STRIDE * clip_rows
    q = L // clip
    plan = [(clip * i, min(L, clip * i + clip - STRIDE + KERNEL) - clip * i) for i in range(q)]
    if L - clip * q >= KERNEL:
        plan.append((clip * q, L - clip * q))
    expected = (L - (KERNEL - STRIDE)) // STRIDE
    assert sum(frames_of(n) for _, n in plan) == expected, (L, clip_rows, plan, expected)
    return plan, expected


def hubert_features(wav16k, weights: HubertWeights, device="cuda", encoder=None, clip_rows: int = CLIP_ROWS) -> np.ndarray:
    """The array the reference saves as aud_hu.npy for 16 kHz samples [L], fp32 [E // 2, 2, hidden] (an odd last row is
    dropped).  The wav is normalised as a whole; all clips of equal length go to the network as one batch, the others
    alone.  ``encoder`` is called as ``encoder(weights, input_values)`` in place of the HIP operator -- the tests'
    comparand."""
    x = torch.as_tensor(wav16k)
    if x.dim() != 1:
        raise ValueError(f"hubert_features: samples [L], got {tuple(x.shape)}")
    device = torch.device(device)
    plan, expected = clip_plan(x.numel(), clip_rows)
    x = normalise_utterance(x.detach().cpu()).to(device)
    clips = [x[s:s + n] for s, n in plan]
    if encoder is None:
        op = HubertEncoder(weights, device)
        encoder = lambda _, values: op.hidden(values)               # noqa: E731
    rows = [None] * len(clips)
    lengths = [c.numel() for c in clips]
    with torch.no_grad():
        for n in sorted(set(lengths)):
            same = [i for i, m in enumerate(lengths) if m == n]
            out = encoder(weights, torch.stack([clips[i] for i in same]))
            for j, i in enumerate(same):
                rows[i] = out[j].float()
    rows = torch.cat(rows, dim=0)
    assert rows.shape[0] == expected, (rows.shape, expected)
    rows = rows[:expected - expected % 2]
    return rows.reshape(-1, 2, rows.shape[1]).cpu().contiguous().numpy()
