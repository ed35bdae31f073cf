"""From a wav to the audio features of an 'esperanto' head: the wav2vec 2.0 CTC network and the streaming rule around it.

What data_utils/wav2vec.py of the reference does in file mode (``-l 10 -m 50 -r 10``, 50 frames a second): the 16 kHz
audio goes through ``cpierse/wav2vec2-large-xlsr-53-esperanto`` in overlapping runs of 1.4 s, the logits rows kept
from every run are joined to [M, 44], and sixteen rows around every second one are what it saves as aud_eo.npy.

    w = Wav2Vec2Weights.load("wav2vec2-large-xlsr-53-esperanto/")   # the directory a user of the reference already has
    feats = esperanto_features(load_wav16k("aud.wav"), w, "cuda")   # fp32 [M // 2 + 1, 16, 44]
    store, meta = open_identity("data/May", "train", "cuda", audio_extractor="esperanto", audio_features=feats)

On the GPU the network runs in csrc/wav2vec.hip (fp32, inference only); ``wav2vec2_torch`` is the plain-torch statement of
the same arithmetic (any dtype, CPU or GPU) that the tests compare against and a CPU device runs.  The operator's host
side is ``SegmentEncoder``, which hubert.py's operator shares: a device_op.DeviceOperator that states its entry points,
its statement and its output.  The project ships no weights and fetches none.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import asdict, dataclass

import numpy as np
import torch
import torch.nn.functional as F

from .device_op import DeviceOperator

CONV_KERNEL, CONV_STRIDE = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
HEAD_DIM = 64
LN_EPS, NORM_EPS = 1e-5, 1e-7
CHUNK, PREFIX_CHUNKS, RUN_CHUNKS, KEPT_CHUNKS, CONTEXT_ROWS = 320, 10, 70, 20, 10      # wav2vec.py -l 10 -m 50 -r 10
RUN_SAMPLES = RUN_CHUNKS * CHUNK
WINDOW, WINDOW_PAD, WINDOW_STRIDE = 16, 8, 2
WORKSPACE_LIMIT = 1 << 30


@dataclass(frozen=True)
class Wav2Vec2Dims:
    """The dimensions of the network.  The default is the 'large' model of the esperanto checkpoint."""
    conv_dim: int = 512
    hidden: int = 1024
    heads: int = 16
    intermediate: int = 4096
    layers: int = 24
    pos_kernel: int = 128
    pos_groups: int = 16
    vocab: int = 44

    def check(self, head: bool = True) -> "Wav2Vec2Dims":
        """The shapes csrc/wav2vec.hip takes (include/instag_wav2vec.h); ValueError naming the field otherwise.
        ``head=False``: the network without its CTC head (csrc/hubert.hip), where ``vocab`` plays no part."""
        from . import _lib
        rules = (
            ("heads", self.heads >= 1 and self.hidden == self.heads * HEAD_DIM, f"hidden / heads must be {HEAD_DIM}"),
            ("conv_dim", 32 <= self.conv_dim <= 1024 and self.conv_dim % 32 == 0, "a multiple of 32 in [32, 1024]"),
            ("hidden", 32 <= self.hidden <= 1024 and self.hidden % 32 == 0, "a multiple of 32 in [32, 1024]"),
            ("intermediate", 32 <= self.intermediate <= 65536 and self.intermediate % 32 == 0, "a multiple of 32"),
            ("layers", 1 <= self.layers <= _lib.WAV2VEC["INSTAG_WAV2VEC_MAX_LAYERS"],
             f"in [1, {_lib.WAV2VEC['INSTAG_WAV2VEC_MAX_LAYERS']}]"),
            ("pos_kernel", 2 <= self.pos_kernel <= 1024 and self.pos_kernel % 2 == 0, "even, in [2, 1024]"),
            ("pos_groups", self.pos_groups >= 1 and self.hidden % self.pos_groups == 0
             and (self.hidden // self.pos_groups) % 32 == 0, "hidden / pos_groups must be a multiple of 32"),
            ("vocab", 4 <= self.vocab <= 65536 and self.vocab % 4 == 0, "a multiple of 4"),
        )
        for field, ok, rule in rules:
            if not ok and (head or field != "vocab"):
                raise ValueError(f"wav2vec 2.0 config: {field} = {getattr(self, field)} is not supported: {rule}")
        return self

    def hf(self) -> dict:
        """The fields of a ``transformers`` config.json that describe this network."""
        return dict(vocab_size=self.vocab, hidden_size=self.hidden, num_hidden_layers=self.layers,
                    num_attention_heads=self.heads, intermediate_size=self.intermediate, conv_dim=[self.conv_dim] * 7,
                    conv_kernel=list(CONV_KERNEL), conv_stride=list(CONV_STRIDE), conv_bias=True, feat_extract_norm="layer",
                    feat_extract_activation="gelu", hidden_act="gelu", do_stable_layer_norm=True,
                    num_conv_pos_embeddings=self.pos_kernel, num_conv_pos_embedding_groups=self.pos_groups,
                    layer_norm_eps=LN_EPS)


# config.json field -> (the value the kernels are written for, transformers' default when the file leaves it out)
_REQUIRED = (("do_stable_layer_norm", True, False), ("feat_extract_norm", "layer", "group"), ("conv_bias", True, False),
             ("hidden_act", "gelu", "gelu"), ("feat_extract_activation", "gelu", "gelu"),
             ("conv_kernel", list(CONV_KERNEL), list(CONV_KERNEL)), ("conv_stride", list(CONV_STRIDE), list(CONV_STRIDE)),
             ("layer_norm_eps", LN_EPS, LN_EPS))


def dims_of(config, required=_REQUIRED, head: bool = True) -> Wav2Vec2Dims:
    """``config``: a Wav2Vec2Dims, or the dict of a config.json (the group-norm 'base' variant and anything else the
    kernels are not written for raise ValueError naming the field).  ``required``: the (field, value, default) rules;
    ``head=False``: no CTC head, ``vocab_size`` may be missing."""
    if isinstance(config, Wav2Vec2Dims):
        return config.check(head)
    cfg = dict(config)
    for field, want, default in required:
        got = cfg.get(field, default)
        got = list(got) if isinstance(got, (list, tuple)) else got
        if got != want:
            raise ValueError(f"wav2vec 2.0 config: {field} = {got!r} is not supported (only {want!r})")
    try:
        conv_dim = list(cfg.get("conv_dim", [512] * 7))
        if len(conv_dim) != 7 or len(set(conv_dim)) != 1:
            raise ValueError(f"wav2vec 2.0 config: conv_dim = {conv_dim!r} is not supported (seven equal widths)")
        return Wav2Vec2Dims(conv_dim=int(conv_dim[0]), hidden=int(cfg["hidden_size"]), heads=int(cfg["num_attention_heads"]),
                            intermediate=int(cfg["intermediate_size"]), layers=int(cfg["num_hidden_layers"]),
                            pos_kernel=int(cfg.get("num_conv_pos_embeddings", 128)),
                            pos_groups=int(cfg.get("num_conv_pos_embedding_groups", 16)),
                            vocab=int(cfg["vocab_size"] if head else cfg.get("vocab_size", 32))).check(head)
    except KeyError as e:
        raise ValueError(f"wav2vec 2.0 config: misses the field {e.args[0]!r}") from None


def frames_of(n: int) -> int:
    """Logits rows of a run of ``n`` samples: (n - 400) // 320 + 1, through the seven convolutions."""
    for k, s in zip(CONV_KERNEL, CONV_STRIDE):
        n = (n - k) // s + 1
    return n


def macs(dims: Wav2Vec2Dims, n: int = RUN_SAMPLES, head: bool = True) -> int:
    """Multiply-accumulates of one run of ``n`` samples (the products only: MACS of the bench); ``head=False``: without
    the CTC head's product."""
    d, t, total = dims, n, 0
    for l, (k, s) in enumerate(zip(CONV_KERNEL, CONV_STRIDE)):
        t = (t - k) // s + 1
        total += t * d.conv_dim * k * (1 if l == 0 else d.conv_dim)
    total += t * d.conv_dim * d.hidden + t * d.hidden * (d.hidden // d.pos_groups) * d.pos_kernel
    per_layer = 4 * d.hidden * d.hidden + 2 * d.hidden * d.intermediate + 2 * t * d.hidden
    return total + d.layers * t * per_layer + (t * d.hidden * d.vocab if head else 0)


# ---- weights ----------------------------------------------------------------------------------------------------------
_POS = "encoder.pos_conv_embed.conv."
_POS_SPELLINGS = ((_POS + "weight_g", _POS + "weight_v"),
                  (_POS + "parametrizations.weight.original0", _POS + "parametrizations.weight.original1"))
_IGNORED = ("masked_spec_embed",)


def _shapes(d: Wav2Vec2Dims, head: bool = True) -> dict:
    """Canonical key (no ``wav2vec2.`` prefix, the old weight-norm spelling) -> shape; ``head``: with ``lm_head.*``."""
    s = {}
    for i, k in enumerate(CONV_KERNEL):
        p = f"feature_extractor.conv_layers.{i}."
        s[p + "conv.weight"] = (d.conv_dim, 1 if i == 0 else d.conv_dim, k)
        s[p + "conv.bias"] = s[p + "layer_norm.weight"] = s[p + "layer_norm.bias"] = (d.conv_dim,)
    s["feature_projection.layer_norm.weight"] = s["feature_projection.layer_norm.bias"] = (d.conv_dim,)
    s["feature_projection.projection.weight"] = (d.hidden, d.conv_dim)
    s["feature_projection.projection.bias"] = (d.hidden,)
    s[_POS + "bias"] = (d.hidden,)
    s[_POS + "weight_g"] = (1, 1, d.pos_kernel)
    s[_POS + "weight_v"] = (d.hidden, d.hidden // d.pos_groups, d.pos_kernel)
    s["encoder.layer_norm.weight"] = s["encoder.layer_norm.bias"] = (d.hidden,)
    for l in range(d.layers):
        p = f"encoder.layers.{l}."
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[p + f"attention.{name}.weight"] = (d.hidden, d.hidden)
            s[p + f"attention.{name}.bias"] = (d.hidden,)
        s[p + "layer_norm.weight"] = s[p + "layer_norm.bias"] = (d.hidden,)
        s[p + "feed_forward.intermediate_dense.weight"] = (d.intermediate, d.hidden)
        s[p + "feed_forward.intermediate_dense.bias"] = (d.intermediate,)
        s[p + "feed_forward.output_dense.weight"] = (d.hidden, d.intermediate)
        s[p + "feed_forward.output_dense.bias"] = (d.hidden,)
        s[p + "final_layer_norm.weight"] = s[p + "final_layer_norm.bias"] = (d.hidden,)
    if head:
        s["lm_head.weight"] = (d.vocab, d.hidden)
        s["lm_head.bias"] = (d.vocab,)
    return s


class EncoderWeights:
    """What Wav2Vec2Weights and hubert.HubertWeights share: the frozen parameters in fp32 on the CPU, under the
    checkpoint's keys without the model's prefix; the positional convolution's weight norm stays as its two factors
    (``weight_g`` [1,1,k], ``weight_v``).  A subclass names its prefix, whether it has the CTC head, its config rules
    and itself (for the messages)."""
    PREFIX, HEAD, REQUIRED, WHAT = "wav2vec2.", True, _REQUIRED, "wav2vec 2.0"

    def __init__(self, dims: Wav2Vec2Dims, tensors: dict):
        self.dims, self.tensors = dims, tensors

    @classmethod
    def dims_of(cls, config) -> Wav2Vec2Dims:
        try:
            return dims_of(config, cls.REQUIRED, cls.HEAD)
        except ValueError as e:
            raise ValueError(str(e).replace("wav2vec 2.0", cls.WHAT, 1)) from None

    @classmethod
    def load(cls, path):
        """``path``: the model directory (config.json beside pytorch_model.bin, or model.safetensors where the
        safetensors package imports)."""
        path = str(path)
        with open(os.path.join(path, "config.json")) as f:
            config = json.load(f)
        binary = os.path.join(path, "pytorch_model.bin")
        if os.path.exists(binary):
            sd = torch.load(binary, map_location="cpu", weights_only=True)
        else:
            st = os.path.join(path, "model.safetensors")
            if not os.path.exists(st):
                raise FileNotFoundError(f"{path}: neither pytorch_model.bin nor model.safetensors")
            try:
                from safetensors.torch import load_file
            except ImportError:
                raise FileNotFoundError(f"{path}: no pytorch_model.bin, and model.safetensors needs the safetensors "
                                        "package") from None
            sd = load_file(st)
        return cls.from_state_dict(sd, config)

    @classmethod
    def from_state_dict(cls, sd, config):
        """``sd``: the keys of the ``transformers`` module with or without the model's prefix, the positional
        convolution's weight norm as ``weight_g`` / ``weight_v`` (old checkpoints) or
        ``parametrizations.weight.original0`` / ``original1``; ``masked_spec_embed`` and keys the network does not have
        are ignored.  A missing key, a wrong shape and an unsupported config field raise ValueError naming it."""
        dims = cls.dims_of(config)
        flat = {(k[len(cls.PREFIX):] if k.startswith(cls.PREFIX) else k): v for k, v in sd.items()}
        for old, new in zip(*_POS_SPELLINGS):
            if old not in flat and new in flat:
                flat[old] = flat[new]
        tensors = {}
        for key, shape in _shapes(dims, cls.HEAD).items():
            if key not in flat:
                raise ValueError(f"{cls.WHAT} weights: the state dict misses {key!r}")
            t = torch.as_tensor(flat[key]).detach().to(device="cpu", dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{cls.WHAT} weights: {key!r} has shape {tuple(t.shape)}, the config says {shape}")
            tensors[key] = t.clone()
        return cls(dims, tensors)

    @classmethod
    def random(cls, config=Wav2Vec2Dims(), seed: int = 0):
        """Seeded stand-ins in the checkpoint's keys (tests, benches).  Matrices are drawn with a gain over
        1 / sqrt(fan-in): 1.4 in front of a GELU so that the LayerNorm behind it sees both of its sides, 1.5 for q and
        k so that the scores have a standard deviation near 2 and the attention is far from uniform, 1 elsewhere;
        LayerNorm gains are 1 +- 0.2, every bias and shift is 0.1 wide, and the head's gain is 1 so that the classes
        of a row differ by about the row's size."""
        dims = cls.dims_of(config)
        g = torch.Generator().manual_seed(seed)
        tensors = {}
        for key, shape in _shapes(dims, cls.HEAD).items():
            if key.endswith("weight_g"):
                continue                        # follows weight_v, below
            if len(shape) == 1:
                v = 0.1 * torch.randn(shape, generator=g)
                if key.endswith("layer_norm.weight"):
                    v = 1.0 + 2.0 * v
            else:
                fan_in = int(np.prod(shape[1:]))
                gain = 1.5 if (".q_proj." in key or ".k_proj." in key) else \
                    1.4 if ("conv" in key or "intermediate_dense" in key) else 1.0
                v = torch.randn(shape, generator=g) * (gain / fan_in ** 0.5)
            tensors[key] = v
        # g = (1 +- 0.1) ||v||: a folded weight close to v, yet another one
        v = tensors[_POS + "weight_v"]
        norm = v.double().pow(2).sum(dim=(0, 1), keepdim=True).sqrt().float()
        tensors[_POS + "weight_g"] = norm * (1.0 + 0.1 * torch.randn(norm.shape, generator=g))
        return cls(dims, {k: t.float().contiguous() for k, t in tensors.items()})

    def state_dict(self, prefix=None, weight_norm: str = "parametrizations") -> dict:
        """The keys of the ``transformers`` module, under the model's prefix unless ``prefix`` says otherwise
        (``lm_head.*`` carries none); ``weight_norm``: "parametrizations" (torch >= 2.1 modules) or "weight_g" (old
        checkpoints)."""
        prefix = self.PREFIX if prefix is None else prefix
        if weight_norm not in ("parametrizations", "weight_g"):
            raise ValueError(f"weight_norm 'parametrizations' or 'weight_g', got {weight_norm!r}")
        rename = dict(zip(*_POS_SPELLINGS)) if weight_norm == "parametrizations" else {}
        return {("" if k.startswith("lm_head.") else prefix) + rename.get(k, k): t.clone() for k, t in self.tensors.items()}

    def pos_weight(self) -> torch.Tensor:
        """The positional convolution's weight, w = g v / ||v|| with the norm over dims (0, 1) per tap
        (``weight_norm(dim=2)``), folded in fp64 -> fp64 [hidden, hidden / groups, k]."""
        v = self.tensors[_POS + "weight_v"].double()
        return self.tensors[_POS + "weight_g"].double() * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()

    def to(self, device=None, dtype=None) -> dict:
        """Canonical key -> tensor of ``device`` / ``dtype`` for the torch statement; ``pos_weight`` is the fold.  The
        last conversion is kept, so a statement called again on the same device does not move the weights again."""
        key = (torch.device(device) if device is not None else None, dtype)
        if getattr(self, "_converted", (None, None))[0] != key:
            out = {k: t.to(device=device, dtype=dtype) for k, t in self.tensors.items()
                   if not k.startswith(_POS + "weight_")}
            out["pos_weight"] = self.pos_weight().to(device=device, dtype=dtype)
            self._converted = (key, out)
        return self._converted[1]

    def device_pack(self, device):
        """-> (struct Wav2vecWeights, the device tensors it points to): every matrix [K][N] as csrc/wav2vec.hip reads
        it (include/instag_wav2vec.h)."""
        from . import _lib
        d, t = self.dims, self.tensors
        keep = []

        def put(x):
            x = x.to(dtype=torch.float32).contiguous().to(device)
            keep.append(x)
            return x.data_ptr()

        s = _lib.Wav2vecWeights()
        for field, value in asdict(d).items():
            setattr(s, field, value)
        for i in range(7):
            p = f"feature_extractor.conv_layers.{i}."
            w = t[p + "conv.weight"]                                            # [cout, cin, k] -> [(k, cin)][cout]
            s.conv_w[i] = put(w.permute(2, 1, 0).reshape(-1, d.conv_dim))
            s.conv_b[i], s.conv_ln_g[i], s.conv_ln_b[i] = put(t[p + "conv.bias"]), put(t[p + "layer_norm.weight"]), \
                put(t[p + "layer_norm.bias"])
        s.proj_ln_g, s.proj_ln_b = put(t["feature_projection.layer_norm.weight"]), put(t["feature_projection.layer_norm.bias"])
        s.proj_w, s.proj_b = put(t["feature_projection.projection.weight"].t()), put(t["feature_projection.projection.bias"])
        cg = d.hidden // d.pos_groups                                           # [G, cout, cin, k] -> [G][(k, cin)][cout]
        s.pos_w = put(self.pos_weight().reshape(d.pos_groups, cg, cg, d.pos_kernel).permute(0, 3, 2, 1).float())
        s.pos_b = put(t[_POS + "bias"])
        s.enc_ln_g, s.enc_ln_b = put(t["encoder.layer_norm.weight"]), put(t["encoder.layer_norm.bias"])
        if self.HEAD:
            s.head_w, s.head_b = put(t["lm_head.weight"].t()), put(t["lm_head.bias"])
        for l in range(d.layers):
            p = f"encoder.layers.{l}."
            qkv = [p + f"attention.{n}_proj." for n in "qkv"]
            s.ln1_g[l], s.ln1_b[l] = put(t[p + "layer_norm.weight"]), put(t[p + "layer_norm.bias"])
            s.qkv_w[l] = put(torch.cat([t[n + "weight"].t() for n in qkv], dim=1))
            s.qkv_b[l] = put(torch.cat([t[n + "bias"] for n in qkv]))
            s.out_w[l], s.out_b[l] = put(t[p + "attention.out_proj.weight"].t()), put(t[p + "attention.out_proj.bias"])
            s.ln2_g[l], s.ln2_b[l] = put(t[p + "final_layer_norm.weight"]), put(t[p + "final_layer_norm.bias"])
            s.ff1_w[l] = put(t[p + "feed_forward.intermediate_dense.weight"].t())
            s.ff1_b[l] = put(t[p + "feed_forward.intermediate_dense.bias"])
            s.ff2_w[l] = put(t[p + "feed_forward.output_dense.weight"].t())
            s.ff2_b[l] = put(t[p + "feed_forward.output_dense.bias"])
        return s, keep


class Wav2Vec2Weights(EncoderWeights):
    """The parameters of a ``Wav2Vec2ForCTC``: keys without the ``wav2vec2.`` prefix, ``lm_head.*`` among them."""


# ---- plain-torch statement -------------------------------------------------------------------------------------------
def wav2vec2_torch(weights: Wav2Vec2Weights, segments, taps=None):
    """``Wav2Vec2ForCTC(input_values=normalised segments).logits`` in eval mode, segments [B,n] -> [B,T,V], in the
    segments' dtype on their device; no attention mask.  ``taps``: a list that receives (name, tensor) of every stage,
    the attention probabilities [B,heads,T,T] of every layer among them."""
    x = torch.as_tensor(segments)
    if x.dim() != 2 or x.shape[1] < 400:
        raise ValueError(f"wav2vec2: segments [B, n >= 400], got {tuple(x.shape)}")
    w = weights.to(x.device, x.dtype)
    x = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, keepdim=True, unbiased=False) + NORM_EPS)
    out = F.linear(encoder_torch(weights, x, taps), w["lm_head.weight"], w["lm_head.bias"])
    if taps is not None:
        taps.append(("logits", out))
    return out


def encoder_torch(weights: EncoderWeights, x, taps=None):
    """The network behind the samples' normalisation, up to and including the encoder's last LayerNorm: input values
    [B,n] -> [B,T,hidden].  What ``wav2vec2_torch`` and ``hubert.hubert_torch`` share."""
    d = weights.dims
    w = weights.to(x.device, x.dtype)

    def tap(name, v):
        if taps is not None:
            taps.append((name, v))
        return v

    def ln(v, prefix, dim):
        return F.layer_norm(v, (dim,), w[prefix + ".weight"], w[prefix + ".bias"], LN_EPS)

    x = x.unsqueeze(1)
    for i, stride in enumerate(CONV_STRIDE):
        p = f"feature_extractor.conv_layers.{i}."
        x = F.conv1d(x, w[p + "conv.weight"], w[p + "conv.bias"], stride=stride)
        x = tap(f"conv{i}", F.gelu(ln(x.transpose(1, 2), p + "layer_norm", d.conv_dim)).transpose(1, 2))
    x = x.transpose(1, 2)                                                              # [B, T, conv_dim]
    h = tap("projection", F.linear(ln(x, "feature_projection.layer_norm", d.conv_dim),
                                   w["feature_projection.projection.weight"], w["feature_projection.projection.bias"]))
    pos = F.conv1d(h.transpose(1, 2), w["pos_weight"], w[_POS + "bias"], padding=d.pos_kernel // 2, groups=d.pos_groups)
    h = tap("positional", h + F.gelu(pos[..., :-1]).transpose(1, 2))
    B, T, _ = h.shape
    for l in range(d.layers):
        p = f"encoder.layers.{l}."
        y = ln(h, p + "layer_norm", d.hidden)
        q, k, v = (F.linear(y, w[p + f"attention.{n}_proj.weight"], w[p + f"attention.{n}_proj.bias"])
                   .view(B, T, d.heads, HEAD_DIM).transpose(1, 2) for n in "qkv")
        probs = tap(f"layer{l}.attn_probs", torch.softmax((q * HEAD_DIM ** -0.5) @ k.transpose(2, 3), dim=-1))
        ctx = (probs @ v).transpose(1, 2).reshape(B, T, d.hidden)
        h = tap(f"layer{l}.attention", h + F.linear(ctx, w[p + "attention.out_proj.weight"], w[p + "attention.out_proj.bias"]))
        y = F.gelu(F.linear(ln(h, p + "final_layer_norm", d.hidden), w[p + "feed_forward.intermediate_dense.weight"],
                            w[p + "feed_forward.intermediate_dense.bias"]))
        h = tap(f"layer{l}.feed_forward", h + F.linear(y, w[p + "feed_forward.output_dense.weight"],
                                                       w[p + "feed_forward.output_dense.bias"]))
    return ln(h, "encoder.layer_norm", d.hidden)


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class SegmentEncoder(DeviceOperator):
    """The one body of ``Wav2Vec2CTC`` and ``hubert.HubertEncoder``: ``_encode(segments [B,n]) -> [B,T,.]``, fp32 on
    ``device``, on torch's current stream; inference only.  On the GPU the segments go through the ``ENTRY``'s C entry
    points in chunks of at most ``max_batch`` with the one kept workspace of device_op.DeviceOperator; the default
    ``max_batch`` is the largest whose workspace for segments of ``SAMPLES`` samples stays within WORKSPACE_LIMIT.  On a
    CPU device it is the torch statement.  ``tile``: 0, or 1..3 to pin the GEMM tile (the tests hold the tiles against
    each other bit for bit).  A subclass states the names below."""

    ENTRY = ""               # instag_<ENTRY>_{workspace_bytes, taps_floats, forward}
    STATEMENT = None         # staticmethod: the torch statement (weights, segments, taps)
    OUTPUT = ""              # the field of the dimensions that is the output's last dimension
    DROPPED = ""             # the statement's tap that is the output itself
    SAMPLES = 0              # the segment length the default max_batch is sized for
    INPUT = "segments"       # what the messages call the input

    def __init__(self, weights: EncoderWeights, device="cuda", max_batch=None, tile: int = 0):
        self.max_batch, self.tile = self._at_least_one(max_batch), int(tile)
        super().__init__(weights, device)
        if self.max_batch is None and self.device.type == "cuda":
            self.max_batch = self.default_max_batch(weights.dims)

    @classmethod
    def default_max_batch(cls, dims: Wav2Vec2Dims) -> int:
        """The largest batch whose workspace for segments of ``SAMPLES`` samples stays within WORKSPACE_LIMIT (the entry
        point works out the size from the dimensions alone: no weights, no GPU)."""
        from . import _lib
        s = _lib.Wav2vecWeights()
        for field, value in asdict(dims).items():
            setattr(s, field, value)
        one = _lib.workspace_bytes(cls._entry("workspace_bytes")(C.byref(s), 1, cls.SAMPLES))
        return max(1, min(4096, (WORKSPACE_LIMIT - 4096) // one))

    @classmethod
    def _entry(cls, name):
        from . import _lib
        return getattr(_lib.lib(), f"instag_{cls.ENTRY}_{name}")

    @torch.no_grad()
    def _encode(self, segments, taps=None):
        x = torch.as_tensor(segments)
        if x.dim() != 2:
            raise ValueError(f"{type(self).__name__}: {self.INPUT} [B,n], got {tuple(x.shape)}")
        x = x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if self.device.type != "cuda":
            return self._statement(self.STATEMENT, x, taps, ("attn_probs", self.DROPPED))
        from . import _lib
        B, n = x.shape
        w, d, T = C.byref(self._struct), self.weights.dims, frames_of(n)
        # (refuses a segment that is too short or too long)
        nbytes = _lib.workspace_bytes(self._entry("workspace_bytes")(w, max(1, min(B, self.max_batch)), n))
        out = torch.empty(B, T, getattr(d, self.OUTPUT), dtype=torch.float32, device=self.device)
        flat = None if taps is None else self._taps_buffer(self._entry("taps_floats")(w, B, n), B)
        forward = self._entry("forward")
        self._each_chunk(B, nbytes, lambda c, m, ws, size: forward(
            w, _lib.ptr(x[c]), m, n, _lib.ptr(out[c]), ws, size, self.tile, _lib.ptr(flat), _lib.current_stream()),
            f"{self.ENTRY}_forward")
        if taps is not None:
            rows = [n]
            for k, s in zip(CONV_KERNEL, CONV_STRIDE):
                rows.append((rows[-1] - k) // s + 1)
            stages = [(f"conv{l}", (B, t, d.conv_dim)) for l, t in enumerate(rows[1:])]
            stages += [(name, (B, T, d.hidden)) for name in ["projection", "positional"] + [
                f"layer{l}.{part}" for l in range(d.layers) for part in ("attention", "feed_forward")]]
            taps += [(name, v.transpose(1, 2) if name.startswith("conv") else v) for name, v in self._cut(flat, stages)]
        return out


class Wav2Vec2CTC(SegmentEncoder):
    """``logits(segments [B,n]) -> [B,T,V]`` through csrc/wav2vec.hip (SegmentEncoder); the default ``max_batch`` is
    sized for full runs of 22,400 samples."""
    ENTRY, STATEMENT, OUTPUT, DROPPED, SAMPLES = "wav2vec", staticmethod(wav2vec2_torch), "vocab", "logits", RUN_SAMPLES

    def logits(self, segments, taps=None):
        """``taps``: a list that receives (name, tensor) of every stage as ``wav2vec2_torch``'s does, but for the
        attention probabilities (debug: one chunk only, B <= max_batch)."""
        return self._encode(segments, taps)


# ---- the streaming rule and the features ----------------------------------------------------------------------------
def segment_plan(n_samples: int):
    """The runs of the reference's file mode over ``n_samples`` of audio, as a list of
    (start_chunk, zero_chunks, length, left, right): the run is ``zero_chunks`` chunks of 320 zeros followed by the audio
    from chunk ``start_chunk`` on, ``length`` samples in all, and rows [left, right) of its logits are kept.

    The rule (wav2vec.py -l 10 -m 50 -r 10): ten zero chunks, then the audio chunk by chunk (the last may be short);
    whenever 70 chunks are held the network runs on them and the last 20 stay; at the end it runs once more on what is
    held.  With v the position in (10 zero chunks + audio chunks), run r before the last covers v in [50 r, 50 r + 70)
    and the last one [50 R, 10 + chunks).  A run before the last keeps rows [10, T - 9), the last [10, T)."""
    n = int(n_samples)
    if n < 0:
        raise ValueError(f"segment_plan: n_samples >= 0, got {n}")
    chunks = -(-n // CHUNK)
    held = PREFIX_CHUNKS + chunks
    step = RUN_CHUNKS - KEPT_CHUNKS
    full_runs = (held - RUN_CHUNKS) // step + 1 if held >= RUN_CHUNKS else 0
    short = chunks * CHUNK - n                          # what the last audio chunk lacks
    plan = []
    for r in range(full_runs + 1):
        last = r == full_runs
        a, b = step * r, (held if last else step * r + RUN_CHUNKS)
        length = CHUNK * (b - a) - (short if b == held else 0)
        T = (length - 400) // CHUNK + 1
        right = T if last else min(T, T - (CONTEXT_ROWS - 1))
        zero_chunks = min(max(PREFIX_CHUNKS - a, 0), b - a)
        plan.append((max(a - PREFIX_CHUNKS, 0), zero_chunks, length, CONTEXT_ROWS, max(right, CONTEXT_ROWS)))
    return plan


def unfold_rows(rows: torch.Tensor) -> torch.Tensor:
    """[M,V] -> [M // 2 + 1, 16, V]: out[i, w] = padded[2 i + w] with eight zero rows on each side (the reference's
    ``F.unfold`` with kernel 16, padding 8, stride 2)."""
    M = rows.shape[0]
    padded = torch.cat([rows.new_zeros(WINDOW_PAD, rows.shape[1]), rows, rows.new_zeros(WINDOW_PAD, rows.shape[1])], dim=0)
    idx = WINDOW_STRIDE * torch.arange(M // 2 + 1)[:, None] + torch.arange(WINDOW)[None]
    return padded[idx.to(rows.device)]


def esperanto_features(wav16k, weights: Wav2Vec2Weights, device="cuda", encoder=None) -> np.ndarray:
    """The array the reference saves as aud_eo.npy for 16 kHz samples [L], fp32 [M // 2 + 1, 16, 44].  All full runs
    (22,400 samples) go to the network as one batch, the others alone.  ``encoder`` is called as
    ``encoder(weights, segments)`` in place of the HIP operator -- the tests' comparand."""
    x = torch.as_tensor(wav16k)
    if x.dim() != 1:
        raise ValueError(f"esperanto_features: samples [L], got {tuple(x.shape)}")
    device = torch.device(device)
    x = x.to(device=device, dtype=torch.float32)
    plan = segment_plan(x.numel())
    runs = [torch.cat([x.new_zeros(z * CHUNK), x[s * CHUNK: s * CHUNK + n - z * CHUNK]]) for s, z, n, _, _ in plan]
    if encoder is None:
        op = Wav2Vec2CTC(weights, device)
        encoder = lambda _, segments: op.logits(segments)          # noqa: E731
    kept = [None] * len(plan)
    full = [i for i, run in enumerate(runs) if run.numel() == RUN_SAMPLES and plan[i][4] > plan[i][3]]
    with torch.no_grad():
        if full:
            out = encoder(weights, torch.stack([runs[i] for i in full]))
            for j, i in enumerate(full):
                kept[i] = out[j, plan[i][3]:plan[i][4]]
        for i, run in enumerate(runs):
            if kept[i] is None and plan[i][4] > plan[i][3]:
                kept[i] = encoder(weights, run[None])[0, plan[i][3]:plan[i][4]]
    rows = [k.float() for k in kept if k is not None]
    rows = torch.cat(rows, dim=0) if rows else x.new_zeros(0, weights.dims.vocab)
    return unfold_rows(rows.cpu()).contiguous().numpy()
