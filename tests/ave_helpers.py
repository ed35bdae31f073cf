"""Shared by the 'ave' tests and tests/golden/make_golden_ave.py: the closed-form audio-branch weights of golden G8.

G8 stores no weights (the first AudioNet_ave layer alone is 512 KB).  Instead every tensor of ``audio_net`` and
``audio_att_net`` is set by ``closed_form``: small integers over a power of two, exact in fp32 (and fp16), of both
signs so that both sides of every LeakyReLU occur.  The generator loads the rule into the reference's modules, the
tests into the package's."""
from types import SimpleNamespace

import torch

# tag -> (network class name, args.type, takes the expression vector); the position is the tag's salt in the rule
NETWORKS = (("umf", "MotionNetwork", "face", True), ("pmf_face", "PersonalizedMotionNetwork", "face", True),
            ("pmf_mouth", "PersonalizedMotionNetwork", "mouth", False), ("mouth", "MouthMotionNetwork", "mouth", False))

# divisor per audio-branch tensor: sums of n terms of magnitude ~4 / divisor stay near one
_DIVISORS = {
    "audio_net.encoder_fc1.0.weight": 128.0, "audio_net.encoder_fc1.0.bias": 16.0,
    "audio_net.encoder_fc1.2.weight": 64.0, "audio_net.encoder_fc1.2.bias": 16.0,
    "audio_net.encoder_fc1.4.weight": 32.0, "audio_net.encoder_fc1.4.bias": 16.0,
    "audio_att_net.attentionConvNet.0.weight": 64.0, "audio_att_net.attentionConvNet.0.bias": 16.0,
    "audio_att_net.attentionConvNet.2.weight": 32.0, "audio_att_net.attentionConvNet.2.bias": 16.0,
    "audio_att_net.attentionConvNet.4.weight": 16.0, "audio_att_net.attentionConvNet.4.bias": 16.0,
    "audio_att_net.attentionConvNet.6.weight": 8.0, "audio_att_net.attentionConvNet.6.bias": 16.0,
    "audio_att_net.attentionConvNet.8.weight": 8.0, "audio_att_net.attentionConvNet.8.bias": 16.0,
    "audio_att_net.attentionNet.0.weight": 8.0, "audio_att_net.attentionNet.0.bias": 16.0,
}
AUDIO_KEYS = tuple(_DIVISORS)


def closed_form(shape, salt: int, divisor: float) -> torch.Tensor:
    """v[i] = ((i * i * 3 + i * 7 + salt * 11) mod 17 - 8) / divisor over the flat index i (fp64: every value is exact
    in fp32 as well)."""
    n = 1
    for s in shape:
        n *= int(s)
    i = torch.arange(n, dtype=torch.int64)
    return (((i * i * 3 + i * 7 + salt * 11) % 17 - 8).double() / divisor).reshape(tuple(shape))


def load_closed_form(net, salt: int):
    """Set the audio branch of ``net`` (any of the four networks, the reference's or the package's) by the rule."""
    sd = net.state_dict()
    with torch.no_grad():
        for k, key in enumerate(AUDIO_KEYS):
            sd[key].copy_(closed_form(sd[key].shape, salt * 32 + k, _DIVISORS[key]).to(sd[key].dtype))
    return net


def enc_weights(dim_aud: int) -> torch.Tensor:
    """w of the scalar (enc_a * w).sum() whose gradients G8 records."""
    j = torch.arange(dim_aud, dtype=torch.int64)
    return ((j * 5) % 7 - 3).double() / 4.0


def ave_args(kind: str):
    return SimpleNamespace(audio_extractor="ave", type=kind)


def build_network(tag: str, encoder_cls=None, module=None):
    """Network ``tag`` of NETWORKS with audio_extractor == 'ave' from ``module`` (default: instag_amd.motion_net)."""
    if module is None:
        from instag_amd import motion_net as module
    salt, (_, cls, kind, _) = next((i, n) for i, n in enumerate(NETWORKS) if n[0] == tag)
    kw = {} if encoder_cls is None else dict(encoder_cls=encoder_cls)
    return getattr(module, cls)(args=ave_args(kind), **kw), salt


GRAD_KEYS = ("audio_net.encoder_fc1.0.bias", "audio_net.encoder_fc1.2.bias", "audio_net.encoder_fc1.4.bias",
             "audio_net.encoder_fc1.4.weight")
