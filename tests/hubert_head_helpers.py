"""Shared by the 'hubert' head tests and tests/golden/make_golden_hubert_head.py: the closed-form audio-branch weights
of golden G18.

G18 stores no weights (encoder_conv.0.weight alone is 1.5 MB).  Instead every tensor of ``audio_net``,
``audio_att_net`` and ``exp_encode_net`` is set by ``closed_form``: small integers over a power of two, exact in fp32
(and fp16), of both signs so that both sides of every LeakyReLU occur.  The generator loads the rule into the
reference's modules, the tests into the package's."""
from types import SimpleNamespace

import torch

from tests.ave_helpers import closed_form, enc_weights  # noqa: F401  (the same rule and the same scalar)

# tag -> (network class name, args.type, takes the expression vector); the position is the tag's salt in the rule
NETWORKS = (("umf", "MotionNetwork", "face", True), ("pmf_face", "PersonalizedMotionNetwork", "face", True),
            ("pmf_mouth", "PersonalizedMotionNetwork", "mouth", False), ("mouth", "MouthMotionNetwork", "mouth", False))

# divisor per tensor: a sum of n live terms of magnitude ~5 / divisor against inputs of magnitude ~1 grows like
# 5 sqrt(n) / divisor, so divisors near 5 sqrt(n) keep it near one: n = 2048 live taps in encoder_conv.0 (two of three
# taps x 1024 channels), 128 and 64 in the layers behind it (the centre taps)
_DIVISORS = {
    "audio_net.encoder_conv.0.weight": 256.0, "audio_net.encoder_conv.0.bias": 16.0,
    "audio_net.encoder_conv.2.weight": 64.0, "audio_net.encoder_conv.2.bias": 16.0,
    "audio_net.encoder_conv.4.weight": 64.0, "audio_net.encoder_conv.4.bias": 16.0,
    "audio_net.encoder_conv.6.weight": 32.0, "audio_net.encoder_conv.6.bias": 16.0,
    "audio_net.encoder_fc1.0.weight": 32.0, "audio_net.encoder_fc1.0.bias": 16.0,
    "audio_net.encoder_fc1.2.weight": 32.0, "audio_net.encoder_fc1.2.bias": 16.0,
    "audio_att_net.attentionConvNet.0.weight": 64.0, "audio_att_net.attentionConvNet.0.bias": 16.0,
    "audio_att_net.attentionConvNet.2.weight": 32.0, "audio_att_net.attentionConvNet.2.bias": 16.0,
    "audio_att_net.attentionConvNet.4.weight": 16.0, "audio_att_net.attentionConvNet.4.bias": 16.0,
    "audio_att_net.attentionConvNet.6.weight": 8.0, "audio_att_net.attentionConvNet.6.bias": 16.0,
    "audio_att_net.attentionConvNet.8.weight": 8.0, "audio_att_net.attentionConvNet.8.bias": 16.0,
    "audio_att_net.attentionNet.0.weight": 8.0, "audio_att_net.attentionNet.0.bias": 16.0,
    "exp_encode_net.net.0.weight": 8.0, "exp_encode_net.net.1.weight": 8.0,
}
AUDIO_KEYS = tuple(_DIVISORS)
assert len(AUDIO_KEYS) == 26


def load_closed_form(net, salt: int):
    """Set the per-frame branch of ``net`` (any of the four networks, the reference's or the package's) by the rule;
    a network without the expression branch has 24 of the 26 tensors."""
    sd = net.state_dict()
    with torch.no_grad():
        for k, key in enumerate(AUDIO_KEYS):
            if key in sd:
                sd[key].copy_(closed_form(sd[key].shape, salt * 32 + k, _DIVISORS[key]).to(sd[key].dtype))
    return net


def hubert_args(kind: str):
    return SimpleNamespace(audio_extractor="hubert", type=kind)


def build_network(tag: str, encoder_cls=None, module=None):
    """Network ``tag`` of NETWORKS with audio_extractor == 'hubert' from ``module`` (default: instag_amd.motion_net)."""
    if module is None:
        from instag_amd import motion_net as module
    salt, (_, cls, kind, _) = next((i, n) for i, n in enumerate(NETWORKS) if n[0] == tag)
    kw = {} if encoder_cls is None else dict(encoder_cls=encoder_cls)
    return getattr(module, cls)(args=hubert_args(kind), **kw), salt


BIAS_KEYS = tuple(f"audio_net.encoder_conv.{i}.bias" for i in (0, 2, 4, 6)) + \
    tuple(f"audio_net.encoder_fc1.{i}.bias" for i in (0, 2))
CONV1_KEY = "audio_net.encoder_conv.0.weight"        # G18 records the gradient of its first CONV1_ROWS rows
CONV1_ROWS = 4
