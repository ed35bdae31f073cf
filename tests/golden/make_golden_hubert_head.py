"""Generate golden G18 (tests/golden/g18_hubert_head.npz): the reference's four motion networks built with
audio_extractor='hubert', per-frame audio branch only.

Run in the build container only (needs the reference checkout; never on the GPU box), on the CPU:

    python tests/golden/make_golden_hubert_head.py

The reference's scene/motion_net.py is imported the way make_golden_ave.py does it.  No weights are stored: the branch
of every network is set by the closed-form rule of tests/hubert_head_helpers.py, which the tests load into the
package's modules too.  Stored: the window a [8, 1024, 2] (fp16 quarter-integers), per network enc_a in fp64, the fp64
gradients of (enc_a * w).sum() with respect to the six AudioNet biases and the first four rows of
encoder_conv.0.weight, the attention weights of the softmax (checked here: none above 0.9), and the sorted state_dict
names and shapes.
"""
import sys
sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_ave import _reference_motion_net  # noqa: E402


def hubert_head_nets():
    mn = _reference_motion_net()
    from tests import hubert_head_helpers as H
    torch.manual_seed(41)
    # quarter-integer samples: exact in fp32 and fp16 (the window is stored as fp16)
    a = (torch.randn(8, 1024, 2, generator=torch.Generator().manual_seed(43)) * 4).round() / 4
    res = dict(a=a.numpy().astype(np.float16))
    assert np.array_equal(res["a"].astype(np.float32), a.numpy())
    layout = {}
    for tag, _, _, _ in H.NETWORKS:
        net, salt = H.build_network(tag, module=mn)
        layout[tag] = sorted((k, list(v.shape)) for k, v in net.state_dict().items())
        assert tuple(net.audio_net.encoder_conv[0].weight.shape) == (128, 1024, 3)
        H.load_closed_form(net, salt)
        net = net.double()
        feat = net.audio_net(a.double())                                   # [8, dim_aud]
        y = net.audio_att_net.attentionNet(net.audio_att_net.attentionConvNet(feat.unsqueeze(0).permute(0, 2, 1))
                                           .view(1, 8))
        assert float(y.detach().max()) < 0.9, (tag, y)                     # the softmax over the windows is not saturated
        assert float((feat > 0).double().mean()) > 0.1 and float((feat < 0).double().mean()) > 0.1
        enc_a = net.encode_audio(a.double())
        assert enc_a.dtype == torch.float64 and tuple(enc_a.shape) == (1, net.audio_dim)
        (enc_a * H.enc_weights(net.audio_dim)).sum().backward()
        params = dict(net.named_parameters())
        res[f"{tag}.enc_a"] = enc_a.detach().numpy()
        res[f"{tag}.softmax"] = y.detach().numpy()
        for k in H.BIAS_KEYS:
            res[f"{tag}.grad.{k}"] = params[k].grad.numpy()
        res[f"{tag}.grad.{H.CONV1_KEY}"] = params[H.CONV1_KEY].grad[:H.CONV1_ROWS].numpy()
    res["layout"] = np.frombuffer(json.dumps(layout).encode(), dtype=np.uint8)
    out = f"{HERE}/g18_hubert_head.npz"
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")
    for tag, _, _, _ in H.NETWORKS:
        print(tag, "softmax max", float(res[f"{tag}.softmax"].max()), "|enc_a| max", float(np.abs(res[f"{tag}.enc_a"]).max()),
              "|d conv1| max", float(np.abs(res[f"{tag}.grad.{H.CONV1_KEY}"]).max()))


if __name__ == "__main__":
    hubert_head_nets()
