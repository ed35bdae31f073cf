"""Generate golden G8 (tests/golden/g8_ave_nets.npz): the reference's four motion networks built with
audio_extractor='ave', audio branch only.

Run in the build container only (needs the reference checkout; never on the GPU box), on the CPU:

    python tests/golden/make_golden_ave.py

The reference's scene/motion_net.py is imported the way make_golden.py does it (the oracle grid encoder injected as
`gridencoder`, the CUDA extensions never imported).  No weights are stored: the audio branch of every network is set
by the closed-form rule of tests/ave_helpers.py, which the tests load into the package's modules too.  Stored: the
window a [8, 1, 512], per network enc_a in fp64, the fp64 gradients of (enc_a * w).sum() with respect to the three
AudioNet_ave biases and encoder_fc1.4.weight, the attention weights of the softmax (checked here: none above 0.9),
and the sorted state_dict names and shapes.
"""
import sys
sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree
import importlib.util
import json
import os
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _reference_motion_net():
    sys.path.insert(0, ROOT)
    from oracle import grid_torch
    fake = types.ModuleType("gridencoder")
    fake.GridEncoder = grid_torch.GridEncoder
    sys.modules["gridencoder"] = fake
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("ref_motion_net_ave", f"{REF}/scene/motion_net.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.path.remove(REF)
    return mod


def ave_nets():
    mn = _reference_motion_net()
    from tests import ave_helpers as H
    torch.manual_seed(41)
    # quarter-integer samples: exact in fp32 and fp16 (the window is stored as fp16)
    a = (torch.randn(8, 1, 512, generator=torch.Generator().manual_seed(42)) * 4).round() / 4
    res = dict(a=a.numpy().astype(np.float16))
    assert np.array_equal(res["a"].astype(np.float32), a.numpy())
    layout = {}
    for tag, _, _, _ in H.NETWORKS:
        net, salt = H.build_network(tag, module=mn)
        layout[tag] = sorted((k, list(v.shape)) for k, v in net.state_dict().items())
        H.load_closed_form(net, salt)
        net = net.double()
        feat = net.audio_net(a.double())                                   # [8, dim_aud]
        y = net.audio_att_net.attentionNet(net.audio_att_net.attentionConvNet(feat.unsqueeze(0).permute(0, 2, 1))
                                           .view(1, 8))
        assert float(y.detach().max()) < 0.9, (tag, y)                              # the softmax over the windows is not saturated
        assert float((feat > 0).double().mean()) > 0.1 and float((feat < 0).double().mean()) > 0.1
        enc_a = net.encode_audio(a.double())
        assert enc_a.dtype == torch.float64 and tuple(enc_a.shape) == (1, net.audio_dim)
        (enc_a * H.enc_weights(net.audio_dim)).sum().backward()
        params = dict(net.named_parameters())
        res[f"{tag}.enc_a"] = enc_a.detach().numpy()
        res[f"{tag}.softmax"] = y.detach().numpy()
        for k in H.GRAD_KEYS:
            res[f"{tag}.grad.{k}"] = params[k].grad.numpy()
    res["layout"] = np.frombuffer(json.dumps(layout).encode(), dtype=np.uint8)
    out = f"{HERE}/g8_ave_nets.npz"
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")
    for tag, _, _, _ in H.NETWORKS:
        print(tag, "softmax max", float(res[f"{tag}.softmax"].max()), "|enc_a| max", float(np.abs(res[f"{tag}.enc_a"]).max()))


if __name__ == "__main__":
    ave_nets()
