"""Generate golden G14 (tests/golden/g14_parsing.npz): the reference's BiSeNet(19) (data_utils/face_parsing/model.py,
resnet.py) in eval mode and fp64 on one seeded 64 x 96 frame.

Run in the build container only (needs the reference checkout; never on the GPU box), on the CPU:

    python tests/golden/make_golden_parsing.py

The reference's modules are loaded by file path.  ``Resnet18.__init__`` fetches ImageNet weights through
``torch.utils.model_zoo.load_url`` and model.py imports torchvision, which it never uses; before any reference module
is executed ``load_url`` is replaced by a function that returns an empty dict (nothing is fetched, the construction
keeps its own initialisation) and an empty module stands in for torchvision.  No weights are stored: the seeded rule
of tests/parsing_helpers.py is loaded into the reference module under the checkpoint's own keys.  Stored: the u8 frame
[64,96,3], the fp64 logits at 1/8 resolution (the output of ``conv_out``), the fp64 full-size logits and the labels,
every stage's fraction of positive units, and the state-dict names and shapes.
"""
import sys
sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree
import importlib.util
import json
import os
import types

import numpy as np
import torch
import torch.utils.model_zoo

REF = "/root/reference/data_utils/face_parsing"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _reference_model():
    torch.utils.model_zoo.load_url = lambda *a, **k: {}
    sys.modules["torchvision"] = types.ModuleType("torchvision")

    def load(name, file):
        spec = importlib.util.spec_from_file_location(name, f"{REF}/{file}")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    load("resnet", "resnet.py")
    return load("ref_face_parsing_model", "model.py")


def parsing():
    model_py = _reference_model()
    sys.path.insert(0, ROOT)
    from tests import parsing_helpers as H
    net = model_py.BiSeNet(19)
    ckpt = H.state_dict()
    net.load_state_dict(ckpt)                                      # strict: the rule gives a complete checkpoint
    net = net.eval().double()
    layout = sorted((k, list(v.shape)) for k, v in ckpt.items())
    assert len(layout) == 191 and sum(int(np.prod(s)) if s else 1 for _, s in layout) == 13313119

    frame = H.seeded_frames(1, H.G14_H, H.G14_W)
    mean = np.array([0.485, 0.456, 0.406])
    std = np.array([0.229, 0.224, 0.225])
    x = torch.from_numpy(((frame.numpy().astype(np.float64) / 255.0 - mean) / std).transpose(0, 3, 1, 2).copy())

    taps, low = [], []
    stages = [net.cp.resnet.layer1[0], net.cp.resnet.layer1[1], net.cp.resnet.layer2[0], net.cp.resnet.layer2[1],
              net.cp.resnet.layer3[0], net.cp.resnet.layer3[1], net.cp.resnet.layer4[0], net.cp.resnet.layer4[1],
              net.cp.conv_avg, net.cp.arm32.conv, net.cp.conv_head32, net.cp.arm16.conv, net.cp.conv_head16,
              net.ffm.convblk, net.conv_out.conv]
    hooks = [m.register_forward_hook(lambda m, i, o: taps.append(o.detach())) for m in stages]
    # the stem's ReLU is functional: its output is the max-pool's input
    hooks.append(net.cp.resnet.maxpool.register_forward_hook(lambda m, i, o: taps.insert(0, i[0].detach())))
    hooks.append(net.conv_out.register_forward_hook(lambda m, i, o: low.append(o.detach())))
    with torch.no_grad():
        full = net(x)
    for h in hooks:
        h.remove()
    assert full.dtype == torch.float64 and tuple(full.shape) == (1, 19, H.G14_H, H.G14_W)
    assert len(taps) == 16 and tuple(low[0].shape) == (1, 19, H.G14_H // 8, H.G14_W // 8)
    positive = H.liveness(taps)
    assert all(0.2 <= p <= 0.8 for p in positive), positive       # every stage is alive on both sides
    labels = full[0].numpy().argmax(0).astype(np.uint8)           # test.py:101
    assert len(np.unique(labels)) >= 5, np.unique(labels)

    res = dict(frame=frame[0].numpy(), logits8=low[0][0].numpy(), full=full[0].numpy(), labels=labels,
               positive=np.asarray(positive), layout=np.frombuffer(json.dumps(layout).encode(), dtype=np.uint8))
    path = f"{HERE}/g14_parsing.npz"
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("positive fraction per stage", [round(p, 3) for p in positive], "labels", np.unique(labels).tolist(),
          "max |logit|", float(low[0].abs().max()))
    with torch.no_grad():
        full32 = net.float()(x.float()).double()
    top = full.topk(2, dim=1).values
    print("fp32 torch vs fp64: relative to max |logit|", float((full32 - full).abs().max() / full.abs().max()),
          "labels differing", int((full32[0].numpy().argmax(0) != labels).sum()),
          "smallest top-two margin", float((top[:, 0] - top[:, 1]).min()))


if __name__ == "__main__":
    parsing()
