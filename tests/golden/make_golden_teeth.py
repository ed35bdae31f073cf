"""Generate golden G15 (tests/golden/g15_teeth.npz): the reference's fpn-fp segmentor -- ``ResNetV1c`` (depth 50),
``FPN`` and ``FPNHead`` of data_utils/easyportrait/mmseg, built from the ``model`` dict of
local_configs/easyportrait_experiments_v2/fpn-fp/fpn-fp.py -- in eval mode and fp64 on one seeded 64 x 96 frame.

Run in the build container only (needs the reference checkout; never on the GPU box), on the CPU:

    python tests/golden/make_golden_teeth.py

The reference's modules (backbones/resnet.py, utils/res_layer.py, necks/fpn.py, decode_heads/decode_head.py and
decode_heads/fpn_head.py) are loaded by file path.  They import mmcv, which is not installed: before any reference
module is executed, plain-torch stand-ins are registered for exactly what those files import, together with empty parent
packages so that their relative imports resolve -- ``build_conv_layer`` -> ``nn.Conv2d``, ``build_norm_layer`` ->
``("bn<postfix>", nn.BatchNorm2d)``, ``build_plugin_layer`` (unused), ``ConvModule`` (``conv`` [+ ``bn``] [+
``activate``], a bias exactly when there is no norm), ``BaseModule`` / ``Sequential`` -> ``nn.Module`` /
``nn.Sequential``, ``auto_fp16`` / ``force_fp32`` -> identity, ``_BatchNorm``, ``mmseg.ops.resize`` ->
``F.interpolate`` and ``Upsample`` on it, registries whose ``register_module()`` returns the class, and, for the head's
base class, ``build_loss`` / ``build_pixel_sampler`` / ``accuracy`` that build nothing.  The head is the reference's own
``FPNHead`` loaded this way, not a restatement; what ``EncoderDecoder.encode_decode`` does around the three modules
(backbone, neck, ``forward_test``, the bilinear ``resize`` to the frame's size with ``align_corners=False``) is four
lines here, and ``label = argmax`` is create_teeth_mask.py's (the softmax in between is monotone).

No weights are stored: the seeded rule of tests/teeth_helpers.py is loaded strictly into the three modules under the
checkpoint's own keys.  Stored: the u8 frame [64,96,3], the fp64 logits at 1/4 resolution (the output of ``conv_seg``),
the fp64 full-size logits and the labels, every stage's fraction of positive units, and the state-dict names and shapes.
"""
import sys
sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree
import importlib.util
import json
import os
import runpy
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REF = "/root/reference/data_utils/easyportrait"
CONFIG = f"{REF}/local_configs/easyportrait_experiments_v2/fpn-fp/fpn-fp.py"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


class _ConvModule(nn.Module):
    def __init__(self, cin, cout, kernel_size, stride=1, padding=0, conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type="ReLU"), inplace=True):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=norm_cfg is None)
        if norm_cfg is not None:
            self.bn = nn.BatchNorm2d(cout)
        if act_cfg is not None:
            assert act_cfg["type"] == "ReLU"
            self.activate = nn.ReLU(inplace=inplace)

    def forward(self, x):
        x = self.conv(x)
        if hasattr(self, "bn"):
            x = self.bn(x)
        return self.activate(x) if hasattr(self, "activate") else x


class _BaseModule(nn.Module):
    def __init__(self, init_cfg=None):
        super().__init__()


class _Sequential(nn.Sequential):
    def __init__(self, *args, init_cfg=None):
        super().__init__(*args)


def _resize(input, size=None, scale_factor=None, mode="nearest", align_corners=None, warning=True):
    return F.interpolate(input, size, scale_factor, mode, align_corners)


class _Upsample(nn.Module):
    def __init__(self, size=None, scale_factor=None, mode="nearest", align_corners=None):
        super().__init__()
        self.scale_factor, self.mode, self.align_corners = float(scale_factor), mode, align_corners

    def forward(self, x):
        return _resize(x, [int(t * self.scale_factor) for t in x.shape[-2:]], None, self.mode, self.align_corners)


class _Registry:
    def register_module(self):
        return lambda cls: cls


def _stand_ins():
    def module(name, package=False, **attrs):
        m = types.ModuleType(name)
        if package:
            m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    identity = lambda *a, **k: (lambda f: f)
    module("mmcv", package=True)
    module("mmcv.cnn", ConvModule=_ConvModule,
           build_conv_layer=lambda cfg, *a, **k: nn.Conv2d(*a, **k),
           build_norm_layer=lambda cfg, n, postfix="": (f"bn{postfix}", nn.BatchNorm2d(n)),
           build_plugin_layer=None)
    module("mmcv.runner", BaseModule=_BaseModule, Sequential=_Sequential, auto_fp16=identity, force_fp32=identity)
    module("mmcv.utils", package=True)
    module("mmcv.utils.parrots_wrapper", _BatchNorm=nn.modules.batchnorm._BatchNorm)
    module("mmseg", package=True)
    module("mmseg.ops", resize=_resize, Upsample=_Upsample)
    module("mmseg.core", build_pixel_sampler=lambda *a, **k: None)
    module("mmseg.models", package=True)
    module("mmseg.models.builder", BACKBONES=_Registry(), NECKS=_Registry(), HEADS=_Registry(),
           build_loss=lambda cfg: nn.Module())
    module("mmseg.models.losses", accuracy=None)
    for pkg in ("utils", "backbones", "necks", "decode_heads"):
        module(f"mmseg.models.{pkg}", package=True)


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, f"{REF}/mmseg/models/{file}")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _reference_model():
    _stand_ins()
    sys.modules["mmseg.models.utils"].ResLayer = _load("mmseg.models.utils.res_layer", "utils/res_layer.py").ResLayer
    resnet = _load("mmseg.models.backbones.resnet", "backbones/resnet.py")
    fpn = _load("mmseg.models.necks.fpn", "necks/fpn.py")
    _load("mmseg.models.decode_heads.decode_head", "decode_heads/decode_head.py")
    head = _load("mmseg.models.decode_heads.fpn_head", "decode_heads/fpn_head.py")
    cfg = runpy.run_path(CONFIG)["model"]
    args = lambda d: {k: v for k, v in d.items() if k != "type"}
    assert (cfg["backbone"]["type"], cfg["neck"]["type"], cfg["decode_head"]["type"]) == ("ResNetV1c", "FPN", "FPNHead")
    net = nn.Module()
    net.backbone = resnet.ResNetV1c(**args(cfg["backbone"]))
    net.neck = fpn.FPN(**args(cfg["neck"]))
    net.decode_head = head.FPNHead(**args(cfg["decode_head"]))
    return net, cfg


def teeth():
    net, cfg = _reference_model()
    sys.path.insert(0, ROOT)
    from tests import teeth_helpers as H
    from instag_amd import teeth as T
    ckpt = H.state_dict()
    net.load_state_dict(ckpt)                                      # strict: the rule gives a complete state dict
    net = net.eval().double()
    layout = sorted((k, list(v.shape)) for k, v in ckpt.items())
    convs = sum(1 for k, s in layout if len(s) == 4)
    params = sum(int(np.prod(s)) for k, s in layout if s and not k.endswith(("running_mean", "running_var")))
    assert convs == 71 and cfg["decode_head"]["num_classes"] == 8 == ckpt["decode_head.conv_seg.weight"].shape[0]

    frame = H.seeded_frames(1, H.G15_H, H.G15_W)
    norm = cfg["decode_head"]["align_corners"], tuple(T.MEAN), tuple(T.STD)
    test_norm = runpy.run_path(CONFIG)["img_norm_cfg"]
    assert norm == (False, tuple(test_norm["mean"]), tuple(test_norm["std"])) and test_norm["to_rgb"]
    x = torch.from_numpy(((frame.numpy().astype(np.float64) - np.array(test_norm["mean"])) / np.array(test_norm["std"]))
                         .transpose(0, 3, 1, 2).copy())

    positive = []
    stem = net.backbone.stem
    stages = [stem[2], stem[5], stem[8]]
    stages += [blk for name in net.backbone.res_layers for blk in getattr(net.backbone, name)]
    stages += list(net.neck.fpn_convs)
    stages += [m for head in net.decode_head.scale_heads for m in head if isinstance(m, _ConvModule)]
    assert len(stages) == 30
    hooks = [m.register_forward_hook(lambda m, i, o: positive.extend(H.liveness([o.detach()]))) for m in stages]
    with torch.no_grad():                                          # EncoderDecoder.encode_decode
        low = net.decode_head.forward_test(net.neck(net.backbone(x)), None, None)
        full = _resize(low, size=x.shape[2:], mode="bilinear", align_corners=cfg["decode_head"]["align_corners"])
    for h in hooks:
        h.remove()
    assert full.dtype == torch.float64 and tuple(full.shape) == (1, 8, H.G15_H, H.G15_W)
    assert len(positive) == 30 and tuple(low.shape) == (1, 8, H.G15_H // 4, H.G15_W // 4)
    assert all(0.2 <= p <= 0.8 for p in positive), positive       # every stage is alive on both sides
    labels = full[0].numpy().argmax(0).astype(np.uint8)           # (softmax is monotone) inference.py / create_teeth_mask.py
    assert len(np.unique(labels)) >= 5, np.unique(labels)
    share = float((labels == T.TEETH).mean())
    assert 0.002 <= share <= 0.5, share

    res = dict(frame=frame[0].numpy(), logits4=low[0].numpy(), full=full[0].numpy(), labels=labels,
               positive=np.asarray(positive), layout=np.frombuffer(json.dumps(layout).encode(), dtype=np.uint8))
    path = f"{HERE}/g15_teeth.npz"
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes;", len(layout), "keys,", convs, "convolutions,", params, "parameters")
    print("positive fraction per stage", [round(p, 3) for p in positive], "labels", np.unique(labels).tolist(),
          "teeth share", round(share, 4), "max |logit|", float(low.abs().max()))
    with torch.no_grad():
        net = net.float()
        low32 = net.decode_head.forward_test(net.neck(net.backbone(x.float())), None, None)
        full32 = _resize(low32, size=x.shape[2:], mode="bilinear", align_corners=False).double()
    top = full.topk(2, dim=1).values
    print("fp32 torch vs fp64: relative to max |logit|", float((full32 - full).abs().max() / full.abs().max()),
          "labels differing", int((full32[0].numpy().argmax(0) != labels).sum()),
          "smallest top-two margin", float((top[:, 0] - top[:, 1]).min()))


if __name__ == "__main__":
    teeth()
