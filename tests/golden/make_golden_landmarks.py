"""Generate golden G19 (tests/golden/g19_landmarks.npz): FAN-2D-4 in eval mode and fp64 on one seeded 64 x 64 crop, by a
second statement of the network and of the arithmetic around it.

    python tests/golden/make_golden_landmarks.py                 # on the CPU

The face_alignment package is not a dependency and was not at hand: the ``nn.Module`` classes of
tests/landmarks_helpers.py are written in the layout of its models.py (the same module names, BatchNorm modules,
``torch.cat``) and share no code with ``instag_amd.landmarks.fan_torch``; ``crop_loops`` and ``decode_loops`` there
state the crop and the decode pixel by pixel and landmark by landmark.  No test compares with a face_alignment run.

No weights are stored: ``FANWeights.random(19)`` is loaded strictly into the module under the package's keys.  Stored:
the u8 frame [96,80,3], the box (it crosses the frame's edge), the u8 crop [64,64,3] of it, the last stack's fp64 heatmaps
[68,16,16] of that crop, the landmarks [68,2] decoded from them, every stack's largest entry, and the state-dict names
and shapes.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def landmarks():
    sys.path.insert(0, ROOT)
    from tests import landmarks_helpers as H
    net = H.module()
    ckpt = H.state_dict()
    layout = sorted((k, list(v.shape)) for k, v in ckpt.items())
    convs = sum(1 for k, s in layout if len(s) == 4)
    params = sum(int(np.prod(s)) for k, s in layout if s and not k.endswith(("running_mean", "running_var")))
    assert convs == 194, convs

    frame = H.seeded_frames(1, H.G19_H, H.G19_W, seed=H.SEED)[0].numpy()
    box = np.asarray(H.G19_BOX, dtype=np.float32)
    crop = H.crop_loops(frame, box, H.G19_S)
    assert 0.05 < float((crop == 0).all(axis=2).mean()) < 0.6                # part of the crop lies outside the frame
    x = torch.from_numpy(crop.astype(np.float64).transpose(2, 0, 1)[None] / 255.0)
    with torch.no_grad():
        stacks = net(x)
    heat = stacks[-1][0].numpy()
    assert heat.dtype == np.float64 and heat.shape == (68, 16, 16)
    lms = H.decode_loops(heat, box)
    assert len({tuple(p) for p in lms.tolist()}) >= 20                       # the maxima are spread over the map
    scales = np.asarray([float(s.abs().max()) for s in stacks])

    path = f"{HERE}/g19_landmarks.npz"
    np.savez_compressed(path, frame=frame, box=box, crop=crop, heatmaps=heat, landmarks=lms, scales=scales,
                        layout=np.frombuffer(json.dumps(layout).encode(), dtype=np.uint8))
    print("wrote", path, os.path.getsize(path), "bytes;", len(layout), "keys,", convs, "convolutions,", params, "parameters")
    print("largest entry per stack", scales.tolist(), "distinct landmarks", len({tuple(p) for p in lms.tolist()}))
    with torch.no_grad():
        got32 = H.module(dtype=torch.float32)(x.float())[-1][0].double().numpy()
    print("fp32 torch vs fp64, relative to the largest entry", float(np.abs(got32 - heat).max() / np.abs(heat).max()))


if __name__ == "__main__":
    landmarks()
