"""Generate golden G20 (tests/golden/g20_face_detect.npz): S3FD in fp64 on one seeded 64 x 96 frame, by a second statement
of the network and of the tail behind it.

    python tests/golden/make_golden_face_detect.py                 # on the CPU

The face_alignment package is not a dependency and was not at hand: the ``nn.Module`` of tests/face_detect_helpers.py is
written in the layout of its net_s3fd.py (one ``nn.Conv2d`` per module name, an ``L2Norm`` module) and shares no code
with ``instag_amd.face_detect.s3fd_torch``; ``tail_loops`` and ``nms_loop`` there state the scores, the decode and the
suppression position by position in Python floats.  No test compares with a face_alignment run.

No weights are stored: ``S3FDWeights.random(20)`` is loaded strictly into the module under the package's keys.  Stored:
the u8 frame [64,96,3], the 12 fp64 maps (conf, loc per level; level 0's conf has its four raw channels), the
candidates (index, score, box) and the detections (index, score, box) of the second statement, and the state-dict
names and shapes.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def face_detect():
    sys.path.insert(0, ROOT)
    from tests import face_detect_helpers as H
    net = H.module()
    layout = sorted((k, list(v.shape)) for k, v in net.state_dict().items())
    convs = sum(1 for k, s in layout if len(s) == 4)
    assert convs == 31 and len(layout) == 65, (convs, len(layout))

    frame = H.seeded_frames(1, H.G20_H, H.G20_W, seed=H.SEED)[0].numpy()
    with torch.no_grad():
        maps = [m.numpy() for m in net(H.bgr_input(frame[None]))]
    assert all(m.dtype == np.float64 for m in maps)
    sides = [tuple(m.shape[2:]) for m in maps[::2]]
    assert sides == [(16, 24), (8, 12), (4, 6), (6, 7), (3, 4), (2, 2)], sides
    t = H.tail_loops(maps)
    assert 16 <= len(t["index"]) <= H.MAX_CANDIDATES and len(t["det_index"]) >= 2 and not t["overflow"]

    path = f"{HERE}/g20_face_detect.npz"
    np.savez_compressed(path, frame=frame, **{f"map{i}": m[0] for i, m in enumerate(maps)}, cand_index=t["index"],
                        cand_score=t["score"], cand_boxes=t["boxes"], det_index=t["det_index"], det_score=t["det_score"],
                        det_boxes=t["det_boxes"], layout=np.frombuffer(json.dumps(layout).encode(), dtype=np.uint8))
    print("wrote", path, os.path.getsize(path), "bytes;", len(layout), "keys,", convs, "convolutions")
    print("candidates", len(t["index"]), "detections", len(t["det_index"]), "largest entry per map",
          [round(float(np.abs(m).max()), 3) for m in maps])


if __name__ == "__main__":
    face_detect()
