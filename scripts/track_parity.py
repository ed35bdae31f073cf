"""Measure the landmark-fit kernels against the fp64 statement on the shapes of tests/test_track_gpu.py and write the
figures (per quantity: |hip - fp64|, |fp32 CPU statement - fp64|, the bound) as JSON.

    python scripts/track_parity.py profiles/r04_track_parity.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instag_amd import track  # noqa: E402
from tests import test_track_gpu as T  # noqa: E402
from tests import track_helpers as th  # noqa: E402


def main(out):
    report = {}
    for (case, scale), name in zip(T.TRAJECTORIES, T.IDS):
        m, st64 = T._setup(case, scale=scale)
        tracker = track.LandmarkTracker(m, "cuda")
        st = st64.clone(device="cuda", dtype=torch.float32)
        entry = dict(frames=case[0], candidates=case[1], seed=case[4], perturbation=scale)
        near0 = th.near_tie_frames(m, st64)
        want, s32 = {}, {}
        for s, o in ((st64, want), (st64.clone(dtype=torch.float32), s32)):
            lan, g, frame, _ = track.loss_and_grads_torch(m, s)
            o.update(loss=lan.double(), g_id=g["id"].double(), g_exp=g["exp"].double(), g_pose=g["pose"].double())
        lan, g = tracker.loss_and_grads(st)
        entry["loss_and_grads"] = th.parity(dict(loss=lan, g_id=g["id"], g_exp=g["exp"], g_pose=g["pose"]), want, s32, ~near0)
        st64, st32, near = th.run_fp64_and_fp32(m, st64, [("pose", 40, 0.1)])
        tracker.fit_pose(st, 40, 0.1)
        entry["pose_40"] = th.parity(th.state_tensors(st), th.state_tensors(st64), th.state_tensors(st32), ~near)
        st64, st32, near2 = th.run_fp64_and_fp32(m, st64, [("fresh",), ("joint", 40, 0.1)])
        st.fresh_idexp_optimizer()
        tracker.fit_joint(st, 40, 0.1, 0.1)
        entry["joint_40"] = th.parity(th.state_tensors(st), th.state_tensors(st64), th.state_tensors(st32), ~(near | near2))
        entry["frames_left_out"] = [int(near0.sum()), int((near | near2).sum())]
        report[name] = entry
        print(name, json.dumps(entry), flush=True)
    with open(out, "w") as f:
        json.dump(dict(columns=["hip_vs_fp64", "fp32_statement_vs_fp64", "bound", "bound_set_by_ulp_floor"], cases=report), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
