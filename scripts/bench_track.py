"""Time the landmark fit (instag_amd.track) on a synthetic identity: the kernels against the plain torch statement on
the same GPU, per stage and loop of the reference schedule.

    python scripts/bench_track.py [--frames 7000] [--candidates 20] [--torch-iters 0] [--out profiles/track_bench.json]

The identity is tests/track_helpers.py's seeded one (F frames, P candidates per contour slot, id_dim 100, exp_dim 79).
Every figure is a host clock around work that ends in a device synchronise, after a warm-up of each launch shape.
--torch-iters N > 0 times only N iterations of each loop of the torch statement and scales them to the schedule (the
statement's iteration cost does not depend on the iteration); 0 runs its whole schedule."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instag_amd import track  # noqa: E402
from tests import track_helpers as th  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stage(fit_pose, fit_joint, st, schedule, limit=0):
    """-> {"pose": seconds, "joint": seconds} of one stage on state ``st``; limit > 0: that many iterations per loop,
    scaled to the loop's length."""
    out = {}
    for loop, segments in (("pose", schedule[0]), ("joint", schedule[1])):
        if loop == "joint":
            st.fresh_idexp_optimizer()
        total = sum(n for n, _ in segments)
        if limit and limit < total:
            n, lr = limit, segments[0][1]
            sec = timed(lambda: fit_pose(st, n, lr) if loop == "pose" else fit_joint(st, n, lr, lr))
            out[loop] = sec * total / n
        else:
            out[loop] = timed(lambda: [fit_pose(st, n, lr) if loop == "pose" else fit_joint(st, n, lr, lr)
                                       for n, lr in segments])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=7000)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track needs a GPU: a timing taken elsewhere says nothing")
    m = th.model(7, a.candidates)
    lms = th.identity(m, a.frames, 7, 1000.0)["lms"]
    tracker = track.LandmarkTracker(m, "cuda")
    sides = {"hip": (tracker.fit_pose, tracker.fit_joint, 0),
             "torch": (lambda s, n, lr: track.fit_pose_torch(m, s, n, lr),
                       lambda s, n, x, y: track.fit_joint_torch(m, s, n, x, y), a.torch_iters)}
    result = dict(frames=a.frames, candidates=a.candidates, id_dim=m.id_dim, exp_dim=m.exp_dim,
                  focal_frames=len(lms[::40]), torch_iters_timed=a.torch_iters or "whole schedule",
                  device=torch.cuda.get_device_name(0), seconds={})
    for name, (fit_pose, fit_joint, limit) in sides.items():
        for stage_name, make, schedule in (
                ("focal", lambda: track._focal_state(m, lms, th.H, th.W, track.FOCALS, 40, "cuda", torch.float32),
                 track.focal_schedule()),
                ("coarse", lambda: tracker.init_state(lms, [1000.0], th.H, th.W), track.coarse_schedule())):
            warm = make()                                              # every launch shape once
            fit_pose(warm, 3, 0.1)
            fit_joint(warm, 3, 0.1, 0.1)
            result["seconds"][f"{name}.{stage_name}"] = stage(fit_pose, fit_joint, make(), schedule, limit)
            print(name, stage_name, result["seconds"][f"{name}.{stage_name}"], flush=True)
    sec = result["seconds"]
    result["total_seconds"] = {n: sum(sum(sec[f"{n}.{s}"].values()) for s in ("focal", "coarse")) for n in sides}
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
