"""Median ms per mouth pretraining step (instag_amd/pretrain.py PretrainMouthTrainer) in the warm phase, for K = 1 and
K = 5 identities of 20k mouth and 100k face Gaussians each at 512x512, with eager launches and with captured steps.  In
the same process, window by window in turn, the step with the pretraining operator switched off is timed too
(``fused_deform=False``: today's torch-composed personalised branch of render_motion_mouth_con plus torch loss terms), so
both figures see the same machine state.  A window is ``--steps`` consecutive steps between two synchronisations; the
figure is the median over ``--windows`` (>= 7) windows, with the windows' spread beside it.  Prints one JSON line and
writes it to ``--out``.

    python scripts/bench_pretrain_mouth.py [--n-mouth 20000] [--n-face 100000] [--size 512] [--steps 20] [--windows 7]
                                           [--out profiles/r07_pretrain_mouth_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


class CyclingPartner:
    """Every (identity, partner) pair in turn, so that graph mode has met all K (K - 1) keys after K (K - 1) steps of a
    round-robin identity sequence (the timing does not depend on which partner a step reads)."""

    def __init__(self, K):
        self.K, self.n = K, [0] * K

    def __call__(self, idx):
        if self.K < 2:
            return None
        self.n[idx] += 1
        return (idx + 1 + self.n[idx] % (self.K - 1)) % self.K


def window(tr, frames, K, steps, start):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(start, start + steps):
        tr.step(i % K, frames[i % len(frames)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def run(K, a, graph):
    from instag_amd.pretrain import build_mouth_pretrainer
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    from instag_amd.train import make_frame
    dev = torch.device("cuda")
    cams = toy_cameras(a.size)
    frames = [make_frame(cams[i].to(dev), synthetic_frame(a.size, i, dev)) for i in range(4)]
    trainers = {}
    for name, fused in (("fused", True), ("composed", False)):
        tr = build_mouth_pretrainer(K, a.n_mouth, a.n_face, dev, seed=0, densify=False, fused_deform=fused)
        tr.iteration = tr.sched.warm_step + 1          # warm phase: every term of the step
        tr.partner = CyclingPartner(K)
        if graph:
            tr.enable_graph()
        trainers[name] = tr
    pos = 0
    warm = max(5, K * max(1, K - 1) + K)               # (graph mode: every key captured before the timed windows)
    for tr in trainers.values():
        window(tr, frames, K, warm, 0)
    pos = warm
    times = {name: [] for name in trainers}
    for _ in range(a.windows):
        for name, tr in trainers.items():
            times[name].append(window(tr, frames, K, a.steps, pos))
        pos += a.steps
    out = {}
    for name, tr in trainers.items():
        assert torch.isfinite(tr.last["loss"])
        t = times[name]
        out[name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
        if graph:
            out[name]["captures"] = tr.captures
        tr.disable_graph()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-mouth", type=int, default=20000)
    ap.add_argument("--n-face", type=int, default=100000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_pretrain_mouth_bench.json"))
    a = ap.parse_args()
    assert a.windows >= 7, "medians of at least 7 windows"
    out = {"metric": "pretrain_mouth_step_ms", "mouth_gaussians": a.n_mouth, "face_gaussians": a.n_face, "size": a.size,
           "steps_per_window": a.steps, "windows": a.windows, "device": torch.cuda.get_device_name(0)}
    for K in (1, 5):
        for mode in ("eager", "captured"):
            out[f"K{K}_{mode}"] = run(K, a, mode == "captured")
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
