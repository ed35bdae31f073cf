"""Median ms per pretraining step (instag_amd/pretrain.py) in the warm phase, for K = 1 and K = 5 identities of 100k
Gaussians each at 512x512, with captured steps (graph mode) and with eager launches.  The K = 5 - K = 1 difference is
what the contrast term adds (four more PMF forwards without gradient and their heads in the deform operator).  Prints
one JSON line.  ``--k 5 --mode eager`` times one configuration alone (for a profiler run).

    python scripts/bench_pretrain.py [--n 100000] [--size 512] [--steps 30] [--warmup 5] [--k K] [--mode graph|eager]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def run(K, n, size, steps, warmup, graph):
    from instag_amd.pretrain import IdentitySampler, build_pretrainer
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    from instag_amd.train import make_frame
    dev = torch.device("cuda")
    cams = toy_cameras(size)
    frames = [make_frame(cams[i].to(dev), synthetic_frame(size, i, dev)) for i in range(4)]
    tr = build_pretrainer(K, n, dev, seed=0, densify=False)
    tr.iteration = tr.sched.warm_step + 1          # warm phase: every term of the step
    pick = IdentitySampler(K, seed=0)
    if graph:
        tr.enable_graph()
        # every (identity, hair / non-hair) step captured before the timed window
        warmup = max(warmup, 20 * K)
    times = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.step(pick(), frames[i % len(frames)])
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(tr.last["loss"])
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=0, help="one K only (with --mode)")
    ap.add_argument("--mode", choices=("graph", "eager"), default="graph")
    a = ap.parse_args()
    if a.k:
        ms = run(a.k, a.n, a.size, a.steps, a.warmup, a.mode == "graph")
        print(json.dumps({"metric": f"pretrain_step_ms_{a.mode}", "K": a.k, "ms": round(ms, 3)}))
        return
    out = {"metric": "pretrain_step_ms", "gaussians_per_identity": a.n, "size": a.size}
    for mode in ("graph", "eager"):
        k1 = run(1, a.n, a.size, a.steps, a.warmup, mode == "graph")
        k5 = run(5, a.n, a.size, a.steps, a.warmup, mode == "graph")
        out[mode] = {"K1_ms": round(k1, 3), "K5_ms": round(k5, 3), "K5_minus_K1_ms": round(k5 - k1, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
