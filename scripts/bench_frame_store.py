"""Feeding a captured face step: resident packed frames, HostFrameFeeder, the 8-bit frame store.

    python scripts/bench_frame_store.py [--gaussians 100000] [--size 512] [--steps 200] [--warmup 30] [--windows 5]

The same eight frames three ways, each way with its own trainer (same seed) and captured step:
  resident -- packed fp32 frames in HBM, one device copy into the step's static frame (the headline's way);
  host     -- the same frames in pinned host memory through HostFrameFeeder (upload one step ahead + the device copy);
  store    -- FrameStore.ref(i): one instag_frame_unpack launch in front of the replay.
The windows alternate between the three ways (each starts from the same snapshot); the figure of a way is the median
of its windows, the spread their range.  Then the feed alone: the unpack launch against the packed copy_from it
replaces, by device events over ``--feed-reps`` calls.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_store(dev, n, size, T=64):
    """scene_synth.synthetic_frame quantised to the 8-bit files of a processed identity."""
    from instag_amd.frame_store import FrameStore
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    rng = np.random.default_rng(0)
    raw = {k: [] for k in ("gt", "torso", "parsing", "teeth", "au_exp", "lips_rect")}
    for i in range(n):
        s = synthetic_frame(size, i)
        raw["gt"].append((s["gt_image"].permute(1, 2, 0) * 255).to(torch.uint8).numpy())
        par = np.full((size, size, 3), 255, dtype=np.uint8)
        par[s["face_mask"].numpy()] = (0, 0, 255)
        par[s["hair_mask"].numpy()] = (0, 0, 0)
        par[s["mouth_mask"].numpy()] = (100, 100, 100)
        raw["parsing"].append(par)
        raw["teeth"].append(np.zeros((size, size), dtype=np.uint8))
        raw["torso"].append(rng.integers(0, 256, (size, size, 4), dtype=np.uint8))
        raw["au_exp"].append(s["au_exp"])
        raw["lips_rect"].append(s["lips_rect"])
    stack = lambda v: torch.stack(v) if torch.is_tensor(v[0]) else np.stack(v)
    store = FrameStore(dev)
    store.append(stack(raw["gt"]), stack(raw["torso"]), rng.integers(0, 256, (size, size, 3), dtype=np.uint8),
                 stack(raw["parsing"]), stack(raw["teeth"]), toy_cameras(size, n), stack(raw["au_exp"]),
                 stack(raw["lips_rect"]), [(7 * i + 5) % T for i in range(n)])
    store.set_audio(torch.randn(T, 29, 16, generator=torch.Generator().manual_seed(1)))
    return store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--feed-reps", type=int, default=500)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_store.py needs a GPU")
    from instag_amd import diff_gauss
    from instag_amd.train import HostFrameFeeder, build_trainer
    dev = torch.device("cuda")
    store = synthetic_store(dev, args.frames, args.size)
    frames = [store.frame(i, background=False) for i in range(args.frames)]          # the resident fp32 form
    host = [HostFrameFeeder.to_host(f) for f in frames]
    refs = [store.ref(i, background=False) for i in range(args.frames)]
    n = args.frames

    ways = {}
    for name in ("resident", "host", "store"):
        tr = build_trainer(args.gaussians, dev, seed=0)
        graph = tr.enable_graph(frames[0])
        if name == "host":
            feeder = HostFrameFeeder(frames[0], dev)
            run = lambda k, tr=tr, feeder=feeder: feeder.run(tr.step, host, k)
        elif name == "resident":
            run = lambda k, tr=tr: [tr.step(frames[i % n]) for i in range(k)]
        else:
            run = lambda k, tr=tr: [tr.step(refs[i % n]) for i in range(k)]
        run(args.warmup)
        torch.cuda.synchronize()
        ways[name] = dict(trainer=tr, graph=graph, run=run, snap=tr.snapshot(), times=[])
    for _ in range(args.windows):                               # alternate: the ways share whatever else the host does
        for name, w in ways.items():
            w["trainer"].restore(w["snap"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w["run"](args.steps)
            torch.cuda.synchronize()
            w["times"].append(1e3 * (time.perf_counter() - t0) / args.steps)
    losses = {}
    for name, w in ways.items():
        if w["graph"].check_overflow():
            raise SystemExit(f"instance capacity exceeded in the {name} windows")
        losses[name] = float(w["trainer"].last["loss"])
    # same data, same seed, same number of steps from the same snapshot: the three ways end at the same loss
    same = losses["resident"] == losses["store"] == losses["host"]

    static = frames[0].clone_static()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.feed_reps):
                fn(i)
            b.record()
            b.synchronize()
            out.append(1e3 * a.elapsed_time(b) / args.feed_reps)
        return statistics.median(out)

    unpack_us = timed(lambda i=0: static.copy_from(refs[i % n]))
    copy_us = timed(lambda i=0: static.copy_from(frames[i % n]))
    for w in ways.values():
        w["trainer"]._drop_graph()
    diff_gauss.set_capacity_plan(None)

    px = args.size * args.size
    small = 45 * 4 + 8 * 29 * 16 * 4
    res = dict(bench="frame_store", gaussians=args.gaussians, size=args.size, steps=args.steps, windows=args.windows,
               step_ms={k: round(statistics.median(w["times"]), 4) for k, w in ways.items()},
               step_ms_windows={k: [round(t, 4) for t in w["times"]] for k, w in ways.items()},
               step_ms_spread={k: round(max(w["times"]) - min(w["times"]), 4) for k, w in ways.items()},
               feed_us=dict(unpack_launch=round(unpack_us, 2), packed_copy=round(copy_us, 2)),
               # face layout: image 12 B/px + three masks
               bytes_per_step=dict(resident=dict(device_read=int(frames[0]._buf.numel()), device_write=int(frames[0]._buf.numel())),
                                   host=dict(link=int(host[0]._buf.numel()), device_read=int(frames[0]._buf.numel()),
                                             device_write=2 * int(frames[0]._buf.numel())),
                                   store=dict(device_read=4 * px + small, device_write=15 * px + small)),
               store_bytes_per_frame=int(store.nbytes // len(store)), final_loss=losses, same_final_loss=same)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
