"""Preparing an identity: the background call and the frame stage, on the device and on the host.

    python scripts/bench_prepare.py [--size 512] [--samples 300] [--frames 6000] [--batch 256] [--host-samples 4]

A synthetic identity (a head ellipse, a neck bar, a torso block, jittered; 32 distinct frames, repeated) at ``--size``:
  background -- instag_prep_background over ``--samples`` samples, ms per call (median of ``--reps`` calls, wall clock
                around a call that ends synchronised);
  frames     -- instag_prep_frames over ``--frames`` frames in batches of ``--batch`` resident frames, frames/s
                (device events around the whole run, median of ``--reps`` runs);
  host       -- the plain statements (prepare.background_torch / frames_torch) on ``--host-samples`` samples / frames,
                and sklearn's kd-tree distances for the same samples when sklearn is importable: seconds per sample /
                per frame on this machine's CPU.
Checks the device results of the host's samples against the statement first.  Prints one JSON line.
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


def scene(F, H, W, seed=0):
    rng = np.random.default_rng(seed)
    ori = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    parsing = np.full((F, H, W, 3), 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(F):
        cy, cx = int(0.3 * H) + rng.integers(-H // 24, H // 24 + 1), W // 2 + rng.integers(-W // 10, W // 10 + 1)
        ry, rx = int(0.15 * H), int(0.12 * W)
        head = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        nw = rx // 2
        neck = (yy >= cy + ry - 2) & (yy < cy + ry + H // 12) & (np.abs(xx - cx) <= nw) & ~head
        top = cy + ry + H // 12
        torso = (yy >= top - (np.abs(xx - cx) <= nw + 3) * 2) & (np.abs(xx - cx) <= int(0.3 * W)) & ~head & ~neck
        parsing[f][head], parsing[f][neck], parsing[f][torso] = (0, 0, 255), (0, 255, 0), (255, 0, 0)
    return ori, parsing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--samples", type=int, default=300)
    ap.add_argument("--frames", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--host-samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prepare.py needs a GPU")
    from instag_amd import prepare as P
    dev = torch.device("cuda")
    H = W = args.size
    ori, par = scene(args.distinct, H, W)
    d_ori, d_par = torch.from_numpy(ori).to(dev), torch.from_numpy(par).to(dev)

    # ---- the host statements (and the device against them) ----
    n = args.host_samples
    t0 = time.perf_counter()
    h_bc, h_d2, h_arg = P.background_torch(ori[:n], par[:n])
    host_bg = (time.perf_counter() - t0) / n
    t0 = time.perf_counter()
    h_gt, h_torso = P.frames_torch(ori[:n], par[:n], h_bc)
    host_fr = (time.perf_counter() - t0) / n
    bc, d2, arg = P.background(d_ori[:n], d_par[:n], dev)
    gt, torso = P.gt_and_torso(d_ori[:n], d_par[:n], bc, device=dev)
    same = all(torch.equal(a.cpu(), b) for a, b in ((bc, h_bc), (d2, h_d2), (arg, h_arg), (gt, h_gt), (torso, h_torso)))
    kd = None
    try:
        from sklearn.neighbors import NearestNeighbors
        xy = np.mgrid[0:H, 0:W].reshape(2, -1).transpose()
        t0 = time.perf_counter()
        for s in range(n):
            fg = np.stack(np.nonzero(~(par[s] == 255).all(-1))).transpose()
            NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(fg).kneighbors(xy)
        kd = (time.perf_counter() - t0) / n
    except ImportError:
        pass

    # ---- the device ----
    idx = torch.arange(args.samples, device=dev) % args.distinct
    s_ori, s_par = d_ori[idx].contiguous(), d_par[idx].contiguous()
    bg_ms = []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bc = P.background(s_ori, s_par, dev)[0]
        bg_ms.append(1e3 * (time.perf_counter() - t0))
    del s_ori, s_par
    B = min(args.batch, args.frames)
    idx = torch.arange(B, device=dev) % args.distinct
    b_ori, b_par = d_ori[idx].contiguous(), d_par[idx].contiguous()
    gt = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    torso = torch.empty(B, H, W, 4, dtype=torch.uint8, device=dev)
    sizes = [B] * (args.frames // B) + ([args.frames % B] if args.frames % B else [])
    fps = []
    for _ in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in sizes:
            P.frames_into(b_ori[:k], b_par[:k], bc, gt[:k], torso[:k], batch=k)
        b.record()
        b.synchronize()
        fps.append(args.frames / (1e-3 * a.elapsed_time(b)))
    px = H * W
    res = dict(bench="prepare", size=args.size, samples=args.samples, frames=args.frames, batch=B,
               background_ms=round(statistics.median(bg_ms[1:]), 3), background_ms_runs=[round(t, 3) for t in bg_ms[1:]],
               frames_per_s=round(statistics.median(fps[1:]), 1), frames_per_s_runs=[round(f, 1) for f in fps[1:]],
               frames_gb_per_s=round(statistics.median(fps[1:]) * px * 13 / 1e9, 1),      # 3 + 3 read, 3 + 4 written
               host=dict(samples=n, background_s_per_sample=round(host_bg, 3), frames_s_per_frame=round(host_fr, 3),
                         kd_tree_s_per_sample=None if kd is None else round(kd, 3)),
               device_equals_statement=same)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
