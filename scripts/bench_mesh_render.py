"""Time the 3DMM mesh renderer (instag_amd.mesh_render) and one iteration of each photometric fit at the reference's sizes.

    python scripts/bench_mesh_render.py [--grid 186] [--size 512] [--batch 32] [--reps 20] [--out profiles/mesh_render_bench.json]

The mesh is tests/photo_helpers.py's seeded grid: 186 x 186 gives 34,596 vertices and 68,450 triangles (the reference's
model has 34,650 vertices), id_dim 100, exp_dim 79, tex_dim 100, rendered at size x size in batches of ``batch`` with the
reference's settings.  Every figure is the median of ``reps`` host-clock windows around work that ends in a device
synchronise, after a warm-up of each launch shape.  The plain statement is dense over the faces of every pixel and cannot
run at this size, so there is no torch column: the kernels are set against the bytes and the atomics they need."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instag_amd import mesh_render as mr  # noqa: E402
from instag_amd import track  # noqa: E402
from tests import photo_helpers as ph  # noqa: E402


def median_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=186)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit-iters", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_render needs a GPU: a timing taken elsewhere says nothing")
    H = W = a.size
    B = a.batch
    m = ph.model(a.grid, 7, False, 100, 79, 100)
    sc = ph.scene(m, B, 7, param_std=0.005)      # a smooth sheet: vertices move by a small fraction of a grid cell
    r = mr.MeshRenderer(m, ph.focal_for(H, W), H, W, "cuda")
    geo, tex, light = (sc[k].float().cuda() for k in ("rott_geo", "texture", "light"))
    screen = r.screen(geo)
    colours = r.vertex_stage(geo, tex, light)
    ids = r.select(screen)
    out = r.blend(screen, colours, ids)
    covered = int((ids[..., 0] >= 0).sum())
    both = int((ids[..., 1] >= 0).sum())
    up_img, up_col = torch.randn_like(out), torch.randn_like(colours)
    res = dict(device=torch.cuda.get_device_name(0), vertices=m.N, triangles=int(r.T), listed_per_vertex=int(r.M), batch=B, H=H, W=W,
               covered_pixels=covered, pixels_with_two_faces=both, reps=a.reps, ms={})

    def leaves(*ts):
        return [t.detach().clone().requires_grad_(True) for t in ts]

    def vertex_bwd():
        l = leaves(geo, tex, light)
        torch.autograd.grad(r.vertex_stage(*l), l, up_col)

    def blend_bwd():
        l = leaves(screen, colours)
        torch.autograd.grad(r.blend(*l, ids), l, up_img)

    def whole():
        l = leaves(geo, tex, light)
        torch.autograd.grad(r(*l), l, up_img)

    for name, fn in (("vertex_forward", lambda: r.vertex_stage(geo, tex, light)), ("vertex_forward_backward", vertex_bwd),
                     ("select", lambda: r.select(screen)), ("blend_forward", lambda: r.blend(screen, colours, ids)),
                     ("blend_forward_backward", blend_bwd), ("render_forward", lambda: r(geo, tex, light)),
                     ("render_forward_backward", whole)):
        res["ms"][name] = dict(zip(("median", "min", "max"), median_ms(fn, a.reps)))
        print(name, res["ms"][name], flush=True)
    # what the blend backward adds: 36 floats per face slot at the most (3 corners x (3 screen + 3 colour), two slots)
    ms = res["ms"]
    bwd = ms["blend_forward_backward"]["median"] - ms["blend_forward"]["median"]
    res["blend_backward_atomic_floats_upper_bound"] = 18 * (covered + both)
    res["blend_backward_atomic_GB_per_s"] = 4 * 18 * (covered + both) / (bwd * 1e-3) / 1e9
    # one iteration of each fit: the renderer against the torch remainder (landmarks, full-mesh GEMMs, losses, Adam)
    F = B
    p = dict(id=sc["id"].float(), exp=sc["exp"].float(), euler=sc["euler"].float(), trans=sc["trans"].float())
    focal = ph.focal_for(H, W)
    lands = track.landmarks_torch(m, sc["id"].expand(F, -1), sc["exp"], sc["euler"], sc["trans"], focal, W / 2.0, H / 2.0)
    lms = track.project_torch(lands, sc["euler"], sc["trans"], focal, W / 2.0, H / 2.0)[:, :, :2].float()
    images = torch.as_tensor(np.random.default_rng(7).integers(0, 256, (F, H, W, 3), dtype=np.uint8))
    t = mr.PhotometricTracker(m, "cuda")
    t.fit_light(p, lms, images, focal, H, W, B, 2)                       # warm-up of every shape
    full = dict(p, tex=torch.zeros(1, m.tex_dim), light=torch.zeros(F, 27))
    t.fit_frames(full, lms, images, focal, H, W, B, 2)
    for name, fn in (("light_fit_iteration", lambda: t.fit_light(p, lms, images, focal, H, W, B, a.fit_iters)),
                     ("fine_fit_iteration", lambda: t.fit_frames(full, lms, images, focal, H, W, B, a.fit_iters))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        once = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        {"light_fit_iteration": lambda: t.fit_light(p, lms, images, focal, H, W, B, 2 * a.fit_iters),
         "fine_fit_iteration": lambda: t.fit_frames(full, lms, images, focal, H, W, B, 2 * a.fit_iters)}[name]()
        torch.cuda.synchronize()
        twice = time.perf_counter() - t0
        res["ms"][name] = (twice - once) / a.fit_iters * 1e3             # (the set-up -- image upload, texture -- cancels)
        print(name, res["ms"][name], flush=True)
    res["renderer_share_of_light_iteration"] = ms["render_forward_backward"]["median"] / ms["light_fit_iteration"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
