"""LPIPS patch term (csrc/lpips.hip): forward + backward time at 512x512 for the face (p = 64, 80, 96) and fuse
(p = 32, 42) patch sizes, per kernel, beside the same term through patch_lpips_torch (library convolutions) on the same
GPU; and the captured face step of the late phase with and without the term.

    python scripts/bench_lpips.py [--json out.json] [--no-step]

Every figure is the median of WINDOWS windows of ITERS calls, timed with events around the window; the two paths of one
patch size are measured in alternating windows of one process."""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instag_amd import lpips as LP

WINDOWS, ITERS = 7, 20
dev = torch.device("cuda")


def window(fn, iters=ITERS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def images(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 9, H), torch.linspace(0, 9, W), indexing="ij")
    base = torch.stack([0.5 + 0.35 * torch.sin(2 * yy + xx), 0.5 + 0.35 * torch.cos(yy - 2 * xx),
                        0.5 + 0.3 * torch.sin(3 * xx) * torch.cos(yy)])
    image = (base + 0.06 * torch.randn(3, H, W, generator=g)).clamp(0.01, 0.99)
    return image.to(dev), (image + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(dev)


def per_kernel(fn):
    """Mean device time per kernel name over a few calls (torch.profiler), or None where tracing is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        rows = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
            if t > 0:
                rows[e.key[:110]] = round(t / 5.0, 2)           # microseconds per call of fn
        return dict(sorted(rows.items(), key=lambda kv: -kv[1]))
    except Exception as exc:                                      # noqa: BLE001 (diagnostic leg only)
        return {"unavailable": repr(exc)}


def term(w, p, lo, hi, rect, results):
    image, gt = images(512, 512, seed=p)
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    r = None if rect is None else torch.tensor(rect, dtype=torch.int32, device=dev)
    op = LP.PatchLPIPS(w, 512, 512, lo, hi)
    x = image.clone().requires_grad_(True)

    def hip():
        v = op(x, gt, p, r, bg if r is not None else None)
        torch.autograd.grad(v, x)

    def hip_fwd():
        with torch.no_grad():
            op(x, gt, p, r, bg if r is not None else None)

    def lib():
        v = LP.patch_lpips_torch(x, gt, p, w, rect, bg if rect is not None else None)
        torch.autograd.grad(v, x)

    for f in (hip, hip_fwd, lib):
        window(f, 3)
    t = {"hip": [], "hip_fwd": [], "torch": []}
    for _ in range(WINDOWS):
        t["hip"].append(window(hip))
        t["torch"].append(window(lib))
        t["hip_fwd"].append(window(hip_fwd))
    n = (512 // p) ** 2
    rec = dict(patches=n, hip_fwd_bwd_ms=statistics.median(t["hip"]), hip_fwd_ms=statistics.median(t["hip_fwd"]),
               torch_fwd_bwd_ms=statistics.median(t["torch"]), hip_min_ms=min(t["hip"]), torch_min_ms=min(t["torch"]),
               kernels_us=per_kernel(hip))
    results[f"p{p}"] = rec
    print(f"p={p:3d} ({n:3d} patches): HIP fwd+bwd {rec['hip_fwd_bwd_ms']:.3f} ms (fwd {rec['hip_fwd_ms']:.3f}), "
          f"torch {rec['torch_fwd_bwd_ms']:.3f} ms", flush=True)
    for k, v in list(rec["kernels_us"].items())[:14]:
        print(f"      {v:>10} us  {k}", flush=True)


def face_step(w, results):
    from instag_amd import diff_gauss
    from instag_amd.scene_synth import synthetic_frame, synthetic_gaussians, toy_cameras
    from instag_amd.train import FaceTrainer, make_frame
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, PersonalizedMotionNetwork
    from types import SimpleNamespace
    cams = toy_cameras(512)
    frames = [make_frame(cams[i % len(cams)].to(dev), synthetic_frame(512, i, dev, priors=True)) for i in range(8)]
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    for name, weights in (("face_step_late_ms", None), ("face_step_late_lpips_ms", w)):
        torch.manual_seed(0)
        args = SimpleNamespace(audio_extractor="deepspeech", type="face")
        g = GaussianModel(1, neural_motion_grid=PersonalizedMotionNetwork(args=args).to(dev))
        g.load_raw(synthetic_gaussians(100000, sh_degree=1, seed=0), dev)
        tr = FaceTrainer(g, MotionNetwork(args=args).to(dev), bg, densify=False, schedule="reference", lpips=weights)
        tr.iteration = 7600
        tr.enable_graph(frames[0], keep_state=True)
        i = [0]

        def step():
            tr.step(frames[i[0] % 8])
            i[0] += 1
        window(step, 5)
        ts = [window(step) for _ in range(WINDOWS)]
        results[name] = statistics.median(ts)
        print(f"{name}: {results[name]:.3f} ms (min {min(ts):.3f}), recaptures {tr.recaptures}", flush=True)
        tr._drop_graph()
        diff_gauss.set_capacity_plan(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    w = LP.LPIPSWeights.random(0)
    results = {}
    for p in (64, 80, 96):
        term(w, p, 64, 96, (216, 293, 181, 326), results)
    for p in (32, 42):
        term(w, p, 32, 42, None, results)
    if not a.no_step:
        face_step(w, results)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
