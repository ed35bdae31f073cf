"""Evaluation on the device (csrc/metrics.hip): `frame_metrics` at 512x512 for B = 1 and 4 beside the same figures through
`frame_metrics_torch` (library convolutions, on the same GPU), the inference epilogue with and without dilation, and
`Evaluator.evaluate` over ~100 synthetic frames (face 100k + mouth 20k Gaussians, four frames per replay) beside the
render alone and beside a render + `frame_metrics_torch` + read-back loop.

    python scripts/bench_metrics.py [--json out.json] [--no-evaluate]

Every figure is the median of WINDOWS windows of ITERS calls, timed with events around the window (evaluations: wall
clock around a synchronised call); the paths of one comparison are measured in alternating windows of one process."""
import argparse, json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instag_amd import metrics as M

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


def alternate(fns, iters=ITERS):
    for f in fns.values():
        window(f, 3)
    t = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, f in fns.items():
            t[k].append(window(f, iters))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v)) for k, v in t.items()}


def frame_metrics_bench(results):
    g = torch.Generator().manual_seed(0)
    for B in (1, 4):
        gt = torch.rand(B, 3, 512, 512, generator=g).to(dev)
        pred = (gt + 0.05 * torch.randn(B, 3, 512, 512, generator=g).to(dev))
        meter = M.Meter(dev)
        rec = alternate({
            "hip": lambda: M.frame_metrics(pred, gt, meter=meter),
            "hip_quantize": lambda: M.frame_metrics(pred, gt, quantize=True, meter=meter),
            "torch": lambda: M.frame_metrics_torch(pred, gt),
            "torch_quantize": lambda: M.frame_metrics_torch(pred, gt, quantize=True),
        })
        results[f"frame_metrics_512_B{B}"] = rec
        print(f"frame_metrics 512x512 B={B}: " + ", ".join(f"{k} {v['median_ms']:.4f} ms" for k, v in rec.items()),
              flush=True)


def compose_bench(results):
    g = torch.Generator().manual_seed(1)
    face, mouth, scene = (torch.rand(3, 512, 512, generator=g).to(dev) for _ in range(3))
    a_face, a_mouth = (torch.rand(1, 512, 512, generator=g).to(dev) for _ in range(2))
    bg = torch.zeros(3, device=dev)
    rec = alternate({
        "hip_dilate1_u8": lambda: M.infer_compose(face, a_face, mouth, a_mouth, bg, scene, 1, True),
        "hip_dilate13_u8": lambda: M.infer_compose(face, a_face, mouth, a_mouth, bg, scene, 13, True),
        "torch_dilate13_u8": lambda: M.infer_compose_torch(face, a_face, mouth, a_mouth, bg, scene, 13),
    })
    results["infer_compose_512"] = rec
    print("infer_compose 512x512: " + ", ".join(f"{k} {v['median_ms']:.4f} ms" for k, v in rec.items()), flush=True)


def evaluate_bench(results, n_frames=96, K=4):
    from types import SimpleNamespace
    from instag_amd import diff_gauss
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.infer import FuseRenderer
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    from instag_amd.scene_synth import synthetic_frame, synthetic_gaussians, toy_cameras
    from instag_amd.train import make_frame
    fa = SimpleNamespace(audio_extractor="deepspeech", type="face")
    ma = SimpleNamespace(audio_extractor="deepspeech", type="mouth")
    pc = GaussianModel(1, PersonalizedMotionNetwork(args=fa).to(dev)).load_raw(
        synthetic_gaussians(100000, sh_degree=1, seed=0), dev)
    pcm = GaussianModel(1, PersonalizedMotionNetwork(args=ma).to(dev)).load_raw(
        synthetic_gaussians(20000, sh_degree=1, seed=1), dev)
    net, netm = MotionNetwork(args=fa).to(dev), MouthMotionNetwork(args=ma).to(dev)
    cams = toy_cameras(512)
    base = [make_frame(cams[i % len(cams)].to(dev), synthetic_frame(512, i, dev, background=True)) for i in range(8)]
    frames = [base[i % 8] for i in range(n_frames)]
    gts = [f.original_image for f in frames]
    scenes = [f.talking_dict["background"] for f in frames]
    r = FuseRenderer(pc, net, pcm, netm, torch.zeros(3, device=dev))
    r.enable_graph(base[0], frames_per_replay=K)
    ev = M.Evaluator(r, quantize=True)

    def render_only():
        for g0 in range(0, n_frames, K):
            r.render_batch(frames[g0:g0 + K], scenes[g0:g0 + K])
        torch.cuda.synchronize()

    def evaluate():
        return ev.evaluate(frames, gts, scenes)

    def torch_loop():
        """The same renders, scored the way a user of the torch statement would: per group, read back per group."""
        acc = torch.zeros(5, dtype=torch.float64)
        for g0 in range(0, n_frames, K):
            images = r.render_batch(frames[g0:g0 + K], scenes[g0:g0 + K])
            acc += M.frame_metrics_torch(images, torch.stack(gts[g0:g0 + K]), quantize=True).double().sum(0).cpu()
        return acc / n_frames

    fns = {"render_only": render_only, "evaluate_hip": evaluate, "render_plus_torch_metrics": torch_loop}
    try:
        for f in fns.values():
            f()
        t = {k: [] for k in fns}
        for _ in range(WINDOWS):
            for k, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) * 1e3)
        rec = {k: dict(median_ms=statistics.median(v), min_ms=min(v), ms_per_frame=statistics.median(v) / n_frames)
               for k, v in t.items()}
        rec.update(frames=n_frames, frames_per_replay=K, report=evaluate(), overflow=bool(r.check_overflow()))
    finally:
        r.close()
        diff_gauss.set_capacity_plan(None)
    results["evaluate_512"] = rec
    print(f"evaluate, {n_frames} frames, {K} per replay: " +
          ", ".join(f"{k} {rec[k]['median_ms']:.2f} ms" for k in fns), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--no-evaluate", action="store_true")
    a = ap.parse_args()
    results = {}
    frame_metrics_bench(results)
    compose_bench(results)
    if not a.no_evaluate:
        evaluate_bench(results)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
