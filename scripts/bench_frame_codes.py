"""Time the per-frame conditioning codes of an 'ave' and of a 'hubert' network: the HIP operators
(instag_frame_code_ave_*, instag_frame_code_wide_*) against the torch module chain of the same commit, the deepspeech
operator for scale, the mouth / fuse steps on 'ave' frames against the same steps on deepspeech frames, and the captured
face / mouth / fuse steps on 'hubert' frames with the operator and with audio.supported patched to False (the torch
modules answer: what a hubert head ran before the wide family existed).

    python scripts/bench_frame_codes.py [--out profiles/ave_frame_codes_bench.json] [--size 512] [--gaussians 100000]

One process, device events around windows of `--iters` calls, the median of `--windows` windows (and their spread).
The hubert operator rows alternate their windows between the HIP operator and the torch chain.
Needs the GPU: there is no CPU fallback."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, windows, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / iters)
    out.sort()
    return dict(median_us=out[len(out) // 2], min_us=out[0], max_us=out[-1], iters=iters, windows=windows)


def timed_alternating(fns, iters, windows, warmup=20):
    """timed() for several callables at once, a window of each in turn: drift of the clocks hits all alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            t1.synchronize()
            out[k].append(t0.elapsed_time(t1) * 1e3 / iters)
    res = {}
    for k, v in out.items():
        v.sort()
        res[k] = dict(median_us=v[len(v) // 2], min_us=v[0], max_us=v[-1], iters=iters, windows=windows)
    return res


def operator_times(iters, windows):
    from instag_amd import audio as A
    from instag_amd.motion_net import MotionNetwork

    class NoEncoder(torch.nn.Module):
        def __init__(self, **kw):
            super().__init__()
            self.output_dim = 12

    dev = torch.device("cuda")
    res = {}
    for extractor, shape in (("ave", (8, 1, 512)), ("deepspeech", (8, 29, 16)), ("hubert", (8, 1024, 2))):
        torch.manual_seed(0)
        net = MotionNetwork(args=SimpleNamespace(audio_extractor=extractor, type="face"), encoder_cls=NoEncoder).to(dev)
        a, e = torch.randn(*shape, device=dev), torch.rand(6, device=dev)
        wa = torch.randn(1, 32, device=dev)
        assert A.supported(net, a, e)
        params = [p for n, p in net.named_parameters() if n.startswith(("audio", "exp_encode"))]

        def forward(torch_branch):
            if torch_branch:
                return net.encode_audio(a), net.encode_exp(e)
            return net.encode_frame(a, e)

        def both(torch_branch):
            enc_a, enc_e = forward(torch_branch)
            torch.autograd.grad((enc_a * wa).sum() + enc_e.sum(), params)

        if extractor == "hubert":
            with torch.no_grad():
                pair = timed_alternating(dict(hip=lambda: forward(False), torch=lambda: forward(True)), iters, windows)
            res.update({f"hubert.{k}.forward": v for k, v in pair.items()})
            pair = timed_alternating(dict(hip=lambda: both(False), torch=lambda: both(True)), iters, windows)
            res.update({f"hubert.{k}.forward_backward": v for k, v in pair.items()})
            continue
        for name, tb in (("hip", False), ("torch", True)):
            with torch.no_grad():
                res[f"{extractor}.{name}.forward"] = timed(lambda: forward(tb), iters, windows)
            res[f"{extractor}.{name}.forward_backward"] = timed(lambda: both(tb), iters, windows)
    return res


def step_times(size, n, iters, windows):
    from instag_amd import diff_gauss
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    from instag_amd.train import make_frame
    from instag_amd.train_stages import FuseTrainer, MouthTrainer
    dev = torch.device("cuda")
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    cams = toy_cameras(size)
    res = {}
    for extractor in ("deepspeech", "ave"):
        frames = [make_frame(cams[i].to(dev), synthetic_frame(size, i, dev, background=True, audio_extractor=extractor))
                  for i in range(3)]
        for kind in ("mouth", "fuse"):
            torch.manual_seed(1)
            fa = SimpleNamespace(audio_extractor=extractor, type="face")
            ma = SimpleNamespace(audio_extractor=extractor, type="mouth")
            pc_face = GaussianModel(1, PersonalizedMotionNetwork(args=fa).to(dev)).create_random(n, dev, seed=1)
            pc_mouth = GaussianModel(1, PersonalizedMotionNetwork(args=ma).to(dev)).create_random(n // 5, dev, seed=2)
            face_net, mouth_net = MotionNetwork(args=fa).to(dev), MouthMotionNetwork(args=ma).to(dev)
            if kind == "mouth":
                tr = MouthTrainer(pc_mouth, mouth_net, pc_face, face_net, bg, densify=False, seed=3, warm_step=0)
            else:
                tr = FuseTrainer(pc_face, face_net, pc_mouth, mouth_net, bg)
            try:
                tr.enable_graph(frames[0])
                k = [0]

                def step():
                    tr.step(frames[k[0] % 3])
                    k[0] += 1
                res[f"{kind}_step.{extractor}"] = timed(step, iters, windows, warmup=10)
            finally:
                diff_gauss.set_capacity_plan(None)
            del tr
    return res


def hubert_step_times(size, n, iters, windows):
    """Captured face, mouth and fuse steps on 'hubert' frames: with the operator, then with audio.supported patched to
    False while the step is built and captured (the capture holds the torch modules' launches)."""
    from instag_amd import audio as A, diff_gauss
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork, PersonalizedMotionNetwork
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    from instag_amd.train import build_trainer, make_frame
    from instag_amd.train_stages import FuseTrainer, MouthTrainer
    dev = torch.device("cuda")
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    cams = toy_cameras(size)
    frames = [make_frame(cams[i].to(dev), synthetic_frame(size, i, dev, background=True, audio_extractor="hubert"))
              for i in range(3)]
    real = A.supported
    res = {}
    for kind in ("face", "mouth", "fuse"):
        for branch in ("hip", "torch"):
            A.supported = real if branch == "hip" else (lambda *a, **k: False)
            try:
                torch.manual_seed(1)
                if kind == "face":
                    tr = build_trainer(n, dev, seed=1, densify=False, audio_extractor="hubert")
                else:
                    fa = SimpleNamespace(audio_extractor="hubert", type="face")
                    ma = SimpleNamespace(audio_extractor="hubert", type="mouth")
                    pc_face = GaussianModel(1, PersonalizedMotionNetwork(args=fa).to(dev)).create_random(n, dev, seed=1)
                    pc_mouth = GaussianModel(1, PersonalizedMotionNetwork(args=ma).to(dev)).create_random(n // 5, dev, seed=2)
                    face_net, mouth_net = MotionNetwork(args=fa).to(dev), MouthMotionNetwork(args=ma).to(dev)
                    if kind == "mouth":
                        tr = MouthTrainer(pc_mouth, mouth_net, pc_face, face_net, bg, densify=False, seed=3, warm_step=0)
                    else:
                        tr = FuseTrainer(pc_face, face_net, pc_mouth, mouth_net, bg)
                tr.enable_graph(frames[0])
                k = [0]

                def step():
                    tr.step(frames[k[0] % 3])
                    k[0] += 1
                res[f"{kind}_step.hubert.{branch}"] = timed(step, iters, windows, warmup=10)
            finally:
                A.supported = real
                diff_gauss.set_capacity_plan(None)
            del tr
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ave_frame_codes_bench.json")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_codes.py measures on the GPU; none found")
    res = dict(device=torch.cuda.get_device_name(0), unit="microseconds per call (median of windows)")
    res.update(operator_times(args.iters, args.windows))
    if not args.no_steps:
        res.update(step_times(args.size, args.gaussians, max(20, args.iters // 4), args.windows))
        res.update(hubert_step_times(args.size, args.gaussians, max(20, args.iters // 4), args.windows))
    for extractor in ("ave", "hubert"):
        for k in ("forward", "forward_backward"):
            res[f"{extractor}.speedup.{k}"] = (res[f"{extractor}.torch.{k}"]["median_us"]
                                               / res[f"{extractor}.hip.{k}"]["median_us"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
