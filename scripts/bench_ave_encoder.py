"""AudioEncoder of the 'ave' extractor (csrc/ave_encoder.hip): the 1,500 windows of a one-minute clip at 25 fps through
AudioEncoder.encode, beside audio_encoder_torch (library convolutions + batch norm) on the same GPU in batches of 128,
the reference's DataLoader batch (scene/dataset_readers.py:130).

    python scripts/bench_ave_encoder.py [--json out.json]

Every figure is the median of WINDOWS windows of ITERS calls, timed with device events around the window; the two paths
are measured in alternating windows of one process.  FLOPs are 2 x the multiply-adds of the thirteen convolutions
(ave_encoder.MACS_PER_WINDOW per window); the peak is the 157.3 TFLOP/s of the fp32 MFMA.  Per layer: the operator's
twelve launches from a device trace (layers 11 and 12 are one launch), the torch chain block by block with events."""
import argparse, os, statistics, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bench_audio import agreement, alternate, dump, summary
from instag_amd import ave_encoder as AE

WINDOWS, ITERS = 7, 10
N_WINDOWS = 1500
TORCH_BATCH = 128
dev = torch.device("cuda")


def window(fn, iters=ITERS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def clip_mel():
    """A [T,80] mel with exactly N_WINDOWS windows."""
    T = 16 + (N_WINDOWS - 2) * 80 // 25
    while AE.window_starts(T).numel() < N_WINDOWS:
        T += 1
    assert AE.window_starts(T).numel() == N_WINDOWS
    g = torch.Generator().manual_seed(0)
    return (torch.rand(T, 80, generator=g) * 8 - 4).to(dev)


def operator_layers(fn, launches=12):
    """Mean device time of each of the operator's launches, in launch order, in microseconds per clip."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if "instag" in e.name and ("first_layer" in e.name or "conv_kernel" in e.name
                                                                    or "tail_kernel" in e.name)]
        ev.sort(key=lambda e: e.time_range.start)
        if not ev or len(ev) % launches:
            return {"unavailable": f"{len(ev)} kernel events"}
        names = ["layer 0"] + [f"layer {l}" for l in range(1, 11)] + ["layers 11+12"]
        out = {n: 0.0 for n in names}
        for i, e in enumerate(ev):
            out[names[i % launches]] += float(getattr(e, "device_time", 0) or getattr(e, "cuda_time", 0))
        return {k: round(v, 1) for k, v in out.items()}
    except Exception as exc:                                      # noqa: BLE001 (diagnostic leg only)
        return {"unavailable": repr(exc)}


def torch_layers(weights, windows):
    """The torch chain block by block on one batch of TORCH_BATCH windows: microseconds per clip (scaled by batches)."""
    lays = weights.to(dev, torch.float32)
    x = windows
    out = {}
    with torch.no_grad():
        for l, (lay, (_, _, _, stride, pad, residual)) in enumerate(zip(lays, AE.LAYERS)):
            def block(x=x, lay=lay, stride=stride, pad=pad, residual=residual):
                y = F.conv2d(x, lay["weight"], lay["bias"], stride=stride, padding=pad)
                y = F.batch_norm(y, lay["mean"], lay["var"], lay["gamma"], lay["beta"], training=False, eps=AE.BN_EPS)
                return F.relu(y + x if residual else y)
            window(block, 3)
            t = statistics.median(window(block) for _ in range(5))
            out[f"layer {l}"] = round(t * 1e3 * N_WINDOWS / TORCH_BATCH, 1)
            x = block()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    a = ap.parse_args()
    w = AE.AudioEncoderWeights.random(0)
    mel = clip_mel()
    enc = AE.AudioEncoder(w, dev)
    windows = AE.cut_windows(mel)

    def hip():
        return enc.encode(mel)

    def lib():
        with torch.no_grad():
            return torch.cat([AE.audio_encoder_torch(w, windows[i:i + TORCH_BATCH])
                              for i in range(0, N_WINDOWS, TORCH_BATCH)])

    rel = agreement(hip(), lib(), 1e-5)
    for f in (hip, lib):
        window(f, 3)
    t = alternate({"hip": hip, "torch": lib}, WINDOWS, window)
    res = dict(windows=N_WINDOWS, gflop_per_clip=2.0 * AE.MACS_PER_WINDOW * N_WINDOWS / 1e9, max_batch=enc.max_batch,
               hip_vs_torch_rel=rel)
    for k, text in summary(res, t, AE.MACS_PER_WINDOW * N_WINDOWS, "{}_ms_per_clip").items():
        print(f"{k:5s}: {res[f'{k}_ms_per_clip']:.3f} ms per clip (min {res[f'{k}_min_ms']:.3f}), {text}", flush=True)
    res["hip_layers_us"] = operator_layers(hip)
    res["torch_layers_us"] = torch_layers(w, windows[:TORCH_BATCH])
    print("per layer, us per clip (operator | torch chain):")
    for k in res["torch_layers_us"]:
        print(f"  {k:12s} {res['hip_layers_us'].get(k, '')!s:>10} | {res['torch_layers_us'][k]:>10}")
    for k, v in res["hip_layers_us"].items():
        if k not in res["torch_layers_us"]:
            print(f"  {k:12s} {v!s:>10} |")
    dump(res, a.json)


if __name__ == "__main__":
    main()
