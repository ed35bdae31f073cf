"""The body of bench_parsing.py and bench_teeth.py: 256 seeded 512 x 512 frames through a frame operator, beside its
torch statement (library convolutions + batch norm, the same chunks) on the same GPU and the fp32 statement on the CPU.

The GPU figures are the median of WINDOWS windows of one pass over all frames, after one warm-up pass of each path (the
agreement check), timed with device events around the window; the two GPU paths are measured in alternating windows of
one process.  The CPU statement is timed on CPU_FRAMES frames with the wall clock.  FLOPs are 2 x the multiply-adds of
the convolutions (the module's macs_per_frame); the peak is the 157.3 TFLOP/s of the fp32 MFMA.  Per kernel: the
operator's launches from a device trace of one chunk."""
import argparse, json, re, statistics, time
import torch

WINDOWS = 5
CPU_FRAMES = 2
PEAK_TFLOPS = 157.3
dev = torch.device("cuda")


def seeded_frames(n, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, 32, 32, generator=g)
    img = torch.nn.functional.interpolate(low, (size, size), mode="bilinear", align_corners=False)
    img = 0.7 * img + 0.3 * torch.rand(n, 3, size, size, generator=g)
    return (img * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def operator_kernels(fn):
    """Device time of the operator's kernels in one call, summed by kernel name, in microseconds."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if "instag" not in e.name:
                continue
            m = re.search(r"(\w+_kernel(<[^>]*>)?)", e.name)
            name = m.group(1) if m else e.name[:60]
            t = float(getattr(e, "device_time", 0) or getattr(e, "cuda_time", 0))
            n, s = out.get(name, (0, 0.0))
            out[name] = (n + 1, s + t)
        return {k: {"launches": n, "us": round(s, 1)} for k, (n, s) in sorted(out.items(), key=lambda kv: -kv[1][1])}
    except Exception as exc:                                      # noqa: BLE001 (diagnostic leg only)
        return {"unavailable": repr(exc)}


def main(module, weights, make_operator, run, statement, extra=lambda got: {}):
    """``module``: instag_amd.parsing or .teeth; ``make_operator(weights, device, max_batch)``; ``run(operator,
    frames)`` and ``statement(weights, frames)`` give the two paths' outputs, u8 with one entry or one RGB triple per
    pixel; ``extra(operator's output)``: further entries of the result."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    host = seeded_frames(a.frames, module.SIZE)
    frames = host.to(dev)
    op = make_operator(weights, dev, max_batch=a.batch)

    def hip():
        return run(op, frames)

    def lib():
        return torch.cat([statement(weights, frames[i:i + a.batch]) for i in range(0, a.frames, a.batch)])

    def differing(x, y):
        d = x != y
        return float((d.any(dim=-1) if d.dim() == 4 else d).double().mean())

    # faster and different is not faster: the paths agree on the timed inputs (this pass is also the warm-up)
    got, want = hip(), lib()
    differ = differing(got, want)
    assert differ < 0.01, differ
    l_hip, l_lib = op.logits(frames[:a.batch]), op.net_torch(weights, module.normalise(frames[:a.batch]))
    rel = float((l_hip - l_lib).abs().max() / l_lib.abs().max())
    assert rel < 1e-4, rel
    t0 = time.perf_counter()
    cpu = statement(weights, host[:CPU_FRAMES])
    cpu_s = (time.perf_counter() - t0) / CPU_FRAMES
    cpu_differ = differing(got[:CPU_FRAMES].cpu(), cpu)

    t = {"hip": [], "torch": []}
    for _ in range(WINDOWS):
        t["hip"].append(window(hip))
        t["torch"].append(window(lib))
    flop = 2.0 * module.macs_per_frame() * a.frames
    res = dict(frames=a.frames, size=module.SIZE, batch=a.batch, gmac_per_frame=module.macs_per_frame() / 1e9,
               **extra(got), logits_hip_vs_torch_rel=rel, pixels_differing_hip_vs_torch=differ,
               pixels_differing_hip_vs_cpu=cpu_differ, cpu_fp32_frames_per_s=1.0 / cpu_s,
               cpu_threads=torch.get_num_threads())
    print(f"cpu  : {1.0 / cpu_s:.2f} frames/s (fp32 statement, {torch.get_num_threads()} threads, {CPU_FRAMES} frames)")
    for k in ("hip", "torch"):
        ms = statistics.median(t[k])
        res[f"{k}_ms"] = ms
        res[f"{k}_min_ms"] = min(t[k])
        res[f"{k}_frames_per_s"] = a.frames / (ms * 1e-3)
        res[f"{k}_tflops"] = flop / (ms * 1e-3) / 1e12
        res[f"{k}_fraction_of_fp32_mfma_peak"] = res[f"{k}_tflops"] / PEAK_TFLOPS
        print(f"{k:5s}: {ms:.1f} ms for {a.frames} frames (min {min(t[k]):.1f}), {res[f'{k}_frames_per_s']:.1f} frames/s, "
              f"{res[f'{k}_tflops']:.2f} TFLOP/s, {100 * res[f'{k}_fraction_of_fp32_mfma_peak']:.1f} % of the fp32 MFMA peak",
              flush=True)
    res["hip_kernels_one_chunk"] = operator_kernels(lambda: run(op, frames[:a.batch]))
    for k, v in res["hip_kernels_one_chunk"].items():
        print(f"  {k:62s} {v}")
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
