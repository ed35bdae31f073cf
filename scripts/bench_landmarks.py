"""Face landmarks (csrc/landmarks.hip): 256 seeded 512 x 512 frames with one box each through LandmarkNet.landmarks,
beside the torch statement in fp32 on the same GPU in the same session.

    python scripts/bench_landmarks.py [--json profiles/landmarks_bench.json] [--frames 256] [--batch 32]

The operator's figure is the whole chain: crop kernel, network, decode kernel.  The torch chain is ``fan_torch`` (library
convolutions, batch norm, cat, pools, in the same chunks) and ``decode_torch`` on crops that are ready on the device: its
crop is integer work on the CPU (``crop_torch``) and is left out of its time, which favours it.  Both are the median of
WINDOWS windows of one pass over all frames after a warm-up pass of each (the agreement check), timed with device events,
in alternating windows of one process.  FLOPs are 2 x ``macs_per_face`` of the layer table; the peak is the 157.3 TFLOP/s
of the fp32 MFMA.  Per kernel: the operator's launches from a device trace of one chunk.
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import _bench_frames as BF
from instag_amd import landmarks as L

WINDOWS = 5

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    weights = L.FANWeights.random(0)
    host = BF.seeded_frames(a.frames, 512)
    g = torch.Generator().manual_seed(1)
    corner = torch.rand(a.frames, 2, generator=g) * 200 + 40                   # boxes of 180 .. 300 pixels inside the frame
    boxes = torch.cat([corner, corner + 180 + torch.rand(a.frames, 2, generator=g) * 120], dim=1)
    frames = host.to(BF.dev)
    net = L.LandmarkNet(weights, BF.dev, max_batch=a.batch)
    crops = net.crop(frames, boxes)

    def hip():
        return net.landmarks(frames, boxes)

    def hip_network():
        return torch.cat([net.heatmaps(crops[i:i + a.batch]) for i in range(0, a.frames, a.batch)])

    @torch.no_grad()
    def lib():
        return torch.cat([L.decode_torch(L.fan_torch(weights, L.normalise(crops[i:i + a.batch])), boxes[i:i + a.batch])
                          for i in range(0, a.frames, a.batch)])

    # faster and different is not faster: the paths agree on the timed inputs (this pass is also the warm-up)
    got, want = hip(), lib()
    differ = float((got != want).any(dim=2).double().mean())
    assert differ < 0.05, differ
    assert torch.equal(crops[:4].cpu(), L.crop_torch(host[:4], boxes[:4]))
    with torch.no_grad():
        h_hip, h_lib = net.heatmaps(crops[:a.batch]), L.fan_torch(weights, L.normalise(crops[:a.batch]))
    rel = float((h_hip - h_lib).abs().max() / h_lib.abs().max())
    assert rel < 1e-4, rel
    hip_network()

    t = {"hip": [], "hip_network": [], "torch": []}
    for _ in range(WINDOWS):
        t["hip"].append(BF.window(hip))
        t["torch"].append(BF.window(lib))
        t["hip_network"].append(BF.window(hip_network))
    macs = L.macs_per_face()
    flop = 2.0 * macs * a.frames
    res = dict(frames=a.frames, frame_size=512, crop_size=L.SIZE, batch=a.batch, gmac_per_face=macs / 1e9, windows=WINDOWS,
               heatmaps_hip_vs_torch_rel=rel, landmarks_differing_hip_vs_torch=differ,
               workspace_mib_per_face=net._L.instag_landmarks_workspace_bytes(1, L.SIZE) / 2 ** 20,
               teeth_fraction_of_fp32_mfma_peak_for_comparison=0.40)
    for k in t:
        ms = statistics.median(t[k])
        res[f"{k}_ms"], res[f"{k}_min_ms"], res[f"{k}_windows_ms"] = ms, min(t[k]), t[k]
        res[f"{k}_faces_per_s"] = a.frames / (ms * 1e-3)
        res[f"{k}_tflops"] = flop / (ms * 1e-3) / 1e12
        res[f"{k}_fraction_of_fp32_mfma_peak"] = res[f"{k}_tflops"] / BF.PEAK_TFLOPS
        print(f"{k:12s}: {ms:.1f} ms for {a.frames} faces (min {min(t[k]):.1f}), {res[f'{k}_faces_per_s']:.1f} faces/s, "
              f"{res[f'{k}_tflops']:.2f} TFLOP/s, {100 * res[f'{k}_fraction_of_fp32_mfma_peak']:.1f} % of the fp32 MFMA peak",
              flush=True)
    res["hip_over_torch"] = res["hip_ms"] / res["torch_ms"]
    res["hip_kernels_one_chunk"] = BF.operator_kernels(lambda: net.landmarks(frames[:a.batch], boxes[:a.batch]))
    for k, v in res["hip_kernels_one_chunk"].items():
        print(f"  {k:62s} {v}")
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
