"""Face detection (csrc/face_detect.hip): 256 seeded 512 x 512 frames through FaceDetector, beside the torch chain in fp32
on the same GPU in the same session.

    python scripts/bench_face_detect.py [--json profiles/face_detect_bench.json] [--frames 256] [--batch 7]

The operator is timed three ways: the network (``maps``), the tail alone (``post`` on maps that are ready: packing the 12
maps into six, the one tail launch per 64 frames) and both (``detect``).  The torch chain is ``s3fd_torch`` (library
convolutions, pools, the L2Norm as torch ops, in the same chunks) and ``post_torch(on_cpu=False)``: the scores, the
decode, the sort and the greedy loop as torch operations on the device, which reads a flag back every round.  All are
the median of WINDOWS windows of one pass over all frames after a warm-up pass of each (the agreement check), timed with
device events, in alternating windows of one process.  The seeded weights' conf heads are shifted and widened
(``conf_shift``, ``conf_gain``) until a frame has on the order of a hundred candidates, as trained weights leave; the
numbers are in the result.  FLOPs are 2 x ``macs_per_frame`` of the layer table; the peak is the 157.3 TFLOP/s of the
fp32 MFMA.  Per kernel: the operator's launches from a device trace of one chunk.
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import _bench_frames as BF
from instag_amd import face_detect as FD

WINDOWS = 5
SIZE = 512
CONF_SHIFT, CONF_GAIN = 5.0, 2.0

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=None)
    a = ap.parse_args()
    weights = FD.S3FDWeights.random(0, conf_shift=CONF_SHIFT, conf_gain=CONF_GAIN)
    frames = BF.seeded_frames(a.frames, SIZE).to(BF.dev)
    det = FD.FaceDetector(weights, BF.dev, max_batch=a.batch)
    batch = det.max_batch
    chunks = [slice(i, i + batch) for i in range(0, a.frames, batch)]

    @torch.no_grad()
    def lib_maps(c):
        return FD.s3fd_torch(weights, FD.normalise_torch(frames[c]))

    def hip_network():
        return det.maps(frames)

    def hip():
        return det.detect(frames)

    def lib_network():
        return [lib_maps(c) for c in chunks]

    def lib():
        return [FD.post_torch(lib_maps(c), SIZE, SIZE, on_cpu=False) for c in chunks]

    # faster and different is not faster: the paths agree on the timed inputs (this pass is also the warm-up)
    got, want = hip(), lib()
    count = torch.cat([w[1] for w in want])
    assert not bool(got[2].any()) and float((got[1] != count).double().mean()) < 0.05
    same = (got[1] == count).cpu()
    box_diff = float((torch.nan_to_num(got[0]) - torch.nan_to_num(torch.cat([w[0] for w in want])))[same.to(BF.dev)].abs().max())
    assert box_diff < 1e-2, box_diff
    maps = hip_network()
    first = lib_maps(chunks[0])
    rel = max(float((m[chunks[0]] - f).abs().max() / f.abs().max()) for m, f in zip(maps, first))
    assert rel < 1e-4, rel
    candidates = [int(c[0].shape[0]) for c in FD.candidates_torch([m[:16].cpu() for m in maps], SIZE, SIZE)]
    lib_first = [[m.clone() for m in first]]

    def hip_tail():
        return det.post(maps, SIZE, SIZE)

    def lib_tail():                                                             # one chunk of the torch tail, scaled below
        return FD.post_torch(lib_first[0], SIZE, SIZE, on_cpu=False)

    hip_tail(), lib_tail()
    t = {"hip": [], "hip_network": [], "hip_tail": [], "torch": [], "torch_network": [], "torch_tail_one_chunk": []}
    for _ in range(WINDOWS):
        t["hip"].append(BF.window(hip))
        t["torch"].append(BF.window(lib))
        t["hip_network"].append(BF.window(hip_network))
        t["torch_network"].append(BF.window(lib_network))
        t["hip_tail"].append(BF.window(hip_tail))
        t["torch_tail_one_chunk"].append(BF.window(lib_tail))
    macs = FD.macs_per_frame(SIZE, SIZE)
    flop = 2.0 * macs * a.frames
    res = dict(frames=a.frames, frame_size=SIZE, batch=batch, gmac_per_frame=macs / 1e9, windows=WINDOWS,
               conf_shift=CONF_SHIFT, conf_gain=CONF_GAIN, candidates_per_frame_first_16=candidates,
               detections_per_frame_mean=float(got[1].double().mean()), maps_hip_vs_torch_rel=rel,
               frames_with_another_count_hip_vs_torch=float((~same).double().mean()), boxes_hip_vs_torch_max_abs=box_diff,
               workspace_mib_per_frame=det._L.instag_face_detect_workspace_bytes(1, SIZE, SIZE) / 2 ** 20,
               teeth_fraction_of_fp32_mfma_peak_for_comparison=0.40)
    for k in t:
        ms = statistics.median(t[k])
        res[f"{k}_ms"], res[f"{k}_min_ms"], res[f"{k}_windows_ms"] = ms, min(t[k]), t[k]
        line = f"{k:22s}: {ms:.2f} ms (min {min(t[k]):.2f})"
        if not k.endswith(("tail", "one_chunk")):
            res[f"{k}_frames_per_s"] = a.frames / (ms * 1e-3)
            res[f"{k}_tflops"] = flop / (ms * 1e-3) / 1e12
            res[f"{k}_fraction_of_fp32_mfma_peak"] = res[f"{k}_tflops"] / BF.PEAK_TFLOPS
            line += (f" for {a.frames} frames, {res[f'{k}_frames_per_s']:.1f} frames/s, {res[f'{k}_tflops']:.2f} TFLOP/s, "
                     f"{100 * res[f'{k}_fraction_of_fp32_mfma_peak']:.1f} % of the fp32 MFMA peak")
        print(line, flush=True)
    res["hip_over_torch"] = res["hip_ms"] / res["torch_ms"]
    res["hip_network_over_torch_network"] = res["hip_network_ms"] / res["torch_network_ms"]
    res["hip_tail_us_per_frame"] = 1e3 * res["hip_tail_ms"] / a.frames
    res["torch_tail_us_per_frame"] = 1e3 * res["torch_tail_one_chunk_ms"] / batch
    res["hip_kernels_one_chunk"] = BF.operator_kernels(lambda: det.detect(frames[:batch]))
    for k, v in res["hip_kernels_one_chunk"].items():
        print(f"  {k:62s} {v}")
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
