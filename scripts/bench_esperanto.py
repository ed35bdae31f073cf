"""wav2vec 2.0 CTC network (csrc/wav2vec.hip): the 60 runs of a one-minute clip (2,999 rows -> 1,500 windows) of the
full-size config with seeded weights through Wav2Vec2CTC.logits, beside wav2vec2_torch in fp32 on the same GPU.

    python scripts/bench_esperanto.py [--json out.json] [--seconds 60] [--tiles]

Both paths take the same chunks: the full runs as one batch, the last run alone.  The figures are the median of five
windows after one warm-up pass of each path (the agreement check), timed with device events, the two paths in alternating
windows of one process.  FLOPs are 2 x wav2vec.macs per run; the peak is the 157.3 TFLOP/s of the fp32 MFMA.  The
weights take about 2.5 GB (host and device copy): not for the test suite.
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from _bench_audio import agreement, alternate, dump, seeded_wav, summary
from _bench_frames import WINDOWS, operator_kernels, window
from instag_amd import wav2vec as W

TEETH_FRACTION = 0.398          # of the peak: the teeth segmenter's convolution (profiles/teeth_bench.json)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--tiles", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    dims = W.Wav2Vec2Dims()
    weights = W.Wav2Vec2Weights.random(dims, 0)
    n = 16000 * a.seconds
    wav = seeded_wav(a.seconds).to(dev)
    plan = W.segment_plan(n)
    runs = [torch.cat([wav.new_zeros(z * W.CHUNK), wav[s * W.CHUNK: s * W.CHUNK + m - z * W.CHUNK]]) for s, z, m, _, _ in plan]
    full = torch.stack([r for r in runs if r.numel() == W.RUN_SAMPLES])
    rest = [r[None] for r in runs if r.numel() != W.RUN_SAMPLES]
    rows = sum(right - left for *_, left, right in plan)
    op = W.Wav2Vec2CTC(weights, dev)
    assert op.max_batch >= full.shape[0], (op.max_batch, full.shape)

    def hip():
        return [op.logits(full)] + [op.logits(r) for r in rest]

    def lib():
        with torch.no_grad():
            return [W.wav2vec2_torch(weights, full)] + [W.wav2vec2_torch(weights, r) for r in rest]

    got = hip()
    rel = agreement(got, lib())                               # (the warm-up)
    times = alternate({"hip": hip, "torch": lib})
    mac = sum(W.macs(dims, r.numel()) for r in runs)
    res = dict(seconds=a.seconds, runs=len(runs), rows=rows, windows=rows // 2 + 1, max_batch=op.max_batch,
               gmac_per_full_run=W.macs(dims) / 1e9, gmac=mac / 1e9, logits_hip_vs_torch_rel=rel,
               teeth_fraction_of_fp32_mfma_peak=TEETH_FRACTION)
    for k, text in summary(res, times, mac).items():
        print(f"{k:5s}: {res[f'{k}_ms']:.1f} ms for {len(runs)} runs of {a.seconds} s of audio (min {res[f'{k}_min_ms']:.1f}), "
              f"{W.macs(dims) / 1e9:.2f} GMAC per run, {text} (teeth convolution: {100 * TEETH_FRACTION:.1f} %)", flush=True)
    if a.tiles:                                               # every GEMM pinned to one tile: what the choice is worth
        for tile, name in ((1, "64x64"), (2, "64x128"), (3, "128x128")):
            op.tile = tile
            assert all(torch.equal(x, y) for x, y in zip(hip(), got)), tile
            res[f"hip_ms_tile_{name}"] = statistics.median(window(hip) for _ in range(WINDOWS))
            print(f"  every GEMM on {name}: {res[f'hip_ms_tile_{name}']:.1f} ms")
        op.tile = 0
    res["hip_kernels_full_batch"] = operator_kernels(lambda: op.logits(full))
    dump(res, a.json, res["hip_kernels_full_batch"])
