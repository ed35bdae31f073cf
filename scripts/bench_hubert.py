"""HuBERT encoder (csrc/hubert.hip): the three clips of a one-minute wav (1000, 1000 and 999 rows -> 2,999 rows) of the
full-size config with seeded weights through HubertEncoder.hidden, beside hubert_torch in fp32 on the same GPU, and
the attention kernel alone beside torch's scaled_dot_product_attention in fp32 on the same q, k, v.

    python scripts/bench_hubert.py [--json out.json] [--seconds 60]

Both paths take the same chunks: the clips of equal length as one batch, the others alone.  The figures are the median
and the minimum of five windows after one warm-up pass of each path (the agreement check), timed with device events,
the two paths in alternating windows of one process.  FLOPs are 2 x wav2vec.macs(head=False) per clip; the attention's
are 2 * 2 * T^2 * 64 * heads per segment, its windows are 20 calls each into a kept output and alternate too; the peak is the 157.3 TFLOP/s of the fp32 MFMA.  The input is seeded noise on a
modulated tone.  The weights take about 2.5 GB (host and device copy): not for the test suite.
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
from _bench_audio import agreement, alternate, dump, seeded_wav, summary
from _bench_frames import operator_kernels
from instag_amd import hubert as HU
from instag_amd import wav2vec as W

ESPERANTO_RATIO = 0.93          # the esperanto path's time over its torch chain's (profiles/esperanto_bench.json)
ATTENTION_REPEATS = 20

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--seconds", type=int, default=60)
    a = ap.parse_args()
    dev = torch.device("cuda")
    dims = W.Wav2Vec2Dims()
    weights = HU.HubertWeights.random(dims, 0)
    n = 16000 * a.seconds
    wav = seeded_wav(a.seconds)
    plan, rows = HU.clip_plan(n)
    values = HU.normalise_utterance(wav).to(dev)
    clips = [values[s:s + m] for s, m in plan]
    lengths = sorted({c.numel() for c in clips}, reverse=True)
    chunks = [torch.stack([c for c in clips if c.numel() == m]) for m in lengths]
    op = HU.HubertEncoder(weights, dev)
    assert op.max_batch >= max(c.shape[0] for c in chunks), (op.max_batch, [tuple(c.shape) for c in chunks])

    def hip():
        return [op.hidden(c) for c in chunks]

    def lib():
        with torch.no_grad():
            return [HU.hubert_torch(weights, c) for c in chunks]

    rel = agreement(hip(), lib())                             # (the warm-up)
    times = alternate({"hip": hip, "torch": lib})
    mac = sum(W.macs(dims, c.numel(), head=False) for c in clips)
    res = dict(seconds=a.seconds, clips=[W.frames_of(c.numel()) for c in clips], rows=rows, pairs=rows // 2,
               chunks=[list(c.shape) for c in chunks], max_batch=op.max_batch,
               gmac_per_full_clip=W.macs(dims, HU.CLIP_SAMPLES, head=False) / 1e9, gmac=mac / 1e9,
               hidden_hip_vs_torch_rel=rel, esperanto_hip_over_torch=ESPERANTO_RATIO)
    for k, text in summary(res, times, mac).items():
        print(f"{k:5s}: {res[f'{k}_ms']:.1f} ms for {len(clips)} clips of {a.seconds} s of audio "
              f"(min {res[f'{k}_min_ms']:.1f}), {text}", flush=True)
    res["hip_over_torch"] = res["hip_ms"] / res["torch_ms"]
    res["within_bar_1p05"] = res["hip_over_torch"] <= 1.05
    print(f"operator / torch chain: {res['hip_over_torch']:.3f} (bar 1.05; esperanto {ESPERANTO_RATIO}); the outputs differ by "
          f"{rel:.2e} of the largest entry", flush=True)

    # the attention kernel alone, at the shapes of the two chunks, beside torch's fused attention on the same q, k, v
    res["attention"] = []
    for B, T in [(c.shape[0], W.frames_of(c.shape[1])) for c in chunks]:
        gq = torch.Generator().manual_seed(2)
        qkv = torch.randn(B, T, 3 * dims.hidden, generator=gq)
        qkv[..., :2 * dims.hidden] *= 2.0 ** 0.5                  # scores with a standard deviation near 2
        qkv = qkv.to(dev)
        q, k, v = (x.reshape(B, T, dims.heads, 64).transpose(1, 2).contiguous() for x in qkv.chunk(3, dim=2))

        ctx = torch.empty(B, T, dims.hidden, device=dev)

        def ours():
            for _ in range(ATTENTION_REPEATS):
                HU.attention(qkv, dims.heads, out=ctx)

        def sdpa():
            for _ in range(ATTENTION_REPEATS):
                F.scaled_dot_product_attention(q, k, v)

        diff = float((HU.attention(qkv, dims.heads) - F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, -1))
                     .abs().max())
        ours(), sdpa()
        t_ours, t_sdpa = ([t / ATTENTION_REPEATS for t in ts] for ts in alternate({"hip": ours, "sdpa": sdpa}).values())
        flop = 2.0 * 2.0 * T * T * 64 * dims.heads * B
        entry = dict(batch=B, frames=T, heads=dims.heads, hip_us=1e3 * statistics.median(t_ours), hip_min_us=1e3 * min(t_ours),
                     sdpa_us=1e3 * statistics.median(t_sdpa), sdpa_min_us=1e3 * min(t_sdpa), max_abs_diff=diff)
        entry["hip_tflops"] = flop / (entry["hip_us"] * 1e-6) / 1e12
        entry["sdpa_tflops"] = flop / (entry["sdpa_us"] * 1e-6) / 1e12
        entry["hip_over_sdpa"] = entry["hip_us"] / entry["sdpa_us"]
        res["attention"].append(entry)
        print(f"attention B={B} T={T}: {entry['hip_us']:.1f} us per layer, {entry['hip_tflops']:.2f} TFLOP/s; torch sdpa fp32 "
              f"{entry['sdpa_us']:.1f} us, {entry['sdpa_tflops']:.2f} TFLOP/s; ours / sdpa {entry['hip_over_sdpa']:.2f}"
              + ("  (SLOWER than torch's)" if entry["hip_over_sdpa"] > 1.0 else ""), flush=True)
    res["hip_kernels_first_chunk"] = operator_kernels(lambda: op.hidden(chunks[0]))
    dump(res, a.json, res["hip_kernels_first_chunk"])
