"""DeepSpeech operator (csrc/deepspeech.hip): the input rows of a one-minute clip (S = 3000) through DeepSpeechEncoder.logits
with seeded weights at the real dimensions, and the recurrence alone (instag_deepspeech_lstm on kept input projections),
beside the torch chain in fp32 on the same GPU in the same process: torch.nn.LSTM(bidirectional) with the weights
remapped plus linear layers (tests/deepspeech_helpers.torch_chain), and that LSTM alone.

    python scripts/bench_deepspeech.py [--json profiles/deepspeech_bench.json] [--seconds 60]

The figures are the median and the minimum of five windows after one warm-up pass of each path (the agreement check),
timed with device events, the two paths in alternating windows.  A step of the recurrence reads all of the recurrent
weights, 2 x 4 cell^2 floats (128 MiB): bytes per step over the step time is the rate at which the step kernel streams
them.  The weights take about 0.3 GB on the host and as much on the device: not for the test suite.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from _bench_audio import agreement, alternate, dump, seeded_wav, summary
from _bench_frames import operator_kernels
from instag_amd import deepspeech as D
from tests.deepspeech_helpers import torch_chain, torch_lstm

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--seconds", type=int, default=60)
    a = ap.parse_args()
    dev = torch.device("cuda")
    dims = D.DeepSpeechDims()
    weights = D.DeepSpeechWeights.random(dims, 0)
    rows = torch.from_numpy(D.input_vectors(D.to_int16(seeded_wav(a.seconds)))).to(dev)
    S = rows.shape[0]
    op = D.DeepSpeechEncoder(weights, dev)
    chain = torch_chain(weights, dev, torch.float32)
    lstm = torch_lstm(weights).to(device=dev, dtype=torch.float32)

    def hip():
        return op.logits(rows)

    def lib():
        return chain(rows)

    rel = agreement(hip(), lib())                             # (the warm-up)
    taps = []
    op.logits(rows, taps)
    h3, hseq = dict(taps)["h3"], dict(taps)["lstm"]
    kernels = weights.lstm_kernels(dev, torch.float32)
    xp = torch.stack([h3 @ wx + b for wx, _, b in kernels], dim=1).contiguous()
    weights._cache = {}
    del kernels, taps

    def hip_lstm():
        return op.recurrence(xp)

    def lib_lstm():
        with torch.no_grad():
            return lstm(h3[:, None])[0]

    rel_lstm = float((hip_lstm() - lib_lstm()[:, 0]).abs().max() / hseq.abs().max())
    assert rel_lstm < 1e-4, rel_lstm
    times = alternate({"hip": hip, "torch": lib, "hip_lstm": hip_lstm, "torch_lstm": lib_lstm})
    step_bytes = 2 * 4 * dims.cell * dims.cell * 4
    res = dict(seconds=a.seconds, steps=S, max_rows=op.rows_per_block(S), dims=dims.__dict__, device=torch.cuda.get_device_name(0),
               logits_hip_vs_torch_rel=rel, lstm_hip_vs_torch_rel=rel_lstm, recurrent_weight_bytes_per_step=step_bytes)
    summary(res, times)
    res["hip_step_us"] = 1e3 * res["hip_lstm_ms"] / S
    res["torch_step_us"] = 1e3 * res["torch_lstm_ms"] / S
    res["hip_step_gb_per_s"] = step_bytes / (res["hip_step_us"] * 1e-6) / 1e9
    res["hip_over_torch"] = res["hip_ms"] / res["torch_ms"]
    res["hip_lstm_over_torch_lstm"] = res["hip_lstm_ms"] / res["torch_lstm_ms"]
    res["hip_outside_the_recurrence_ms"] = res["hip_ms"] - res["hip_lstm_ms"]
    print(f"operator: {res['hip_ms']:.1f} ms for {S} steps ({a.seconds} s of audio; min {res['hip_min_ms']:.1f}); torch chain "
          f"{res['torch_ms']:.1f} ms (min {res['torch_min_ms']:.1f}); operator / torch chain {res['hip_over_torch']:.3f}"
          + ("  (SLOWER than torch's)" if res["hip_over_torch"] > 1.0 else "") + f"; the logits differ by {rel:.2e} of the largest",
          flush=True)
    print(f"recurrence alone: {res['hip_lstm_ms']:.1f} ms, {res['hip_step_us']:.1f} us a step, {res['hip_step_gb_per_s']:.0f} GB/s "
          f"of recurrent weights; torch.nn.LSTM {res['torch_lstm_ms']:.1f} ms, {res['torch_step_us']:.1f} us a step; ours / torch's "
          f"{res['hip_lstm_over_torch_lstm']:.3f}", flush=True)
    res["hip_kernels"] = operator_kernels(hip)
    dump(res, a.json, res["hip_kernels"])
