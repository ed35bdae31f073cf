"""What bench_esperanto.py, bench_hubert.py, bench_deepspeech.py and bench_ave_encoder.py share: the seeded wav, the
warm-up pass that is the agreement check, the alternating windows, the per-path summary and the JSON dump.

The figures are the median and the minimum of the windows after one warm-up pass of each path, timed with device events,
the paths in alternating windows of one process.  The peak is the 157.3 TFLOP/s of the fp32 MFMA."""
import json, statistics
import torch
from _bench_frames import PEAK_TFLOPS, WINDOWS, window


def seeded_wav(seconds):
    """fp32 [16000 seconds] on the CPU: seeded noise on a modulated 220 Hz tone."""
    n = 16000 * seconds
    g = torch.Generator().manual_seed(1)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    return (0.3 * torch.sin(6.283185307179586 * 220.0 * t) * (1.0 + torch.sin(6.283185307179586 * 1.5 * t))
            + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float()


def agreement(got, want, bar=1e-4):
    """max|got - want| / max|want| over the tensors of the two warm-up passes, asserted below ``bar``: faster and
    different is not faster."""
    got, want = (list(v) if isinstance(v, (list, tuple)) else [v] for v in (got, want))
    rel = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(got, want))
    assert rel < bar, rel
    return rel


def alternate(paths, windows=WINDOWS, window=window):
    """name -> the times of ``windows`` windows of every path of ``paths`` (name -> function), taken in turn."""
    times = {k: [] for k in paths}
    for _ in range(windows):
        for k, fn in paths.items():
            times[k].append(window(fn))
    return times


def summary(res, times, macs=None, ms_key="{}_ms"):
    """Per path of ``times`` the median (under ``ms_key``) and the minimum into ``res``; with ``macs`` per window also
    the TFLOP/s (2 x macs) and the fraction of the peak -> name -> the text of these figures."""
    text = {}
    for k, v in times.items():
        ms = res[ms_key.format(k)] = statistics.median(v)
        res[f"{k}_min_ms"] = min(v)
        if macs is not None:
            res[f"{k}_tflops"] = 2.0 * macs / (ms * 1e-3) / 1e12
            res[f"{k}_fraction_of_fp32_mfma_peak"] = res[f"{k}_tflops"] / PEAK_TFLOPS
            text[k] = (f"{res[f'{k}_tflops']:.2f} TFLOP/s, {100 * res[f'{k}_fraction_of_fp32_mfma_peak']:.1f} % of the "
                       "fp32 MFMA peak")
    return text


def dump(res, path, kernels=None):
    """The ``kernels`` table (_bench_frames.operator_kernels) line by line, the result as one JSON line, and the file."""
    for k, v in (kernels or {}).items():
        print(f"  {k:62s} {v}")
    print(json.dumps(res), flush=True)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
