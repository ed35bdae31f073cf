"""Geometry priors (csrc/sapiens.hip): seeded 512 x 512 frames through GeometryNet at the backbone's real size
(sapiens_0.3b: 1024 channels, 24 layers, 16 heads, 3072 tokens), beside the torch statement in fp32 on the same GPU in the
same session.

    python scripts/bench_sapiens.py [--json profiles/sapiens_bench.json] [--frames 4] [--head 512,256,128,64:64,64]

The weights are seeded stand-ins.  The backbone's size is the release's; the head's widths are NOT known to this project
(instag_amd/sapiens.py reads them from a checkpoint's shapes) and come from ``--head deconv widths:conv widths``, whose
default, (512, 256, 128, 64) + (64, 64), is an assumption: a halving stack that ends at 64 channels at 1024 x 768.

Timed: the whole chain (``predict``: resize, patch rows, backbone, head, finish), the backbone alone (``features``), the
head alone (``head``, from features that are ready) and the attention alone at T = 3072, 16 heads, one frame.  The torch
side is ``sapiens_torch`` (its backbone ``vit_torch`` on ready patch rows, its head ``head_torch`` + ``finish_torch``) and
``torch.nn.functional.scaled_dot_product_attention``, all fp32.  Every figure is the median of WINDOWS windows of one
pass over all frames after a warm-up pass of each path (the agreement check), timed with device events, the two sides in
alternating windows of one process.  FLOPs are 2 x ``macs_per_frame`` of the layer table; the peak is the 157.3 TFLOP/s
of the fp32 MFMA.  No time is a pass condition.
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
import _bench_frames as BF
from instag_amd import sapiens as S

WINDOWS = 5

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--head", default="512,256,128,64:64,64")
    ap.add_argument("--kind", default="normal")
    a = ap.parse_args()
    deconv, conv = (tuple(int(c) for c in part.split(",") if c) for part in a.head.split(":"))
    weights = S.SapiensWeights.random(deconv=deconv, conv=conv, kind=a.kind, seed=0)
    host = BF.seeded_frames(a.frames, 512)
    frames = host.to(BF.dev)
    net = S.GeometryNet(weights, BF.dev, a.kind)
    H = W = 512
    T, heads = weights.grid[0] * weights.grid[1], weights.heads

    def each(fn, x):
        return torch.cat([fn(x[i:i + 1]) for i in range(x.shape[0])])

    with torch.no_grad():
        rows = S.patch_rows_torch(frames, weights.in_size)
        feats = net.features(frames)
        qkv = torch.randn(1, T, 3 * 64 * heads, device=BF.dev)
    q, k, v = (t.view(1, T, heads, 64).transpose(1, 2).contiguous() for t in qkv.chunk(3, dim=2))

    paths = {
        "hip": lambda: net.predict(frames),
        "torch": lambda: each(lambda x: S.sapiens_torch(weights, x, a.kind), frames),
        "hip_backbone": lambda: net.features(frames),
        "torch_backbone": lambda: each(lambda x: S.vit_torch(weights, x), rows),
        "hip_head": lambda: net.head(feats, H, W),
        "torch_head": lambda: each(lambda x: S.finish_torch(S.head_torch(weights, x), H, W), feats),
        "hip_attention": lambda: S.attention(qkv, heads),
        "torch_attention": lambda: F.scaled_dot_product_attention(q, k, v),
    }

    # faster and different is not faster: the paths agree on the timed inputs (this pass is also the warm-up)
    with torch.no_grad():
        first = {name: fn() for name, fn in paths.items()}
    rel = {}
    for name in ("", "_backbone", "_head"):
        want = first["torch" + name]
        rel[name] = float((first["hip" + name] - want).abs().max() / want.abs().max())
        assert rel[name] < 2e-3, (name, rel[name])
    ctx = first["torch_attention"].transpose(1, 2).reshape(1, T, 64 * heads)
    rel["_attention"] = float((first["hip_attention"] - ctx).abs().max() / ctx.abs().max())
    assert rel["_attention"] < 1e-4, rel
    del first

    t = {name: [] for name in paths}
    with torch.no_grad():
        for _ in range(WINDOWS):
            for name, fn in paths.items():
                t[name].append(BF.window(fn))
    macs = S.macs_per_frame(weights, H, W)
    backbone_macs = T * S.PATCH_K * weights.hidden + weights.layers * T * (
        4 * weights.hidden ** 2 + 2 * weights.hidden * weights.intermediate + 2 * T * weights.hidden)
    head_macs = macs - backbone_macs
    attention_macs = 2 * T * T * 64 * heads
    ws = S.GeometryNet.workspace_bytes(weights, 1)
    res = dict(frames=a.frames, frame_size=512, input=list(weights.in_size), tokens=T, kind=a.kind,
               head_deconv=list(deconv), head_conv=list(conv), head_widths_are_an_assumption=True, windows=WINDOWS,
               gmac_per_frame=macs / 1e9, gmac_backbone=backbone_macs / 1e9, gmac_head=head_macs / 1e9,
               workspace_mib_per_frame=ws / 2 ** 20, default_max_batch=net.max_batch,
               hip_vs_torch_rel={("chain" if not k else k[1:]): v for k, v in rel.items()})
    count = {"": (macs, a.frames), "_backbone": (backbone_macs, a.frames), "_head": (head_macs, a.frames),
             "_attention": (attention_macs, 1)}
    for name in paths:
        ms = statistics.median(t[name])
        m, n = count[name[name.index("_"):] if "_" in name else ""]
        res[f"{name}_ms"], res[f"{name}_min_ms"], res[f"{name}_windows_ms"] = ms, min(t[name]), t[name]
        res[f"{name}_ms_per_frame"] = ms / n
        res[f"{name}_tflops"] = 2.0 * m * n / (ms * 1e-3) / 1e12
        res[f"{name}_fraction_of_fp32_mfma_peak"] = res[f"{name}_tflops"] / BF.PEAK_TFLOPS
        print(f"{name:16s}: {ms / n:9.3f} ms per frame (min {min(t[name]) / n:.3f}), {res[f'{name}_tflops']:.2f} TFLOP/s, "
              f"{100 * res[f'{name}_fraction_of_fp32_mfma_peak']:.1f} % of the fp32 MFMA peak", flush=True)
    for name in ("", "_backbone", "_head", "_attention"):
        res[f"hip{name}_over_torch"] = res[f"hip{name}_ms"] / res[f"torch{name}_ms"]
        print(f"hip{name} / torch{name}: {res[f'hip{name}_over_torch']:.3f}")
    res["hip_kernels_one_frame"] = BF.operator_kernels(lambda: net.predict(frames[:1]))
    for k_, v_ in res["hip_kernels_one_frame"].items():
        print(f"  {k_:62s} {v_}")
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
