"""Measure the mesh renderer's kernels and the photometric fits against the fp64 statement on the cases of
tests/test_photometric_gpu.py and write the figures (per quantity: |hip - fp64|, |fp32 CPU statement - fp64|, the bound,
whether the ulp floor set it) as JSON.

    python scripts/photometric_parity.py profiles/photometric_parity.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instag_amd import mesh_render as mr  # noqa: E402
from tests import photo_helpers as ph  # noqa: E402
from tests import test_photometric_gpu as T  # noqa: E402


def main(out):
    report, worst = {}, (0.0, "")
    for name in T.CASES:
        r = T.ref(name)
        rr = T.renderer_of(r)
        cov = int(r["covered"].sum())
        entry = dict(covered_pixels=cov, flip_risk=int((r["risk"] & r["covered"]).sum()), kinks=int((r["kink"] & r["covered"]).sum()),
                     left_out_share=float(((r["risk"] | r["kink"]) & r["covered"]).sum()) / cov)
        leaves = [t.cuda().requires_grad_(True) for t in r["inputs"]]
        col = rr.vertex_stage(*leaves)
        g = torch.autograd.grad(col, leaves, r["up_col"].cuda())
        entry["vertex"] = ph.parity(dict(colours=col.detach(), d_geo=g[0], d_tex=g[1], d_light=g[2]), r["vertex64"], r["vertex32"])
        entry["render"] = ph.parity(T.hip_render(r, rr)[0], r["render64"], r["render32"])
        s, c = (t.cuda().requires_grad_(True) for t in r["blend_in"])
        o = rr.blend(s, c, r["ids64"].to(torch.int32).cuda())
        g = T._grads(o, (r["up_raw"] * (~r["blend_kink"])[..., None]).cuda(), [s, c])
        entry["blend"] = ph.parity(dict(image=o.detach(), d_screen=g[0], d_colours=g[1]), r["blend64"], r["blend32"])
        report[name] = entry
    f = T.fits()
    p = f["p"]
    t = mr.PhotometricTracker(f["m"], "cuda")
    args = (p["lms"], p["images"], p["focal"], T.FIT["H"], T.FIT["W"], T.FIT["batch"])
    light = t.fit_light(f["start"], *args, T.FIT["light_iters"], **p["settings"])
    start = {k: v.float() for k, v in f["light64"].items()}
    w64, w32 = (mr.fit_frames_torch(f["m"], start, *args, T.FIT["fine_iters"], dtype=d, **p["settings"]) for d in (torch.float64, torch.float32))
    fine = t.fit_frames(start, *args, T.FIT["fine_iters"], **p["settings"])
    report["fits"] = dict(light=ph.parity(light, f["light64"], f["light32"]), fine=ph.parity(fine, w64, w32))
    for name, entry in report.items():
        for stage, rep in entry.items():
            if isinstance(rep, dict):
                for k, (err, e32, bound, floor) in rep.items():
                    if err / bound > worst[0]:
                        worst = (err / bound, f"{name} {stage} {k}")
    report["largest_error_over_bound"] = dict(ratio=worst[0], where=worst[1])
    print(json.dumps(report["largest_error_over_bound"]))
    with open(out, "w") as fp:
        json.dump(report, fp, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "profiles/photometric_parity.json")
