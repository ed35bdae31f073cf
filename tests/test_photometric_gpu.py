"""GPU: the mesh renderer's kernels (csrc/mesh_render.hip) and the photometric fits against the fp64 plain statement.

Bounds: the rule of tests/track_helpers.parity.  |HIP - fp64 statement| <= 4 x |fp32 CPU statement - fp64 statement| on
the same fp32 inputs, never below 4 fp32 ulp of the quantity's largest magnitude; no tolerance is fixed in advance.
Measured on an MI355X: profiles/photometric_parity.json, DESIGN section 21.

Left out of the image and gradient comparisons are the flip-risk pixels of the fp64 statement (photo_helpers.flip_risk:
some outside face within 1e-3 relative of the blur radius, or the second and third candidate depth within 1e-5 of each
other), and of the gradient comparisons also the kinks (photo_helpers.gradient_kinks).  At most 5 % of the covered pixels
may be left out; exact ties are no risk and stay in.

The small images run with sigma scaled by (512 / min(H, W))^2, which gives the workload's regime of several candidate
faces per pixel (at the reference's sigma the blur radius would be 0.17 pixel here); one case runs at the reference's own
settings."""
import os

import numpy as np
import pytest
import torch

from instag_amd import mesh_render as mr
from instag_amd import track
from tests import photo_helpers as ph

pytestmark = pytest.mark.gpu

# name: (grid n, H, W, B, second sheet, euler std, sideways shift, seed, spoiled, sigma scaled)
CASES = {
    "9x9-48x56-B2": (9, 48, 56, 2, False, 0.15, 0.0, 31, False, True),
    "33x33-40x40-B1-subpixel": (33, 40, 40, 1, False, 0.15, 0.0, 32, False, True),
    "5x5-64x72-B3-offscreen": (5, 64, 72, 3, False, 0.15, 0.9, 33, False, True),
    "17x17-sheet-64x64-B2": (17, 64, 64, 2, True, 0.15, 0.0, 34, False, True),
    "17x17-rotated-64x64-B2": (17, 64, 64, 2, False, 0.6, 0.0, 35, False, True),
    "9x9-zero-area-and-behind-48x56-B2": (9, 48, 56, 2, True, 0.15, 0.0, 31, True, True),
    "17x17-256x256-B1-reference-settings": (17, 256, 256, 1, False, 0.15, 0.0, 36, False, False),
}
_REF = {}


def _grads(out, upstream, leaves):
    return torch.autograd.grad((out * upstream).sum(), leaves)


def ref(name):
    """Everything the CPU statements say about a case, computed once: fp64 and fp32 on the same fp32 inputs."""
    if name in _REF:
        return _REF[name]
    n, H, W, B, sheet, euler_std, shift, seed, spoiled, scaled = CASES[name]
    m = ph.model(n, seed, sheet)
    sc = ph.scene(m, B, seed, euler_std, shift)
    if spoiled:                                            # one zero-area face; the second sheet wholly behind the camera
        sc = ph.spoil(sc, m)
        sc["rott_geo"][:, n * n:, 2] += 9.0
    tris, vert_tris = m.topology_tensors("cpu")
    focal = ph.focal_for(H, W)
    sigma = ph.scaled_sigma(H, W) if scaled else mr.SIGMA
    blur = mr.blur_radius_of(sigma)
    inputs = [sc[k].float() for k in ("rott_geo", "texture", "light")]
    gen = torch.Generator().manual_seed(seed)
    up_col = torch.randn(B, m.N, 3, generator=gen, dtype=torch.float64).float()
    up_img = torch.randn(B, H, W, 4, generator=gen, dtype=torch.float64).float()
    r = dict(m=m, H=H, W=W, B=B, focal=focal, sigma=sigma, blur=blur, inputs=inputs, up_col=up_col, tris=tris, vert_tris=vert_tris)
    # the fp64 statement decides what is left out
    geo64 = inputs[0].double()
    screen64 = mr.screen_torch(geo64, focal, H, W)
    ids64 = mr.select_torch(screen64, tris, H, W, blur)
    col64 = mr.vertex_stage_torch(geo64, inputs[1].double(), inputs[2].double(), tris, vert_tris)
    _, terms = mr.blend_torch(screen64, col64, tris, ids64, H, W, sigma=sigma, return_terms=True)
    risk = ph.flip_risk(screen64, tris, H, W, blur)
    kink = ph.gradient_kinks(terms, ids64)
    covered = ids64[..., 0] >= 0
    r.update(ids64=ids64, risk=risk, kink=kink, covered=covered, screen64=screen64)
    r["up_raw"], r["up_img"] = up_img, up_img * (~(risk | kink))[..., None]
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        leaves = [t.to(dtype).requires_grad_(True) for t in inputs]
        col = mr.vertex_stage_torch(*leaves, tris, vert_tris)
        g = torch.autograd.grad(col, leaves, up_col.to(dtype))
        r["vertex" + tag] = dict(colours=col.detach(), d_geo=g[0], d_tex=g[1], d_light=g[2])
        out = mr.render_torch(*leaves, tris, vert_tris, focal, H, W, sigma=sigma)
        g = _grads(out, r["up_img"].to(dtype), leaves)
        r["render" + tag] = dict(image=out.detach() * (~risk)[..., None], d_geo=g[0], d_tex=g[1], d_light=g[2])
        # the blend alone, on the fp32 screen / colours the kernels get and the fp64 statement's ids
        screen_in = mr.screen_torch(inputs[0], focal, H, W)
        col_in = r["vertex64"]["colours"].float()
        s, c = screen_in.to(dtype).requires_grad_(True), col_in.to(dtype).requires_grad_(True)
        out, terms = mr.blend_torch(s, c, tris, ids64, H, W, sigma=sigma, return_terms=True)
        if tag == "64":
            r["blend_kink"] = ph.gradient_kinks(terms, ids64)
            r["blend_in"] = (screen_in, col_in)
        g = _grads(out, up_img.to(dtype) * (~r["blend_kink"])[..., None], [s, c])
        r["blend" + tag] = dict(image=out.detach(), d_screen=g[0], d_colours=g[1])
    _REF[name] = r
    return r


def renderer_of(r):
    return mr.MeshRenderer(r["m"], r["focal"], r["H"], r["W"], "cuda", sigma=r["sigma"])


def hip_render(r, rr=None):
    rr = rr or renderer_of(r)
    leaves = [t.cuda().requires_grad_(True) for t in r["inputs"]]
    out, ids = rr(*leaves, return_ids=True)
    g = _grads(out, r["up_img"].cuda(), leaves)
    return dict(image=out.detach().cpu() * (~r["risk"])[..., None], d_geo=g[0], d_tex=g[1], d_light=g[2]), ids, out.detach()


def left_out(r):
    out, cov = int(((r["risk"] | r["kink"]) & r["covered"]).sum()), int(r["covered"].sum())
    print(f"left out: {out} of {cov} covered pixels ({100.0 * out / cov:.2f} %), flip risk {int((r['risk'] & r['covered']).sum())}, "
          f"kinks {int((r['kink'] & r['covered']).sum())}")
    assert cov > 0 and out <= 0.05 * cov
    return out / cov


@pytest.mark.parametrize("name", CASES)
def test_vertex_stage_forward_and_backward(name):
    r = ref(name)
    rr = renderer_of(r)
    leaves = [t.cuda().requires_grad_(True) for t in r["inputs"]]
    col = rr.vertex_stage(*leaves)
    g = torch.autograd.grad(col, leaves, r["up_col"].cuda())
    got = dict(colours=col.detach(), d_geo=g[0], d_tex=g[1], d_light=g[2])
    ph.assert_parity(ph.parity(got, r["vertex64"], r["vertex32"]), f"vertex[{name}]")


@pytest.mark.parametrize("name", CASES)
def test_selection_takes_candidates_of_the_statement(name):
    r = ref(name)
    rr = renderer_of(r)
    H, W, T = r["H"], r["W"], r["tris"].shape[0]
    ids = rr.select(rr.screen(r["inputs"][0].cuda())).cpu().long()
    assert ids.dtype == torch.int64 and int(ids.min()) >= -1 and int(ids.max()) < T
    assert not ((ids[..., 0] < 0) & (ids[..., 1] >= 0)).any()                 # slot 0 fills first
    assert not ((ids[..., 0] >= 0) & (ids[..., 0] == ids[..., 1])).any()
    for r0 in range(0, H, 16):
        rows = (r0, min(H, r0 + 16))
        wide = mr.candidates_dense_torch(r["screen64"], r["tris"], H, W, r["blur"] * (1 + 1e-3), rows)
        t = mr.candidates_dense_torch(r["screen64"], r["tris"], H, W, r["blur"], rows)
        pz = torch.where(t["cand"], t["pz"], torch.full_like(t["pz"], float("inf"))).sort(dim=-1).values
        second = pz[..., 1] if T > 1 else pz[..., 0]
        part = ids[:, rows[0]:rows[1]]
        filled = part >= 0
        chosen_ok = torch.gather(wide["cand"], -1, part.clamp(min=0))
        chosen_pz = torch.gather(t["pz"], -1, part.clamp(min=0))
        assert bool((chosen_ok | ~filled).all()), "a chosen face is no candidate of the fp64 statement"
        assert bool(((chosen_pz <= second[..., None] + 1e-5) | ~filled).all()), "a chosen face lies behind the statement's second"
    keep = ~r["risk"]
    assert torch.equal((ids >= 0).sum(dim=-1)[keep], (r["ids64"] >= 0).sum(dim=-1)[keep])
    same = (ids.sort(dim=-1).values == r["ids64"].sort(dim=-1).values).all(dim=-1)
    print(f"select[{name}]: {int((~same & keep).sum())} kept pixels name another face than the fp64 statement (exact ties)")


@pytest.mark.parametrize("name", CASES)
def test_full_render_forward_and_gradients(name):
    r = ref(name)
    left_out(r)
    got, _, _ = hip_render(r)
    ph.assert_parity(ph.parity(got, r["render64"], r["render32"]), f"render[{name}]")


@pytest.mark.parametrize("name", CASES)
def test_blend_alone_with_the_statements_ids(name):
    r = ref(name)
    rr = renderer_of(r)
    s, c = (t.cuda().requires_grad_(True) for t in r["blend_in"])
    out = rr.blend(s, c, r["ids64"].to(torch.int32).cuda())
    cov = int(r["covered"].sum())
    assert int((r["blend_kink"] & r["covered"]).sum()) <= 0.05 * cov
    up = r["up_raw"] * (~r["blend_kink"])[..., None]
    g = _grads(out, up.cuda(), [s, c])
    got = dict(image=out.detach(), d_screen=g[0], d_colours=g[1])
    ph.assert_parity(ph.parity(got, r["blend64"], r["blend32"]), f"blend[{name}]")


@pytest.mark.parametrize("name", ["9x9-48x56-B2", "17x17-sheet-64x64-B2"])
def test_repeatability(name):
    """Forward runs are bit-identical.  The backward adds into the vertex arrays with float atomicAdd (blend backward: a
    vertex collects from every pixel its faces cover; vertex backward: from the vertices that list its triangles), whose
    order differs from run to run, so two backward runs agree within the parity bound, not bit for bit; d_light alone is
    reduced in a fixed order, but it is reduced from d_colours, which the atomics produced."""
    r = ref(name)
    rr = renderer_of(r)
    a, ids_a, out_a = hip_render(r, rr)
    b, ids_b, out_b = hip_render(r, rr)
    assert torch.equal(out_a, out_b) and torch.equal(ids_a, ids_b)
    report = ph.parity(a, r["render64"], r["render32"])
    for k in ("d_geo", "d_tex", "d_light"):
        diff = float((a[k] - b[k]).abs().max())
        print(f"repeat[{name}] {k}: |run 1 - run 2| = {diff:.3e}, bound {report[k][2]:.3e}")
        assert diff <= report[k][2]
    # with a fixed d_colours the vertex backward's texture and light gradients are bit-repeatable
    leaves = [t.cuda().requires_grad_(True) for t in r["inputs"]]
    runs = [torch.autograd.grad(rr.vertex_stage(*leaves), leaves, r["up_col"].cuda()) for _ in range(2)]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_renderer_under_autograd_equals_the_explicit_calls_and_batches_do_not_mix():
    name = "5x5-64x72-B3-offscreen"
    r = ref(name)
    rr = renderer_of(r)
    got, ids, out = hip_render(r, rr)
    leaves = [t.cuda().requires_grad_(True) for t in r["inputs"]]
    colours = rr.vertex_stage(*leaves)
    screen = rr.screen(leaves[0])
    ids2 = rr.select(screen)
    out2 = rr.blend(screen, colours, ids2)
    assert torch.equal(out2, out) and torch.equal(ids2, ids) and ids.dtype == torch.int32
    d_screen, d_colours = torch.autograd.grad(out2, [screen, colours], r["up_img"].cuda(), retain_graph=True)
    g_vertex = torch.autograd.grad(colours, leaves, d_colours, retain_graph=True)
    g_screen = torch.autograd.grad(screen, leaves[0], d_screen)[0]
    explicit = dict(d_geo=g_vertex[0] + g_screen, d_tex=g_vertex[1], d_light=g_vertex[2])
    report = ph.parity(got, r["render64"], r["render32"])
    for k, v in explicit.items():                                              # (float atomics: within the bound, not bitwise)
        assert float((v.cpu() - got[k].cpu()).abs().max()) <= report[k][2], k
    for b in range(r["B"]):
        one, ids1 = rr(*(t[b:b + 1].cuda() for t in r["inputs"]), return_ids=True)
        assert torch.equal(one[0], out[b]) and torch.equal(ids1[0], ids[b])
    with pytest.raises(ValueError, match="int32"):
        rr.blend(screen, colours, ids.long())
    with pytest.raises(ValueError, match="even"):
        mr.MeshRenderer(r["m"], r["focal"], 64, 71, "cuda")


# ---- short fits --------------------------------------------------------------------------------------------------------------
# Seed 41, perturbation scale 1.0 (tests/photo_helpers.fit_problem), checked on the CPU: the fp64 statement's colour loss
# falls from 19.30 to 4.17 (x 0.22) over the 12 iterations of the light fit, and from 2.78 to 1.59 (x 0.57) over the 8
# iterations of the first batch of the fine fit that follows it.
FIT = dict(n=7, seed=41, F=10, H=16, W=16, batch=4, light_iters=12, fine_iters=8)
_FITS = {}


def fits():
    if not _FITS:
        m = ph.model(FIT["n"], FIT["seed"])
        p = ph.fit_problem(m, FIT["F"], FIT["H"], FIT["W"], FIT["seed"])
        start = {k: v.float() for k, v in p["start"].items()}
        _FITS.update(m=m, p=p, start=start)
        for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
            tl, tf = [], []
            a = mr.fit_light_torch(m, start, p["lms"], p["images"], p["focal"], FIT["H"], FIT["W"], FIT["batch"], FIT["light_iters"],
                                   dtype=dtype, trace=tl, **p["settings"])
            b = mr.fit_frames_torch(m, a, p["lms"], p["images"], p["focal"], FIT["H"], FIT["W"], FIT["batch"], FIT["fine_iters"],
                                    dtype=dtype, trace=tf, **p["settings"])
            _FITS["light" + tag], _FITS["fine" + tag], _FITS["trace" + tag] = a, b, (tl, tf)
    return _FITS


def test_short_light_fit_follows_the_fp64_statement():
    f = fits()
    p, trace = f["p"], []
    tl64 = f["trace64"][0]
    print(f"fp64 statement: colour loss {tl64[0]['col']:.3e} -> {tl64[-1]['col']:.3e}")
    assert tl64[-1]["col"] < 0.5 * tl64[0]["col"]
    got = mr.PhotometricTracker(f["m"], "cuda").fit_light(f["start"], p["lms"], p["images"], p["focal"], FIT["H"], FIT["W"], FIT["batch"],
                                                          FIT["light_iters"], trace=trace, **p["settings"])
    print(f"hip: colour loss {trace[0]['col']:.3e} -> {trace[-1]['col']:.3e}")
    ph.assert_parity(ph.parity(got, f["light64"], f["light32"]), "light fit")
    assert trace[-1]["col"] < trace[0]["col"]


def test_short_fine_fit_follows_the_fp64_statement():
    f = fits()
    p, trace = f["p"], []
    tf64 = [t for t in f["trace64"][1] if t["batch"] == 0]
    print(f"fp64 statement: colour loss of batch 0 {tf64[0]['col']:.3e} -> {tf64[-1]['col']:.3e}")
    assert tf64[-1]["col"] < tf64[0]["col"]
    start = {k: v.float() for k, v in f["light64"].items()}
    want64 = mr.fit_frames_torch(f["m"], start, p["lms"], p["images"], p["focal"], FIT["H"], FIT["W"], FIT["batch"], FIT["fine_iters"],
                                 dtype=torch.float64, **p["settings"])
    want32 = mr.fit_frames_torch(f["m"], start, p["lms"], p["images"], p["focal"], FIT["H"], FIT["W"], FIT["batch"], FIT["fine_iters"],
                                 dtype=torch.float32, **p["settings"])
    got = mr.PhotometricTracker(f["m"], "cuda").fit_frames(start, p["lms"], p["images"], p["focal"], FIT["H"], FIT["W"], FIT["batch"],
                                                           FIT["fine_iters"], trace=trace, **p["settings"])
    assert sorted({(t["start"], t["end"]) for t in trace}) == [(0, 4), (4, 8), (6, 10)]              # the last batch overlaps
    ph.assert_parity(ph.parity(got, want64, want32), "fine fit")
    first = [t for t in trace if t["batch"] == 0]
    print(f"hip: colour loss of batch 0 {first[0]['col']:.3e} -> {first[-1]['col']:.3e}")
    assert first[-1]["col"] < first[0]["col"]


def test_track_identity_photometric_writes_and_round_trips(tmp_path):
    from PIL import Image
    f = fits()
    p, m = f["p"], f["m"]
    os.makedirs(tmp_path / "ori_imgs")
    for i in range(FIT["F"]):
        np.savetxt(tmp_path / "ori_imgs" / f"{i}.lms", p["lms"][i].numpy(), fmt="%.6f")
        Image.fromarray(p["images"][i].numpy()).save(tmp_path / "ori_imgs" / f"{i}.jpg", quality=95)
    kw = dict(focals=(p["focal"],), every=3, focal_iters=(30, 30), coarse_iters=(30, 30), photo_batch=4, **p["settings"])
    plain = track.track_identity(str(tmp_path), m, "cuda", write=False, **kw)
    out = track.track_identity(str(tmp_path), m, "cuda", photometric=True, light_iters=4, fine_iters=3, **kw)
    for name in ("track_params.pt", "transforms_train.json", "transforms_val.json"):
        assert os.path.getsize(tmp_path / name) > 0
    saved = torch.load(tmp_path / "track_params.pt")
    assert list(saved) == ["id", "exp", "euler", "trans", "focal"]
    for k, s in dict(id=(1, m.id_dim), exp=(FIT["F"], m.exp_dim), euler=(FIT["F"], 3), trans=(FIT["F"], 3), focal=(1,)).items():
        assert tuple(saved[k].shape) == s and saved[k].device.type == "cpu" and torch.equal(saved[k], out[k])
        assert torch.isfinite(saved[k]).all()
    assert torch.equal(out["focal"], plain["focal"]) and not torch.equal(out["euler"], plain["euler"])
    assert float(saved["trans"][:, 2].mean()) < -3.0
