"""Seeded synthetic meshes and scenes for the photometric tests (instag_amd/mesh_render.py).  Nothing of it is committed:
everything is regenerated from its seed, in the layout of the reference's 3DMM_info / keys_info / topology_info
dictionaries, so the golden generator (tests/golden/make_golden_photometric.py) can hand the same arrays to the reference.

The mesh is a jittered n x n grid over the cap of tests/track_helpers.py (x in -1 .. 1, y in -1.2 .. 1.2, real depth
relief), 2 (n - 1)^2 triangles; ``vert_tris`` is padded to the largest vertex degree by cycling a vertex's own triangles,
so repeated entries are exercised.  An optional second, smaller sheet lies 0.35 nearer the camera.  Textures are in
40 .. 220, lights ~ N(0, 0.1)."""
import numpy as np
import torch

from instag_amd import mesh_render as mr
from instag_amd import track

EPS32 = float(np.finfo(np.float32).eps)


def grid_mesh(n, seed, second_sheet=False):
    """-> (pts [V,3], tris [T,3], vert_tris [V,M])."""
    rng = np.random.default_rng(seed)

    def sheet(k, scale, dz):
        gx, gy = np.meshgrid(np.linspace(-1.0, 1.0, k), np.linspace(-1.2, 1.2, k))
        h = 2.0 / (k - 1)
        x = scale * (gx + rng.uniform(-0.3, 0.3, gx.shape) * h)
        y = scale * (gy + rng.uniform(-0.3, 0.3, gy.shape) * h * 1.2)
        z = 0.9 * (1.0 - 0.6 * x ** 2 - 0.4 * y ** 2) + rng.normal(0, 0.02, x.shape) + dz
        idx = np.arange(k * k).reshape(k, k)
        a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
        return np.stack([x.ravel(), y.ravel(), z.ravel()], 1), np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])

    pts, tris = sheet(n, 1.0, 0.0)
    if second_sheet:
        p2, t2 = sheet(max(3, n // 2), 0.45, 0.35)
        tris = np.concatenate([tris, t2 + len(pts)])
        pts = np.concatenate([pts, p2])
    own = [[] for _ in range(len(pts))]
    for t, tri in enumerate(tris):
        for v in tri:
            own[v].append(t)
    M = max(len(o) for o in own)
    vert_tris = np.array([[o[i % len(o)] for i in range(M)] for o in own], dtype=np.int64)
    return pts, tris.astype(np.int64), vert_tris


def model_arrays(n, seed, second_sheet=False, id_dim=4, exp_dim=3, tex_dim=5, P=2):
    """-> (info, keys, topo): the three dictionaries Face3DMM.from_arrays takes, of a grid mesh."""
    pts, tris, vert_tris = grid_mesh(n, seed, second_sheet)
    rng = np.random.default_rng(seed + 500)
    V = len(pts)
    flat = pts.reshape(-1) * 1e5
    info = dict(mu_shape=flat * 0.7, mu_exp=flat * 0.3,
                b_shape=rng.normal(0, 0.01e5, (id_dim + 1, 3 * V)), b_exp=rng.normal(0, 0.01e5, (exp_dim + 1, 3 * V)),
                sig_shape=rng.uniform(0.5, 1.5, id_dim + 1), sig_exp=rng.uniform(0.5, 1.5, exp_dim + 1),
                b_tex=rng.normal(0, 8.0, (tex_dim + 1, 3 * V)), mu_tex=rng.uniform(40.0, 220.0, 3 * V),
                sig_tex=rng.uniform(0.5, 1.5, tex_dim + 1))
    keys = dict(keyinds=rng.integers(0, V, 68).astype(np.int64), left_contour=rng.integers(0, V, (8, P)).astype(np.int64),
                right_contour=rng.integers(0, V, (8, P)).astype(np.int64),
                rigid_ids=rng.choice(V, min(V, 12), replace=False).astype(np.int64))
    return info, keys, dict(tris=tris, vert_tris=vert_tris)


_MODELS = {}


def model(n, seed, second_sheet=False, id_dim=4, exp_dim=3, tex_dim=5, P=2):
    key = (n, seed, second_sheet, id_dim, exp_dim, tex_dim, P)
    if key not in _MODELS:
        info, keys, topo = model_arrays(n, seed, second_sheet, id_dim, exp_dim, tex_dim, P)
        _MODELS[key] = track.Face3DMM.from_arrays(info, keys, id_dim, exp_dim, topo=topo, tex_dim=tex_dim)
    return _MODELS[key]


def focal_for(H, W):
    """The cap (x in -1 .. 1 at depth 7) spans about three quarters of the smaller image side."""
    return 2.6 * min(H, W)


def scene(m, B, seed, euler_std=0.15, shift=0.0, param_std=0.5):
    """-> dict(rott_geo [B,V,3], texture [B,V,3], light [B,27], id, exp, tex, euler, trans) in fp64.  ``shift`` moves the
    mesh sideways (in model units: 1.0 puts half of it off-screen).  ``param_std``: spread of the id / exp / tex
    parameters (the bases are white noise per vertex: on a fine mesh with many basis rows anything but a small spread
    crumples the sheet)."""
    rng = np.random.default_rng(seed + 1000)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    id_para, exp = t(rng.normal(0, 0.5, (1, m.id_dim))) * (param_std / 0.5), t(rng.normal(0, 0.5, (B, m.exp_dim))) * (param_std / 0.5)
    tex = t(rng.normal(0, 0.5, (1, m.tex_dim))) * (param_std / 0.5)
    euler = t(rng.normal(0, euler_std, (B, 3)))
    trans = t(rng.normal(0, 0.1, (B, 3)) + np.array([shift, 0.3 * shift, -7.0]))
    light = t(rng.normal(0, 0.1, (B, 27)))
    geo = mr.geometry_torch(m, id_para.expand(B, -1), exp)
    texture = mr.texture_torch(m, tex.expand(B, -1)).clamp(40.0, 220.0)
    return dict(rott_geo=mr.rott_torch(geo, euler, trans), texture=texture, light=light, id=id_para, exp=exp, tex=tex,
                euler=euler, trans=trans)


def scaled_sigma(H, W):
    """The reference's sigma scaled by (512 / min(H, W))^2: on a small image the blur radius spans as many pixels as it does
    at 512 x 512."""
    return mr.SIGMA * (512.0 / min(H, W)) ** 2


def spoil(sc, m):
    """A copy of a scene with one zero-area face in every image: the third corner of a triangle moved onto its second (the
    first triangle whose corners all belong to three or more triangles, so that no vertex normal becomes 0 / 0)."""
    out = dict(sc)
    g = sc["rott_geo"].clone()
    degree = np.bincount(m.tris.reshape(-1), minlength=m.N)
    tri = m.tris[int(np.nonzero((degree[m.tris] >= 3).all(axis=1))[0][0])]
    g[:, tri[2]] = g[:, tri[1]]
    out["rott_geo"] = g
    return out


# ---- what the statement itself cannot decide in fp32 -------------------------------------------------------------------
def flip_risk(screen64, tris, H, W, blur_radius):
    """[B,H,W] bool: pixels of the fp64 statement where some outside face lies within 1e-3 (relative) of the blur radius,
    or the second and third smallest candidate depth differ by 0 < . <= 1e-5."""
    out = []
    for r0 in range(0, H, 16):
        t = mr.candidates_dense_torch(screen64, tris, H, W, blur_radius, (r0, min(H, r0 + 16)))
        edge = (~t["inside"] & ((t["dist"] - blur_radius).abs() <= 1e-3 * blur_radius)).any(dim=-1)
        pz = torch.where(t["cand"], t["pz"], torch.full_like(t["pz"], float("inf"))).sort(dim=-1).values
        if pz.shape[-1] >= 3:
            gap = pz[..., 2] - pz[..., 1]
            edge |= torch.isfinite(pz[..., 2]) & (gap > 0) & (gap <= 1e-5)
        out.append(edge)
    return torch.cat(out, dim=1)


def gradient_kinks(terms, ids):
    """[B,H,W] bool: a selected face has a barycentric within 1e-6 of 0 or 1, or its two nearest edges within 1e-6 relative.
    Exact ties are no kink: two edges tie exactly where their shared corner is the nearest point of both, and the
    gradient is the same whichever is taken."""
    m = ids >= 0
    near = torch.zeros_like(m)
    for w in terms["w"]:
        near |= (w.abs() <= 1e-6) | ((w - 1.0).abs() <= 1e-6)
    e = torch.stack(terms["edges"], dim=-1).sort(dim=-1).values
    near |= (e[..., 1] > e[..., 0]) & ((e[..., 1] - e[..., 0]) <= 1e-6 * e[..., 1])
    return (near & m).any(dim=-1)


def parity(got, want64, stmt32):
    """Per quantity (|got - fp64|, |fp32 statement - fp64|, bound, floor active): the bound is 4 x the fp32 statement's own
    error against the same fp64 run, never below 4 fp32 ulp of the quantity's largest magnitude (tests/track_helpers.parity)."""
    out = {}
    for k, w in want64.items():
        w = w.double().cpu()
        g, s = got[k].double().cpu(), stmt32[k].double().cpu()
        e32 = float((s - w).abs().max())
        floor = EPS32 * float(w.abs().max())
        out[k] = (float((g - w).abs().max()), e32, 4.0 * max(e32, floor), bool(floor > e32))
    return out


def assert_parity(report, what, record=None):
    for k, (err, e32, bound, floor) in report.items():
        print(f"{what} {k}: |hip - fp64| = {err:.3e}  |fp32 statement - fp64| = {e32:.3e}  bound {bound:.3e}"
              f"{' (ulp floor)' if floor else ''}")
        if record is not None:
            record[f"{what} {k}"] = dict(err=err, e32=e32, bound=bound, floor=floor)
    for k, (err, e32, bound, _) in report.items():
        assert err <= bound, (what, k, err, e32, bound)


# ---- a small photometric fitting problem ---------------------------------------------------------------------------------
def fit_problem(m, F, H, W, seed, scale=1.0):
    """Frames rendered by the fp64 statement from known parameters, and a perturbed start.  -> dict(true, start (params:
    id, exp, euler, trans; fp64), lms [F,68,2] fp32, images uint8 [F,H,W,3], focal, settings)."""
    rng = np.random.default_rng(seed + 3000)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    focal, sigma = focal_for(H, W), scaled_sigma(H, W)
    true = dict(id=t(rng.normal(0, 0.5, (1, m.id_dim))), exp=t(rng.normal(0, 0.4, (F, m.exp_dim))),
                euler=t(rng.normal(0, 0.1, (1, 3)) + rng.normal(0, 0.02, (F, 3))),
                trans=t(np.array([0.0, 0.0, -7.0]) + rng.normal(0, 0.05, (1, 3)) + rng.normal(0, 0.02, (F, 3))))
    tex, light = t(rng.normal(0, 0.5, (1, m.tex_dim))), t(rng.normal(0, 0.1, (1, 27))).repeat(F, 1)
    tris, vert_tris = m.topology_tensors("cpu")
    rott = mr.rott_torch(mr.geometry_torch(m, true["id"].expand(F, -1), true["exp"]), true["euler"], true["trans"])
    img = mr.render_torch(rott, mr.texture_torch(m, tex.expand(F, -1)), light, tris, vert_tris, focal, H, W, sigma=sigma)
    images = torch.where(img[..., 3:] > 0, img[..., :3], torch.zeros_like(img[..., :3])).round().to(torch.uint8)
    lands = track.landmarks_torch(m, true["id"].expand(F, -1), true["exp"], true["euler"], true["trans"], focal, W / 2.0, H / 2.0)
    lms = track.project_torch(lands, true["euler"], true["trans"], focal, W / 2.0, H / 2.0)[:, :, :2].to(torch.float32)
    start = dict(id=true["id"] + scale * t(rng.normal(0, 0.1, (1, m.id_dim))),
                 exp=true["exp"] + scale * t(rng.normal(0, 0.1, (F, m.exp_dim))),
                 euler=true["euler"] + scale * t(rng.normal(0, 0.02, (F, 3))),
                 trans=true["trans"] + scale * t(rng.normal(0, 0.03, (F, 3))))
    return dict(true=true, start=start, tex=tex, light=light, lms=lms, images=images, focal=focal, settings=dict(sigma=sigma))
