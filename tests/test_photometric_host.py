"""Host: the plain statement of the mesh renderer and of the two photometric fits (instag_amd/mesh_render.py).

Golden G13 (tests/golden/g13_photometric.npz, generator make_golden_photometric.py) holds the reference's own forward_geo,
forward_geo_sub, forward_tex, forward_rott, cal_col_loss, cal_lap_loss, Render_3DMM.compute_normal and
Illumination_layer on the seeded model of tests/photo_helpers.py.  On the generating machine the fp32 statement was
bit-equal to all eight; the test asks for 4 x the spread the generator recorded (|reference fp32 - statement fp64| on the
same inputs: geo 1.0e-7, geo_sub 8.1e-8, tex 1.4e-5, rott 2.7e-7, normal 2.0e-6, colour 1.8e-4, col_loss 2.1e-6, lap_loss
1.3e-8; never below 4 fp32 ulp of the magnitude), because a GEMM or a reduction may be ordered differently by another
CPU, and for bit-equality of the vertex normals, which are element-wise operations and a sum of M terms."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from instag_amd import mesh_render as mr
from instag_amd import track
from tests import photo_helpers as ph
from tests import track_helpers as th

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_photometric.npz")
KEYS = ("geo", "geo_sub", "tex", "rott", "normal", "colour", "col_loss", "lap_loss")


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    m = ph.model(7, 13)
    d = {k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("in_")}
    B = d["exp"].shape[0]
    tris, vert_tris = m.topology_tensors("cpu")
    ids = d["id"].expand(B, -1)
    geo = mr.geometry_torch(m, ids, d["exp"])
    sub = mr.geometry_sub_torch(m, ids, d["exp"], m.rigid_ids)
    tex = mr.texture_torch(m, d["tex"].expand(B, -1))
    rott = mr.rott_torch(geo, d["euler"], d["trans"])
    normal = mr.vertex_normals_torch(rott, tris, vert_tris)
    rott_sub = mr.rott_torch(sub, d["euler"], d["trans"])
    r = dict(geo=geo, geo_sub=sub, tex=tex, rott=rott, normal=normal, colour=mr.illumination_torch(tex, normal, d["light"]),
             col_loss=mr.color_loss_torch(d["pred"], d["gt"], d["mask"]),
             lap_loss=mr.lap_loss_torch(rott_sub.reshape(B, -1).permute(1, 0)),
             normal_of_golden_rott=mr.vertex_normals_torch(torch.as_tensor(g["rott"]), tris, vert_tris))
    return g, r, d


@pytest.mark.parametrize("key", KEYS)
def test_fp32_statement_reproduces_the_reference(golden, key):
    g, r, _ = golden
    want = torch.as_tensor(g[key]).double()
    err = float((r[key].double().reshape(want.shape) - want).abs().max())
    bound = 4 * max(float(g[f"spread_{key}"]), ph.EPS32 * float(want.abs().max()))
    print(f"{key}: |statement - reference| = {err:.3e}, bound {bound:.3e}")
    assert r[key].dtype == torch.float32 and err <= bound


def test_vertex_normals_are_bit_equal_to_the_reference(golden):
    g, r, _ = golden
    assert np.array_equal(r["normal_of_golden_rott"].numpy(), g["normal"])


def test_golden_inputs_are_the_seeded_scene(golden):
    g, _, d = golden
    sc = ph.scene(ph.model(7, 13), 4, 13)
    for k in ("id", "exp", "tex", "euler", "trans", "light"):
        assert torch.equal(sc[k].float(), d[k])


# ---- the model -------------------------------------------------------------------------------------------------------------
def test_model_loads_texture_and_topology_and_still_serves_the_landmark_fit(tmp_path):
    info, keys, topo = ph.model_arrays(5, 3)
    m = track.Face3DMM.from_arrays(info, keys, 4, 3, topo=topo, tex_dim=5)
    assert m.has_texture and m.has_topology and m.tex_dim == 5 and m.N == 25
    assert m.base_tex.shape == (5, 75) and np.array_equal(m.base_tex, info["b_tex"][:5]) and np.array_equal(m.mu_tex, info["mu_tex"])
    assert np.array_equal(m.sig_tex, info["sig_tex"][:5]) and np.array_equal(m.rigid_ids, keys["rigid_ids"])
    assert m.tris.shape == (32, 3) and m.vert_tris.shape[0] == 25
    for name, d in (("3DMM_info", info), ("keys_info", keys), ("topology_info", topo)):
        np.save(str(tmp_path / f"{name}.npy"), d, allow_pickle=True)
    loaded = track.Face3DMM.load(str(tmp_path), 4, 3, tex_dim=5)
    assert np.array_equal(loaded.tris, m.tris) and np.array_equal(loaded.vert_tris, m.vert_tris) and loaded.tex_dim == 5
    plain = track.Face3DMM.from_arrays({k: v for k, v in info.items() if "tex" not in k},
                                       {k: v for k, v in keys.items() if k != "rigid_ids"}, 4, 3)
    assert not plain.has_texture and not plain.has_topology and plain.rigid_ids is None
    assert np.array_equal(plain.base_id, m.base_id) and np.array_equal(plain.points, m.points)
    with pytest.raises(ValueError, match="without topology"):
        plain.topology_tensors("cpu")
    with pytest.raises(ValueError, match="without texture"):
        plain.texture_tensors("cpu", torch.float32)


@pytest.mark.parametrize("bad", [-1, 32])
def test_vert_tris_outside_the_triangles_raises(bad):
    info, keys, topo = ph.model_arrays(5, 3)
    vt = topo["vert_tris"].copy()
    vt[7, 1] = bad
    with pytest.raises(ValueError, match="vert_tris"):
        track.Face3DMM.from_arrays(info, keys, 4, 3, topo=dict(tris=topo["tris"], vert_tris=vt), tex_dim=5)


def test_a_triangle_listed_twice_counts_twice():
    geo = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=torch.float64)
    tris = torch.tensor([[0, 1, 2], [0, 2, 3]])
    once = mr.vertex_normals_torch(geo, tris, torch.tensor([[0, 1]] * 4))
    twice = mr.vertex_normals_torch(geo, tris, torch.tensor([[0, 0, 1]] * 4))
    n = lambda v: v / v.norm()
    assert torch.allclose(once[0, 0], n(torch.tensor([1.0, 0, 1], dtype=torch.float64)))
    assert torch.allclose(twice[0, 0], n(torch.tensor([1.0, 0, 2], dtype=torch.float64)))


# ---- hand-checkable facts of the statement, fp64 ---------------------------------------------------------------------------
H8 = W8 = 8
S8 = 2.0 / 8
SIG8 = ph.scaled_sigma(8, 8)


def _t(a):
    return torch.tensor(a, dtype=torch.float64)


def _seg(p, a, b):
    d = b - a
    t = np.clip(np.dot(p - a, d) / np.dot(d, d), 0, 1)
    return float(np.sum((p - (a + t * d)) ** 2))


def test_one_triangle_gives_the_interpolated_colour_and_the_sigmoid_of_its_edge_distance():
    screen = _t([[[1.2, 1.1, 7.0], [6.3, 2.0, 7.2], [3.1, 6.4, 6.9]]])
    colours = _t([[[200.0, 10, 30], [20, 180, 60], [90, 40, 220]]])
    tris = torch.tensor([[0, 1, 2]])
    ids = mr.select_torch(screen, tris, H8, W8, mr.blur_radius_of(SIG8))
    out = mr.blend_torch(screen, colours, tris, ids, H8, W8, sigma=SIG8)
    i, j = 3, 3                                                     # centre (3.5, 3.5): inside
    assert ids[0, i, j].tolist() == [0, -1]
    p = np.array([j + 0.5, i + 0.5])
    v = screen[0, :, :2].numpy()
    A = np.array([[v[0, 0], v[1, 0], v[2, 0]], [v[0, 1], v[1, 1], v[2, 1]], [1, 1, 1]])
    w = np.linalg.solve(A, np.array([p[0], p[1], 1.0]))
    assert (w > 0).all()
    want = w @ colours[0].numpy()
    d2 = min(_seg(p, v[a], v[b]) for a, b in ((0, 1), (1, 2), (2, 0))) * S8 ** 2
    assert np.abs(out[0, i, j, :3].numpy() - want).max() < 1e-6     # (up to delta = 1e-10 against a weight of ~ 0.5)
    assert abs(float(out[0, i, j, 3]) - 1 / (1 + math.exp(-d2 / SIG8))) < 1e-12


def test_a_pixel_beyond_the_blur_radius_of_every_face_is_exactly_zero():
    screen = _t([[[1.2, 1.1, 7.0], [4.3, 1.5, 7.2], [2.1, 4.4, 6.9]]])
    colours = _t([[[200.0, 10, 30], [20, 180, 60], [90, 40, 220]]])
    tris = torch.tensor([[0, 1, 2]])
    br = mr.blur_radius_of(SIG8)
    ids = mr.select_torch(screen, tris, H8, W8, br)
    out = mr.blend_torch(screen, colours, tris, ids, H8, W8, sigma=SIG8)
    far = math.sqrt(_seg(np.array([7.5, 7.5]), screen[0, 1, :2].numpy(), screen[0, 2, :2].numpy())) * S8
    assert far ** 2 > br and ids[0, 7, 7].tolist() == [-1, -1]
    assert torch.equal(out[0, 7, 7], torch.zeros(4, dtype=torch.float64))
    assert ids[0, 1, 4].tolist() == [0, -1]                            # outside the face, inside the blur radius: drawn
    assert 0 < float(out[0, 1, 4, 3]) < 0.5


def test_two_parallel_triangles_give_the_front_colour_up_to_the_depth_softmax():
    dz = 0.01
    xy = [[1.2, 1.1], [6.3, 2.0], [3.1, 6.4]]
    screen = _t([[p + [7.0 + dz] for p in xy] + [p + [7.0] for p in xy]])       # face 0 behind, face 1 in front
    c_back, c_front = [200.0, 10, 30], [20.0, 180, 60]
    colours = _t([[c_back] * 3 + [c_front] * 3])
    tris = torch.tensor([[0, 1, 2], [3, 4, 5]])
    ids = mr.select_torch(screen, tris, H8, W8, mr.blur_radius_of(SIG8))
    assert ids[0, 3, 3].tolist() == [1, 0]                                        # nearest first
    out = mr.blend_torch(screen, colours, tris, ids, H8, W8, sigma=SIG8)
    e = math.exp(-(dz / (mr.ZFAR - mr.ZNEAR)) / mr.GAMMA)
    want = (np.array(c_front) + e * np.array(c_back)) / (1 + e)                   # equal coverage probabilities
    assert np.abs(out[0, 3, 3, :3].numpy() - want).max() < 1e-6
    assert np.abs(out[0, 3, 3, :3].numpy() - np.array(c_front)).max() <= e * 255


def test_faces_sharing_the_nearest_corner_tie_exactly_and_the_lower_index_wins():
    # three overlapping triangles with corner (4.4, 4.4) in common, each opening towards (+1, +1): pixel (3, 3) (centre
    # 3.5, 3.5) lies beyond that corner of all three, so its clipped barycentrics are (1, 0, 0) in each
    screen = _t([[[4.4, 4.4, 7.0], [7.5, 4.6, 7.3], [4.7, 7.6, 6.8], [7.4, 5.4, 7.1], [5.4, 7.4, 7.4], [6.9, 4.9, 6.9],
                  [5.2, 7.3, 7.2]]])
    colours = _t([[[200.0, 10, 30], [20, 180, 60], [90, 40, 220], [10, 20, 30], [60, 70, 80], [15, 25, 35], [65, 75, 85]]])
    tris = torch.tensor([[0, 1, 2], [0, 3, 4], [0, 5, 6]])
    br = mr.blur_radius_of(SIG8)
    t = mr.candidates_dense_torch(screen, tris, H8, W8, br)
    assert t["cand"][0, 3, 3].all() and not t["inside"][0, 3, 3].any()
    pz = t["pz"][0, 3, 3]
    assert pz[0] == pz[1] == pz[2] == 7.0 and t["dist"][0, 3, 3, 0] == t["dist"][0, 3, 3, 1] == t["dist"][0, 3, 3, 2]
    ids = mr.select_torch(screen, tris, H8, W8, br)
    assert ids[0, 3, 3].tolist() == [0, 1]
    outs = []
    for pair in ([0, 1], [1, 0], [0, 2], [1, 2]):
        forced = ids.clone()
        forced[0, 3, 3] = torch.tensor(pair)
        outs.append(mr.blend_torch(screen, colours, tris, forced, H8, W8, sigma=SIG8)[0, 3, 3])
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    assert torch.allclose(outs[0][:3], colours[0, 0], rtol=1e-8)


@pytest.fixture(scope="module")
def grid_scene():
    H, W = 48, 56
    m = ph.model(9, 31)
    sc = ph.scene(m, 2, 31)
    tris, vert_tris = m.topology_tensors("cpu")
    sigma = ph.scaled_sigma(H, W)
    screen = mr.screen_torch(sc["rott_geo"], ph.focal_for(H, W), H, W)
    colours = mr.vertex_stage_torch(sc["rott_geo"], sc["texture"], sc["light"], tris, vert_tris)
    ids = mr.select_torch(screen, tris, H, W, mr.blur_radius_of(sigma))
    out = mr.blend_torch(screen, colours, tris, ids, H, W, sigma=sigma)
    risk = ph.flip_risk(screen, tris, H, W, mr.blur_radius_of(sigma))
    return dict(H=H, W=W, m=m, sc=sc, tris=tris, vert_tris=vert_tris, sigma=sigma, screen=screen, colours=colours, ids=ids, out=out,
                risk=risk)


def test_the_face_order_does_not_matter(grid_scene):
    g = grid_scene
    perm = torch.as_tensor(np.random.default_rng(5).permutation(g["tris"].shape[0]))
    tris = g["tris"][perm]
    ids = mr.select_torch(g["screen"], tris, g["H"], g["W"], mr.blur_radius_of(g["sigma"]))
    out = mr.blend_torch(g["screen"], g["colours"], tris, ids, g["H"], g["W"], sigma=g["sigma"])
    keep = ~g["risk"]
    assert float(g["risk"].float().mean()) < 0.05
    assert float((out - g["out"])[keep].abs().max()) < 1e-9
    same = torch.where(ids >= 0, perm[ids.clamp(min=0)], ids).sort(dim=-1).values == g["ids"].sort(dim=-1).values
    assert float(same.all(dim=-1)[keep].float().mean()) > 0.99                    # (exact ties may name another face)


def test_a_shift_by_whole_pixels_shifts_the_image(grid_scene):
    g = grid_scene
    dx, dy = 3, 2
    screen = g["screen"] + _t([float(dx), float(dy), 0.0])
    br = mr.blur_radius_of(g["sigma"])
    ids = mr.select_torch(screen, g["tris"], g["H"], g["W"], br)
    out = mr.blend_torch(screen, g["colours"], g["tris"], ids, g["H"], g["W"], sigma=g["sigma"])
    keep = ~(g["risk"][:, :-dy, :-dx] | ph.flip_risk(screen, g["tris"], g["H"], g["W"], br)[:, dy:, dx:])
    assert float((out[:, dy:, dx:] - g["out"][:, :-dy, :-dx])[keep].abs().max()) < 1e-7


def test_a_face_behind_the_camera_and_a_zero_area_face_draw_nothing_and_get_no_gradient(grid_scene):
    g = grid_scene
    V, T = g["screen"].shape[1], g["tris"].shape[0]
    behind = _t([[[-50.0, -50, -1.0], [150, -40, -2.0], [30, 160, -0.5]]]).expand(2, -1, -1)
    screen = torch.cat((g["screen"], behind), dim=1).clone().requires_grad_(True)
    colours = torch.cat((g["colours"], torch.full((2, 3, 3), 100.0, dtype=torch.float64)), dim=1).clone().requires_grad_(True)
    a, b = g["tris"][40, 0].item(), g["tris"][40, 1].item()
    tris = torch.cat((g["tris"], torch.tensor([[V, V + 1, V + 2], [a, b, b]])))
    ids = mr.select_torch(screen.detach(), tris, g["H"], g["W"], mr.blur_radius_of(g["sigma"]))
    assert int((ids >= T).sum()) == 0 and torch.equal(ids, g["ids"])
    out = mr.blend_torch(screen, colours, tris, ids, g["H"], g["W"], sigma=g["sigma"])
    assert torch.equal(out, g["out"])
    gs, gc = torch.autograd.grad((out * torch.randn(out.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))).sum(),
                                 [screen, colours])
    assert torch.isfinite(gs).all() and torch.equal(gs[:, V:], torch.zeros(2, 3, 3, dtype=torch.float64))
    assert torch.equal(gc[:, V:], torch.zeros(2, 3, 3, dtype=torch.float64)) and float(gs[:, :V].abs().max()) > 0
    # forced into a slot, the zero-area face still yields finite numbers (its area is replaced by 1, as in the kernels)
    forced = ids.clone()
    forced[0, 5, 5, 1] = T + 1
    out = mr.blend_torch(screen, colours, tris, forced, g["H"], g["W"], sigma=g["sigma"])
    assert torch.isfinite(out).all() and all(torch.isfinite(x).all() for x in torch.autograd.grad(out.sum(), [screen, colours]))


def test_gradcheck_of_the_blend_with_fixed_ids():
    rng = np.random.default_rng(8)
    screen = _t([[[1.2, 1.1, 7.0], [6.3, 2.0, 7.2], [3.1, 6.4, 6.9], [6.9, 6.6, 7.1], [0.9, 5.2, 7.05]]])
    colours = _t(rng.uniform(40, 220, (1, 5, 3)))
    tris = torch.tensor([[0, 1, 2], [1, 3, 2], [0, 2, 4]])
    ids = mr.select_torch(screen, tris, H8, W8, mr.blur_radius_of(SIG8))
    assert int((ids[..., 1] >= 0).sum()) > 5
    _, terms = mr.blend_torch(screen, colours, tris, ids, H8, W8, sigma=SIG8, return_terms=True)
    assert not ph.gradient_kinks(terms, ids).any()
    f = lambda s, c: mr.blend_torch(s, c, tris, ids, H8, W8, sigma=SIG8)
    assert torch.autograd.gradcheck(f, (screen.clone().requires_grad_(True), colours.clone().requires_grad_(True)),
                                    eps=1e-7, atol=1e-5, rtol=1e-4)


def test_odd_width_raises():
    screen = _t([[[1.2, 1.1, 7.0], [6.3, 2.0, 7.2], [3.1, 6.4, 6.9]]])
    with pytest.raises(ValueError, match="even"):
        mr.select_torch(screen, torch.tensor([[0, 1, 2]]), 8, 7)


# ---- the schedules of the two fits, on the CPU statement -------------------------------------------------------------------
def test_schedules_are_the_reference_loops():
    s = mr.light_schedule()
    assert len(s) == 71
    assert all(x == (1.0, 3.0, 2.0, 1.0) for x in s[:51])                       # the rate change follows the step of iteration 50
    assert all(x == (0.2, 0.05, 1.0, 0.8) for x in s[51:])                      # and only that one (iter % 50 == 0 and iter > 0)
    assert mr.fine_schedule() == [8.0] * 31 + [1.5] * 19
    assert mr.light_frames(10, 4).tolist() == [0, 2, 4, 6] and mr.light_frames(7000, 32).tolist() == list(range(0, 7000, 218))[:32]
    assert mr.fine_batches(10, 4) == [(0, 4), (4, 8), (6, 10)] and mr.fine_batches(64, 32) == [(0, 32), (32, 64)]
    with pytest.raises(ValueError, match="at least 32 frames"):
        mr.light_frames(31)


@pytest.fixture(scope="module")
def problem():
    m = ph.model(7, 41)
    return m, ph.fit_problem(m, 10, 16, 16, 41)


def test_light_fit_follows_its_schedule_and_leaves_unselected_rows_alone(problem):
    m, p = problem
    trace = []
    out = mr.fit_light_torch(m, p["start"], p["lms"], p["images"], p["focal"], 16, 16, batch=4, iters=53, dtype=torch.float64,
                             trace=trace, **p["settings"])
    assert [t["iter"] for t in trace] == list(range(53)) and trace[0]["frames"] == [0, 2, 4, 6]
    assert all(t["lr_tl"] == 0.1 and t["lr_idf"] == 0.01 and t["w_lan"] == 3.0 for t in trace[:51])
    assert all(abs(t["lr_tl"] - 0.02) < 1e-15 and abs(t["lr_idf"] - 0.002) < 1e-15 and t["w_lan"] == 0.05 and t["w_id"] == 1.0
               and t["w_exp"] == 0.8 for t in trace[51:])
    assert trace[-1]["col"] < trace[0]["col"]
    for k in ("exp", "euler", "trans"):
        for row in (1, 3, 5, 7, 8, 9):
            assert torch.equal(out[k][row], p["start"][k][row])
        assert not torch.equal(out[k][0], p["start"][k][0])
    assert out["light"].shape == (10, 27) and all(torch.equal(out["light"][0], r) for r in out["light"])    # the mean, broadcast
    assert out["tex"].shape == (1, m.tex_dim) and float(out["light"].abs().max()) > 0


def test_fine_fit_batches_overlap_at_the_end_and_take_the_preceding_frames_detached(problem):
    m, p = problem
    base = {k: v.clone() for k, v in p["start"].items()}
    base["tex"], base["light"] = p["tex"], p["light"] * 0.9
    trace = []
    out = mr.fit_frames_torch(m, base, p["lms"], p["images"], p["focal"], 16, 16, batch=4, iters=33, dtype=torch.float64,
                              trace=trace, **p["settings"])
    assert sorted({(t["batch"], t["start"], t["end"]) for t in trace}) == [(0, 0, 4), (1, 4, 8), (2, 6, 10)]
    # the frames in front of start_n join the Laplacian, five at the most: 4 of 4, then 5 of 6
    assert all(t["lap_frames"] == {0: 4, 1: 8, 2: 9}[t["batch"]] for t in trace)
    assert all(t["w_lan"] == (1.5 if t["iter"] > 30 else 8.0) for t in trace)
    # the first eight frames alone: the same batches (0,4), (4,8).  Frames 0 .. 5 of the long run are theirs, bit for bit:
    # later batches read earlier frames (detached) and never write them
    short = {k: (v[:8].clone() if v.shape[0] == 10 else v.clone()) for k, v in base.items()}
    out8 = mr.fit_frames_torch(m, short, p["lms"][:8], p["images"][:8], p["focal"], 16, 16, batch=4, iters=33, dtype=torch.float64,
                               **p["settings"])
    for k in ("exp", "euler", "trans", "light"):
        assert torch.equal(out[k][:6], out8[k][:6])
        assert not torch.equal(out[k][6:8], out8[k][6:8])                           # refitted by the last batch [6, 10)
        assert not torch.equal(out[k][9], base[k][9])
    assert torch.equal(out["id"], base["id"]) and torch.equal(out["tex"], base["tex"])


def test_an_empty_mask_names_the_frame(problem):
    m, p = problem
    away = {k: v.clone() for k, v in p["start"].items()}
    away["trans"][2, 0] += 40.0                                                     # frame 2 leaves the image
    with pytest.raises(ValueError, match="frame 2"):
        mr.fit_light_torch(m, away, p["lms"], p["images"], p["focal"], 16, 16, batch=4, iters=1, **p["settings"])


# ---- track_identity ----------------------------------------------------------------------------------------------------------
def _write_identity(directory, lms, images):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for i, (l, im) in enumerate(zip(lms, images)):
        np.savetxt(os.path.join(directory, f"{i}.lms"), l.numpy(), fmt="%.6f")
        Image.fromarray(im.numpy()).save(os.path.join(directory, f"{i}.jpg"), quality=95)


def test_track_identity_photometric_runs_end_to_end_on_the_cpu(tmp_path, problem):
    m, p = problem
    _write_identity(str(tmp_path / "ori_imgs"), p["lms"], p["images"])
    kw = dict(focals=(p["focal"],), every=4, focal_iters=(3, 3), coarse_iters=(30, 3), photo_batch=4, light_iters=2, fine_iters=2,
              **p["settings"])
    plain = track.track_identity(str(tmp_path), m, "cpu", write=False, **kw)
    out = track.track_identity(str(tmp_path), m, "cpu", photometric=True, **kw)
    saved = torch.load(os.path.join(str(tmp_path), "track_params.pt"))
    assert list(saved) == ["id", "exp", "euler", "trans", "focal"]
    for k, s in dict(id=(1, m.id_dim), exp=(10, m.exp_dim), euler=(10, 3), trans=(10, 3), focal=(1,)).items():
        assert tuple(saved[k].shape) == s and saved[k].dtype == torch.float32 and torch.isfinite(saved[k]).all()
        assert torch.equal(saved[k], out[k])
    assert not torch.equal(out["euler"], plain["euler"]) and torch.equal(out["focal"], plain["focal"])
    assert os.path.exists(tmp_path / "transforms_train.json") and os.path.exists(tmp_path / "transforms_val.json")
    os.remove(tmp_path / "ori_imgs" / "3.jpg")
    with pytest.raises(ValueError, match="jpg"):
        track.track_identity(str(tmp_path), m, "cpu", photometric=True, h=16, w=16, **kw)
    with pytest.raises(ValueError, match="at least 32 frames"):
        track.track_identity(str(tmp_path), m, "cpu", photometric=True, h=16, w=16, **dict(kw, photo_batch=32))


def test_track_identity_photometric_needs_texture_and_topology(tmp_path, problem):
    _, p = problem
    m = th.model(4, 2, 5, 3)
    _write_identity(str(tmp_path / "ori_imgs"), p["lms"], p["images"])
    with pytest.raises(ValueError, match="topology"):
        track.track_identity(str(tmp_path), m, "cpu", photometric=True, photo_batch=4)


# ---- the C entry points --------------------------------------------------------------------------------------------------------
def test_mesh_argument_errors_do_not_need_a_gpu():
    from instag_amd import _lib
    lib = _lib.lib()
    E_ARG, one = 1, 16

    def settings(**kw):
        s = _lib.MeshSettings()
        s.H, s.W, s.K = 8, 8, 2
        s.sigma, s.gamma, s.blur_radius, s.znear, s.zfar, s.eps = 1e-4, 1e-4, 5e-5, 0.01, 20.0, 1e-10
        for k, v in kw.items():
            setattr(s, k, v)
        return ctypes.byref(s)

    def all_calls(s, null=False):
        p = None if null else one
        return (lib.instag_mesh_select(s, p, one, 1, 3, 1, one, one, None),
                lib.instag_mesh_blend_forward(s, one, p, one, one, 1, 3, 1, one, None),
                lib.instag_mesh_blend_backward(s, one, one, one, one, p, 1, 3, 1, one, one, None))

    for bad, text in ((dict(W=7), b"even"), (dict(K=1), b"K = 2"), (dict(K=3), b"K = 2"), (dict(H=0), b"H in"), (dict(sigma=0.0), b"sigma"),
                      (dict(zfar=0.0), b"zfar")):
        for rc in all_calls(settings(**bad)):
            assert rc == E_ARG and text in lib.instag_last_error(), (bad, lib.instag_last_error())
    for rc in all_calls(settings(), null=True):
        assert rc == E_ARG and b"NULL" in lib.instag_last_error()
    assert lib.instag_mesh_select(None, one, one, 1, 3, 1, one, one, None) == E_ARG and b"NULL" in lib.instag_last_error()
    assert lib.instag_mesh_select(settings(), one, one, 0, 3, 1, one, one, None) == E_ARG
    # (calls whose arguments all pass would launch on these placeholder pointers: only the rejected forms are made)
    assert lib.instag_mesh_vertex_forward(one, one, one, one, one, 1, 3, 1, 0, one, None) == E_ARG and b"M " in lib.instag_last_error()
    assert lib.instag_mesh_vertex_forward(one, None, one, one, one, 1, 3, 1, 4, one, None) == E_ARG and b"NULL" in lib.instag_last_error()
    assert lib.instag_mesh_vertex_backward(one, one, one, one, one, one, 1, 3, 1, 4, one, one, None, one, 1 << 20, None) == E_ARG
    assert lib.instag_mesh_vertex_backward(one, one, one, one, one, one, 1, 3, 1, 4, one, one, one, one, 8, None) == 3    # E_SPACE
    assert lib.instag_mesh_vertex_backward_workspace_bytes(2, 300) == 2 * 2 * 27 * 8
    for name in ("instag_mesh_vertex_forward", "instag_mesh_vertex_backward", "instag_mesh_select", "instag_mesh_blend_forward",
                 "instag_mesh_blend_backward", "instag_mesh_vertex_backward_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 10


def test_renderer_and_tracker_on_a_cpu_device_point_to_the_statement():
    m = ph.model(5, 3)
    with pytest.raises(ValueError, match="render_torch"):
        mr.MeshRenderer(m, 100.0, 16, 16, device="cpu")
    with pytest.raises(ValueError, match="fit_light_torch"):
        mr.PhotometricTracker(m, "cpu")
