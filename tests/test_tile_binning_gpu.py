"""GPU: the one-pass instance sort (digit = the whole tile id, csrc/raster_sort.hip tile_pass_kernel) bins exactly
like the digit passes + range kernel it replaces (INSTAG_TILE_SORT=passes): point_list, ranges, sorted keys and
num_rendered bit for bit, images and gradients bit for bit, eager and in capacity mode."""
import numpy as np
import pytest
import torch

from tests.helpers import hip_settings, leaf, make_scene

pytestmark = pytest.mark.gpu


def scene(n, width, height, seed=0):
    a, settings = make_scene(n, max(width, height), seed=seed)
    settings = dict(settings, image_width=width, image_height=height)
    return a, settings


def forward(a, settings, monkeypatch, mode, backward=False):
    from instag_amd import diff_gauss
    from instag_amd.diff_gauss import GaussianRasterizer, debug_export, rasterize_forward
    if mode == "passes":
        monkeypatch.setenv("INSTAG_TILE_SORT", "passes")
    else:
        monkeypatch.delenv("INSTAG_TILE_SORT", raising=False)
    s = hip_settings(settings)
    g = {k: leaf(v, "cuda") for k, v in a.items()}
    if backward:
        m2 = torch.zeros(g["means3D"].shape[0], 3, device="cuda", requires_grad=True)
        outs = GaussianRasterizer(raster_settings=s)(
            means3D=g["means3D"], means2D=m2, shs=g["shs"], opacities=g["opacities"], scales=g["scales"],
            rotations=g["rotations"], extra_attrs=g["extra"])
        (outs[0].sum() + outs[1].sum() + outs[3].sum()).backward()
        torch.cuda.synchronize()
        grads = {k: v.grad for k, v in g.items() if v.grad is not None}
        grads["means2D"] = m2.grad
        return outs, grads
    with torch.no_grad():
        outs, st = rasterize_forward(s, g["means3D"], g["shs"], None, g["opacities"], g["scales"], g["rotations"],
                                     None, g["extra"])
        d = debug_export(st)
    torch.cuda.synchronize()
    assert diff_gauss.sort_stalls() == 0
    return outs, d


def tiles_of(settings):
    return ((settings["image_width"] + 15) // 16) * ((settings["image_height"] + 15) // 16)


@pytest.mark.parametrize("n,width,height", [
    pytest.param(20000, 512, 512, id="512sq-1024-tiles"),
    pytest.param(100000, 512, 512, id="100k-512sq"),
    pytest.param(8000, 520, 300, id="520x300-ragged"),
    pytest.param(20000, 720, 720, id="720sq-2025-tiles"),
    pytest.param(20000, 1024, 1024, id="1024sq-fallback"),
    pytest.param(1, 256, 256, id="single-gaussian"),
])
def test_one_pass_binning_matches_passes(n, width, height, monkeypatch):
    a, settings = scene(n, width, height, seed=3)
    outs_p, d_p = forward(a, settings, monkeypatch, "passes")
    outs_w, d_w = forward(a, settings, monkeypatch, "one-pass")
    assert d_w["R"] == d_p["R"]
    if n > 1:
        assert d_w["R"] > 0
    for k in ("point_list", "ranges", "keys"):
        assert torch.equal(d_w[k], d_p[k]), k
    for o_w, o_p in zip(outs_w, outs_p):
        assert torch.equal(o_w, o_p)
    ranges = d_w["ranges"].cpu().numpy()
    empty = ranges[:, 1] == ranges[:, 0]
    assert (ranges[empty] == 0).all()                     # an empty tile keeps (0, 0)
    assert ranges.shape[0] == tiles_of(settings)


def test_empty_scene(monkeypatch):
    a, settings = scene(500, 256, 256)
    a["means3D"] = settings["campos"].expand(500, 3).clone()    # every Gaussian at the camera centre: all culled
    for mode in ("passes", "one-pass"):
        outs, d = forward(a, settings, monkeypatch, mode)
        assert d["R"] == 0
        assert not d["ranges"].any()


def test_sorted_keys_are_a_stable_argsort(monkeypatch):
    """The exported (tile << 32 | depth) keys of the one-pass sort are sorted, and instances of one key keep the
    depth sort's order (Gaussian index): a NumPy stable argsort by (tile, depth, index) is the identity."""
    a, settings = scene(20000, 600, 420, seed=5)
    _, d = forward(a, settings, monkeypatch, "one-pass")
    keys = d["keys"].cpu().numpy().view(np.uint64)
    gid = d["point_list"].cpu().numpy().astype(np.int64)
    assert keys.size > 100000
    assert np.array_equal(np.argsort(keys, kind="stable"), np.arange(keys.size))
    order = np.lexsort((gid, keys & 0xFFFFFFFF, keys >> 32))
    assert np.array_equal(order, np.arange(keys.size))
    tile = (keys >> 32).astype(np.int64)
    ranges = d["ranges"].cpu().numpy().astype(np.int64)
    counts = np.bincount(tile, minlength=ranges.shape[0])
    assert np.array_equal(ranges[:, 1] - ranges[:, 0], counts)


@pytest.mark.parametrize("width,height", [(512, 512), (700, 700), (1024, 1024)])
def test_one_pass_gradients_match_passes(width, height, monkeypatch):
    a, settings = scene(20000, width, height, seed=7)
    outs_p, g_p = forward(a, settings, monkeypatch, "passes", backward=True)
    outs_w, g_w = forward(a, settings, monkeypatch, "one-pass", backward=True)
    for o_w, o_p in zip(outs_w, outs_p):
        assert torch.equal(o_w, o_p)
    for k in g_p:
        assert torch.equal(g_w[k], g_p[k]), k


def test_capacity_mode_one_pass(monkeypatch):
    """Capacity mode (instance count a device word, spare capacity unsorted): the one-pass sort gives the eager images
    and gradients; with overflow the call is flagged, its dropped instances taken out of the tile totals (no give-up
    reported, nothing out of bounds)."""
    from instag_amd import diff_gauss
    a, settings = scene(20000, 512, 512, seed=11)
    outs_ref, g_ref = forward(a, settings, monkeypatch, "passes", backward=True)
    R = diff_gauss.LAST_STATS["num_rendered"]
    for mode in ("passes", "one-pass"):
        for cap, expect_overflow in ((int(R * 1.4) + 4096, False), (R, False), (R // 3, True)):
            plan = diff_gauss.CapacityPlan([cap], "cuda")
            diff_gauss.set_capacity_plan(plan)
            try:
                plan.begin_step()
                outs, g = forward(a, settings, monkeypatch, mode, backward=True)
            finally:
                diff_gauss.set_capacity_plan(None)
            assert plan.needed() == [R]
            assert bool(plan.overflowed()) == expect_overflow
            assert diff_gauss.sort_stalls() == 0
            if not expect_overflow:
                for o, r in zip(outs, outs_ref):
                    assert torch.equal(o, r)
                for k in g_ref:
                    assert torch.equal(g[k], g_ref[k]), k
            else:
                assert all(torch.isfinite(v).all() for v in g.values())
