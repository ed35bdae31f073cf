"""The colour-only forward blend (``geometry=False``: depth / normal / extra neither blended, checkpointed nor stored,
csrc/raster_blend.hip template parameter GEO) against the full one on the same inputs.

Every kept channel sees the same fp32 operations in the same order in both variants, so the comparisons are
``torch.equal``, not tolerances: image, alpha, aux image, radii, n_contrib, final_T, the tiles' walk lengths, the
backward blend's work list (as a set: its order is that of atomic appends, in two full calls too) and every gradient the
rgb-only backward produces."""
import pytest
import torch

from tests.helpers import hip_settings, leaf, make_scene, oracle_settings

GRAD_KEYS = ("means3D", "means2D", "shs", "opacities", "scales", "rotations", "aux")


def _call(a, settings, geometry, aux, fuse=None, seed=2, repeats=1, use_sh=True):
    """-> list (one per repeat) of dict(outs, state, grads) of a forward + rgb / alpha / aux backward."""
    from instag_amd import diff_gauss
    from instag_amd.diff_gauss import GaussianRasterizer
    n = a["means3D"].shape[0]
    H, W = settings["image_height"], settings["image_width"]
    rast = GaussianRasterizer(hip_settings(settings))
    g = torch.Generator().manual_seed(seed)
    aux0 = torch.rand(n, 3, generator=g)
    w_img, w_alpha, w_aux = (torch.randn(c, H, W, generator=g).cuda() for c in (3, 1, 3))
    results = []
    old = diff_gauss.FUSE_AUX_BACKWARD
    diff_gauss.FUSE_AUX_BACKWARD = fuse
    try:
        for _ in range(repeats):
            plan = diff_gauss._CAPACITY_PLAN
            if plan is not None:
                plan.begin_step()
            inp = {k: leaf(a[k], "cuda") for k in ("means3D", "shs", "opacities", "scales", "rotations")}
            inp["means2D"] = torch.zeros(n, 3, device="cuda", requires_grad=True)
            inp["aux"] = aux0.cuda().requires_grad_(True) if aux else None
            colours = dict(shs=inp["shs"]) if use_sh else dict(colors_precomp=torch.sigmoid(inp["shs"][:, 0, :]))
            diff_gauss.KEEP_LAST_STATE = True
            try:
                outs = rast(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                            scales=inp["scales"], rotations=inp["rotations"], extra_attrs=torch.ones(n, 1, device="cuda"),
                            **colours, **({"aux_colors": inp["aux"]} if aux else {}),
                            **({} if geometry else {"geometry": False}))
                # (a capacity-mode state: no instance lists -- their tail behind the binned count is not data)
                state = diff_gauss.debug_export(diff_gauss.LAST_STATS.pop("state"), lists=plan is None)
            finally:
                diff_gauss.KEEP_LAST_STATE = False
            loss = (outs[0] * w_img).sum() + (outs[3] * w_alpha).sum()
            if aux:
                loss = loss + (outs[6] * w_aux).sum()
            loss.backward()
            results.append(dict(outs=outs, state=state,
                                grads={k: v.grad.clone() for k, v in inp.items() if v is not None and v.grad is not None}))
    finally:
        diff_gauss.FUSE_AUX_BACKWARD = old
    return results


def _same(full, col, aux, what=""):
    fo, co = full["outs"], col["outs"]
    assert co[1] is None and co[2] is None and co[5] is None, what          # depth, normal, extra: not there
    assert fo[1] is not None and fo[2] is not None
    for i, name in ((0, "color"), (3, "alpha"), (4, "radii")) + (((6, "aux"),) if aux else ()):
        assert torch.equal(fo[i], co[i]), (what, name)
    assert col["state"]["geometry"] is False and full["state"]["geometry"] is True
    for k in ("n_contrib", "final_T", "ranges", "point_list", "tiles_touched"):
        assert (k in full["state"]) == (k in col["state"]), (what, k)
        if k in full["state"]:
            assert torch.equal(full["state"][k], col["state"][k]), (what, k)
    if "work_list" in full["state"]:
        assert torch.equal(full["state"]["work_list"], col["state"]["work_list"]), (what, "work list")
        assert full["state"]["blend_mode"] == 0 and col["state"]["blend_mode"] == 1, what
    assert full["grads"].keys() == col["grads"].keys(), what
    for k in GRAD_KEYS:
        if k == "aux" and not aux:
            continue
        assert k in full["grads"], (what, k)
        assert torch.equal(full["grads"][k], col["grads"][k]), (what, k)
        assert bool(torch.isfinite(col["grads"][k]).all()), (what, k)


def _long_walk_scene(size=96):
    """dense and faint: lists of thousands of entries, rays that cross many 128-entry segments (shared tiles exist)"""
    a, settings = make_scene(12000, size, sh_degree=1, seed=11)
    a["opacities"] = a["opacities"] * 0.12
    return a, settings


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["two-stage", "capacity"])
@pytest.mark.parametrize("aux,fuse", [(False, None), (True, False), (True, True)],
                         ids=["no-aux", "aux-split-backward", "aux-fused-backward"])
@pytest.mark.parametrize("kernel,share", [("tile", "0"), ("segment", "0"), ("segment", "1")],
                         ids=["tile", "segment", "segment-share-all"])
def test_colour_only_equals_full(kernel, share, aux, fuse, mode, monkeypatch):
    """Both forward kernels, unshared and shared tiles, with and without the aux colour set (fused and split aux
    backward), eager two-stage and capacity mode -- where every slot is called three times, so that from the second call
    on its walk hints are live and helper workgroups take part."""
    from instag_amd import diff_gauss
    monkeypatch.setenv("INSTAG_BLEND_FWD", kernel)
    monkeypatch.setenv("INSTAG_BLEND_FWD_SHARE_ALL", share)
    a, settings = _long_walk_scene()
    if mode == "two-stage":
        full = _call(a, settings, True, aux, fuse)
        col = _call(a, settings, False, aux, fuse)
    else:
        _call(a, settings, True, aux, fuse)
        cap = int(diff_gauss.LAST_STATS["num_rendered"] * 1.1) + 64
        runs = {}
        for geometry in (True, False):
            plan = diff_gauss.CapacityPlan([cap], "cuda")
            diff_gauss.set_capacity_plan(plan)
            try:
                runs[geometry] = _call(a, settings, geometry, aux, fuse, repeats=3)
                assert plan.overflowed() == []
                if kernel == "segment":
                    assert int((plan.walk_hints[0][:36] >= 24).sum()) > 0      # (hints were live: tiles of >= 3 segments)
            finally:
                diff_gauss.set_capacity_plan(None)
        full, col = runs[True], runs[False]
    assert int(full[0]["state"]["n_contrib"].max()) > 4 * 128, "scene too shallow for this test"
    for rep, (f_, c_) in enumerate(zip(full, col)):
        _same(f_, c_, aux, f"call {rep}")
        _same(full[0], c_, aux, f"call {rep} against the first full call")
    assert diff_gauss.sort_stalls() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["tile", "segment"])
def test_colour_only_ragged_image_and_precomputed_colours(kernel, monkeypatch):
    """200 x 200 is 12.5 tiles each way: the last row and column of tiles are partly outside the image."""
    monkeypatch.setenv("INSTAG_BLEND_FWD", kernel)
    a, settings = make_scene(6000, 200, sh_degree=1, seed=0)
    for aux in (False, True):
        for use_sh in (True, False):
            full = _call(a, settings, True, aux, use_sh=use_sh)[0]
            col = _call(a, settings, False, aux, use_sh=use_sh)[0]
            _same(full, col, aux, f"aux={aux} sh={use_sh}")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["tile", "segment"])
def test_colour_only_empty_scene(kernel, monkeypatch):
    """Every Gaussian behind the camera: no instance at all -- background image, zero alpha, zero gradients, and the same
    again in capacity mode."""
    from instag_amd import diff_gauss
    monkeypatch.setenv("INSTAG_BLEND_FWD", kernel)
    a, settings = make_scene(500, 100, sh_degree=1)
    a["means3D"] = a["means3D"] + torch.tensor([0.0, 0.0, 5.0])
    for capacity in (False, True):
        if capacity:
            diff_gauss.set_capacity_plan(diff_gauss.CapacityPlan([4096, 4096], "cuda"))
        try:
            full = _call(a, settings, True, True)[0]
            col = _call(a, settings, False, True)[0]
        finally:
            diff_gauss.set_capacity_plan(None)
        _same(full, col, True, f"capacity={capacity}")
        bg = settings["bg"].cuda()[:, None, None]
        assert torch.equal(col["outs"][0], bg.expand_as(col["outs"][0])) and float(col["outs"][3].detach().abs().max()) == 0.0
        assert int(col["outs"][4].sum()) == 0 and float(col["grads"]["means3D"].abs().max()) == 0.0


@pytest.mark.gpu
def test_colour_only_image_against_the_oracle():
    """The colour-only image and alpha against oracle/rasterize_ref.py, at the bar of the full forward (<= 1e-4)."""
    from instag_amd.diff_gauss import GaussianRasterizer
    from oracle import rasterize_ref as R
    n, size = 3000, 128
    a, settings = make_scene(n, size, sh_degree=2, seed=3)
    outs_o = R.rasterize(a["means3D"], torch.zeros(n, 3), a["shs"], None, a["opacities"], a["scales"], a["rotations"],
                         None, a["extra"], oracle_settings(settings))
    g = {k: v.cuda() for k, v in a.items()}
    with torch.no_grad():
        outs = GaussianRasterizer(hip_settings(settings))(
            means3D=g["means3D"], means2D=torch.zeros(n, 3, device="cuda"), shs=g["shs"], opacities=g["opacities"],
            scales=g["scales"], rotations=g["rotations"], extra_attrs=g["extra"], geometry=False)
    assert outs[1] is None and outs[2] is None and outs[5] is None
    for i, name in ((0, "image"), (3, "alpha")):
        err = float((outs[i].cpu() - outs_o[i].detach()).abs().max())
        print(f"colour-only {name}: max abs error against the oracle {err:.3e}")
        assert err <= 1e-4, (name, err)
    assert torch.equal(outs[4].cpu(), outs_o[4])


@pytest.mark.gpu
def test_depth_gradient_over_colour_only_state_raises():
    """A backward that asks for a depth gradient over a colour-only state is refused, by the C call itself
    (INSTAG_E_ARG and a message), not answered with numbers."""
    import ctypes as C
    from instag_amd import _lib, diff_gauss
    from instag_amd._lib import ptr
    n, size = 2000, 96
    a, settings = make_scene(n, size, sh_degree=1, seed=5)
    g = {k: v.cuda() for k, v in a.items()}
    outs, st = diff_gauss.rasterize_forward(hip_settings(settings), g["means3D"], g["shs"], None, g["opacities"],
                                            g["scales"], g["rotations"], None, g["extra"], geometry=False)
    assert outs[1] is None and outs[2] is None and st.geometry is False
    want = dict(means3D=True, means2D=True, shs=True, colors=False, opacities=True, scales=True, rotations=True,
                cov3D=False, extra=False)
    g_color = torch.ones(3, size, size, device="cuda")
    g_depth = torch.ones(1, size, size, device="cuda")
    # the Python layer refuses first
    with pytest.raises(RuntimeError, match="colour-only"):
        diff_gauss.rasterize_backward(st, g_color, g_depth, None, None, None, want)
    # and so does the library when it is called directly
    L = _lib.lib()
    ws = torch.empty(L.instag_raster_backward_workspace_bytes(n, st.R), dtype=torch.uint8, device="cuda")
    d_m3 = torch.empty(n, 3, device="cuda")
    rc = L.instag_raster_backward(C.byref(st.args), ptr(st.geom), st.geom.numel(), ptr(st.binning), st.binning.numel(),
                                  ptr(st.image), st.image.numel(), st.R, ptr(st.radii), ptr(g_color), ptr(g_depth),
                                  None, None, None, ptr(ws), ws.numel(), ptr(d_m3), None, None, None, None, None,
                                  None, None, None, None, None, None, None, 0, _lib.current_stream())
    assert rc != 0
    assert "colour-only" in L.instag_last_error().decode()
    # the rgb-only backward over the same state still works
    out = diff_gauss.rasterize_backward(st, g_color, None, None, None, None, want)
    assert bool(torch.isfinite(out["means3D"]).all()) and float(out["means3D"].abs().max()) > 0
    # a forward with only one of depth / normal is an argument error
    color = torch.empty(3, size, size, device="cuda")
    alpha = torch.empty(1, size, size, device="cuda")
    rc = L.instag_raster_forward_stage2(C.byref(st.args), ptr(st.geom), st.geom.numel(), ptr(st.binning),
                                        st.binning.numel(), ptr(st.image), st.image.numel(), st.R, ptr(color),
                                        ptr(g_depth), None, ptr(alpha), None, None, None, _lib.current_stream())
    assert rc != 0 and "go together" in L.instag_last_error().decode()


def test_face_trainer_asks_for_geometry_exactly_in_the_priors_phase(monkeypatch):
    """CPU: FaceTrainer's forward passes need_geometry = phase.priors to render_motion, in the plain step and in the
    three-segment one."""
    from instag_amd import renderer
    from instag_amd.train import FacePhase, FaceTrainer, face_phase

    class Asked(Exception):
        pass

    def stub(*args, **kwargs):
        raise Asked(kwargs.get("need_geometry", "not passed"))

    monkeypatch.setattr(renderer, "render_motion", stub)
    tr = FaceTrainer.__new__(FaceTrainer)          # (the forward reads nothing of the trainer before the call)
    tr.g = tr.motion_net = tr.bg = None
    tr.on_gpu = True
    phases = [FacePhase(), FacePhase(align=False, warm=False), face_phase(5001), face_phase(6050),
              FacePhase(priors=True, prior_depth=True)]
    assert [p.priors for p in phases] == [False, False, True, True, True]
    for phase in phases:
        for step in (tr._forward_backward, tr._forward_backward_cut):
            with pytest.raises(Asked) as e:
                step(None, phase)
            assert e.value.args[0] is phase.priors, (phase, step.__name__)
