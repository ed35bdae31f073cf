"""Host tests of the Sapiens normal / depth chain (instag_amd/sapiens.py): the torch statement against golden G21, the
8-bit resize on hand-computed pixels and against the slow loop statement, the state-dict walk with every refusal, the
finish against ``F.interpolate``, the conditions the GPU tests put on their own inputs, an identity directory through
``geometry_identity`` and ``read_identity`` (files and ``priors=``), and the C entries' argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from instag_amd import sapiens as S
from tests import sapiens_helpers as G


# ---- the statement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "depth"])
def test_statement_matches_g21(golden_dir, kind):
    g21 = np.load(f"{golden_dir}/g21_sapiens.npz")
    w = G.weights("T", kind, int(g21["weights_seed"]))
    frame = G.frames_of(1, *G.G21_FRAME, int(g21["frame_seed"]))
    want = torch.from_numpy(g21[kind])
    got = S.sapiens_torch(w, frame, kind, dtype=torch.float64)[0]
    assert tuple(got.shape) == ((3,) + G.G21_FRAME if kind == "normal" else G.G21_FRAME) and got.dtype == torch.float64
    err, scale = G.relative(got, want)
    print(f"g21 {kind}: fp64 statement {err:.3e} scale {scale:.3e}")
    assert err < 1e-12
    e32, _ = G.relative(S.sapiens_torch(w, frame, kind)[0], want)
    assert G.E32_WINDOW[0] < e32 < G.E32_WINDOW[1], e32
    if kind == "normal":                       # unit vectors up to the 1e-5 in the denominator: 1 - 1e-5 / |n|, |n| > 1e-3
        assert float((want.pow(2).sum(0).sqrt() - 1).abs().max()) < 1e-2


@pytest.mark.parametrize("name,kind,B,H,W", [("T", "normal", 2, 40, 56), ("T", "depth", 1, 64, 48), ("U", "depth", 2, 50, 38)])
def test_every_stage_of_the_test_configs_has_its_e32_in_the_window(name, kind, B, H, W):
    """The gains of tests/sapiens_helpers.py: no stage is dead, constant or beyond fp32's reach."""
    case = G.case(name, kind, B, H, W)
    assert list(case.taps)[0] == "tokens" and list(case.taps)[-1] == "out"
    for stage, want in case.taps.items():
        e, scale = case.e32(stage)
        print(f"{name} {kind} {stage}: e32 {e:.3e} scale {scale:.3e}")
        assert scale > 0.1 and float(want.std()) > 0.02 * scale, stage
    for b in range(B):
        case.e32("out", slice(b, b + 1))
    if B > 1:
        assert not torch.equal(case.want[0], case.want[1])


# ---- the 8-bit resize -----------------------------------------------------------------------------------------------------
def test_resize_on_hand_computed_pixels():
    f = torch.zeros(1, 2, 2, 3, dtype=torch.uint8)
    f[0, :, :, 0] = torch.tensor([[0, 100], [200, 255]])
    f[0, :, :, 1] = 255
    f[0, :, :, 2] = torch.tensor([[10, 20], [30, 40]])
    # an upscale 2 x 2 -> 4 x 4: centres at -1/4 (clamped: pixel 0), 1/4, 3/4 (weights 512 and 1536 of 2048) and 5/4
    # (at the last pixel: clamped)
    up = S.resize_u8_torch(f, (4, 4))[0]
    assert up[:, :, 1].eq(255).all()
    assert up[0, :, 0].tolist() == [0, 25, 75, 100] and up[3, :, 0].tolist() == [200, 214, 241, 255]
    assert up[:, 0, 0].tolist() == [0, 50, 150, 200]
    # the interior pixel (1, 1): (1536 (1536 * 0 + 512 * 100) + 512 (1536 * 200 + 512 * 255) + 2^21) >> 22 = 72.19 -> 72
    assert int(up[1, 1, 0]) == (1536 * 512 * 100 + 512 * (1536 * 200 + 512 * 255) + 2 ** 21) >> 22 == 72
    # rounding half up: (10, 20, 30, 40) at (3/4, 3/4) is (10 + 60 + 90 + 360) / 16 = 32.5 -> 33; at (1/4, 1/4)
    # (90 + 60 + 90 + 40) / 16 = 17.5 -> 18
    assert int(up[2, 2, 2]) == 33 and int(up[1, 1, 2]) == 18
    # a downscale 4 -> 2 along x: centres at 1/2 and 5/2: the means of pixels (0, 1) and (2, 3), halves rounded up
    row = torch.tensor([10, 21, 200, 100], dtype=torch.uint8).view(1, 1, 4, 1).expand(1, 2, 4, 3).contiguous()
    down = S.resize_u8_torch(row, (2, 2))[0]
    assert down[0, :, 0].tolist() == [16, 150] and down[1, :, 2].tolist() == [16, 150]
    # a border: 3 -> 5, the centres -1/5 and 11/5 fall outside [0, 2] and take the edge pixels unchanged
    edge = torch.tensor([7, 100, 250], dtype=torch.uint8).view(1, 3, 1, 1).expand(1, 3, 3, 3).contiguous()
    assert S.resize_u8_torch(edge, (5, 3))[0, :, 0, 0].tolist() == [7, 44, 100, 190, 250]
    # the network's own size passes unchanged
    same = G.frames_of(1, 12, 9, 3)
    assert torch.equal(S.resize_u8_torch(same, (12, 9)), same)


@pytest.mark.parametrize("src,size", G.PATCH_ROWS_CASES)
def test_patch_rows_are_the_loop_statement(src, size):
    frames = G.frames_of(2, *src, seed=src[0])
    for dtype in (torch.float32, torch.float64):
        got, want = S.patch_rows_torch(frames, size, dtype), G.slow_patch_rows(frames, size, dtype)
        assert got.dtype == dtype and tuple(got.shape) == (2, (size[0] // 16) * (size[1] // 16), 768)
        assert torch.equal(got, want)
    # the padding of 2: the first two rows and columns of the first token are zeros, nothing else of it is
    first = got[0, 0].view(3, 16, 16)
    assert float(first[:, :2].abs().max()) == 0 and float(first[:, :, :2].abs().max()) == 0
    assert bool((first[:, 2:, 2:] != 0).any())


# ---- the state-dict walk ----------------------------------------------------------------------------------------------------
def test_the_head_is_read_from_the_shapes():
    t, u = G.weights("T", "normal"), G.weights("U", "depth")
    assert (t.hidden, t.heads, t.intermediate, t.layers, t.grid, t.in_size) == (128, 2, 256, 2, (4, 3), (64, 48))
    assert (t.deconv, t.conv, t.out_channels, t.kind, t.map_size) == ([64, 32, 32, 32], [32], 3, "normal", (64, 48))
    assert t.deconv_affine == [False] * 4 and t.conv_affine == [False]
    assert (u.hidden, u.heads, u.layers, u.in_size, u.deconv, u.conv, u.out_channels, u.kind) == \
        (64, 1, 1, (80, 48), [32], [32, 32], 1, "depth")
    assert all(u.deconv_affine) and all(u.conv_affine) and u.map_size == (10, 6)
    # through a state dict and an mmengine checkpoint, bit for bit; keys outside the network are ignored
    sd = u.state_dict()
    again = S.SapiensWeights.from_state_dict({"meta": {}, "state_dict": dict(sd, **{"data_preprocessor.mean": torch.zeros(3)})},
                                             grid=(5, 3))
    assert set(again.state_dict()) == set(sd) and all(torch.equal(again.tensors[k], v) for k, v in sd.items())
    assert S.macs_per_frame(u, 50, 38) == 15 * 768 * 64 + 15 * (4 * 64 * 64 + 2 * 64 * 128 + 2 * 15 * 64) \
        + 60 * 4 * 64 * 32 + 60 * 32 * 32 * 2 + 60 * 32
    with pytest.raises(ValueError, match="kind 'depth' has 1 channels"):
        S.sapiens_torch(t, G.frames_of(1, 20, 20, 1), "depth")


def test_load_reads_a_saved_state_dict_and_a_checkpoint(tmp_path):
    u = G.weights("U", "depth")
    torch.save(u.state_dict(), tmp_path / "plain.pth")
    torch.save({"meta": {"epoch": 1}, "state_dict": u.state_dict()}, tmp_path / "ckpt.pth")
    for name in ("plain.pth", "ckpt.pth"):
        w = S.SapiensWeights.load(tmp_path / name, grid=(5, 3))
        assert all(torch.equal(w.tensors[k], v) for k, v in u.tensors.items())


def _refused(sd, match, **kw):
    with pytest.raises(ValueError, match=match):
        S.SapiensWeights.from_state_dict(sd, **{"grid": (4, 3), **kw})


def test_every_refusal_names_its_key_or_field():
    base = G.weights("T", "normal").state_dict()
    sd = dict(base)
    sd["decode_head.deconv_layers.3.weight"] = torch.zeros(64, 32, 3, 3)
    _refused(sd, r"decode_head\.deconv_layers\.3\.weight.*only 4 x 4")
    sd = dict(base)
    sd["decode_head.conv_layers.0.weight"] = torch.zeros(32, 32, 3, 3)
    _refused(sd, r"decode_head\.conv_layers\.0\.weight.*only 1 x 1")
    sd = dict(base)
    sd["decode_head.deconv_layers.9.weight"] = torch.zeros(32, 48, 4, 4)
    _refused(sd, r"decode_head\.deconv_layers\.9\.weight.*width of 48")
    sd = dict(base)
    sd["decode_head.deconv_layers.0.bias"] = torch.zeros(64)
    _refused(sd, r"decode_head\.deconv_layers\.0\.bias.*no bias")
    sd = dict(base)
    sd["decode_head.deconv_layers.1.running_mean"] = torch.zeros(64)
    _refused(sd, r"decode_head\.deconv_layers\.1\.running_mean")
    _refused(base, r"heads = 4.*hidden / heads must be 64", heads=4)
    big = {k: v for k, v in base.items()}
    big["backbone.patch_embed.projection.weight"] = torch.zeros(1280, 3, 16, 16)
    _refused(big, r"backbone\.patch_embed\.projection\.weight.*hidden = 1280.*at most 1024")
    sd = dict(base)
    sd["backbone.pos_embed"] = torch.zeros(1, 13, 128)
    _refused(sd, r"backbone\.pos_embed.*\(1, 13, 128\).*\(1, 12, 128\).*class token")
    _refused(base, r"backbone\.pos_embed.*expected \(1, 3072, 128\) for grid = \(64, 48\)", grid=(64, 48))
    sd = dict(base)
    sd["backbone.layers.1.gamma_1"] = torch.ones(128)
    _refused(sd, r"backbone\.layers\.1\.gamma_1.*unknown tensor under backbone\.layers")
    sd = {k: v for k, v in base.items() if k != "backbone.layers.1.attn.proj.bias"}
    _refused(sd, r"misses 'backbone\.layers\.1\.attn\.proj\.bias'")
    sd = dict(base)
    sd["backbone.layers.0.attn.qkv.weight"] = torch.zeros(384, 64)
    _refused(sd, r"backbone\.layers\.0\.attn\.qkv\.weight.*\(384, 64\).*\(384, 128\)")
    sd = dict(base)
    sd["decode_head.conv_seg.weight"] = torch.zeros(2, 32, 1, 1)
    _refused(sd, r"decode_head\.conv_seg\.weight")
    with pytest.raises(ValueError, match="kind 'depth' has 1 channels"):
        S.GeometryNet(G.weights("T", "normal"), "cpu", kind="depth")
    with pytest.raises(ValueError, match="max_batch >= 1"):
        S.GeometryNet(G.weights("T", "normal"), "cpu", max_batch=0)


# ---- the finish -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,h,w,H,W", [(3, 10, 6, 25, 31), (1, 10, 6, 7, 5), (3, 8, 8, 8, 8), (1, 4, 3, 40, 56)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_finish_is_interpolate_and_the_reference_normalisation(C_, h, w, H, W, dtype):
    raw = torch.randn(2, C_, h, w, generator=torch.Generator().manual_seed(h * W), dtype=dtype)
    want = F.interpolate(raw, size=(H, W), mode="bilinear", align_corners=False)
    if C_ == 3:
        want = want / (torch.linalg.norm(want, dim=1, keepdim=True) + 1e-5)
    else:
        want = want[:, 0]
    got = S.finish_torch(raw, H, W)
    assert got.dtype == dtype and tuple(got.shape) == tuple(want.shape)
    # (two orders of the same four products; a short normal magnifies their rounding by 1 / |n|, here up to about 100)
    assert float((got - want).abs().max()) <= (2e-5 if dtype == torch.float32 else 1e-13)


# ---- the stage tests' own inputs ---------------------------------------------------------------------------------------------
def test_stage_cases_meet_their_conditions():
    for T, heads, B in G.ATTENTION_SHAPES:
        G.attention_case(T, heads, B).check_inputs()
    c = G.crafted_attention()
    c.e32()
    s, probs, r = c.scores[0, 0], torch.softmax(c.scores, dim=-1), c.rows
    assert int(s[r["rising"]].argmax()) == c.T - 1 and bool((s[r["rising"]].diff() > 0).all())
    assert int(s[r["first"]].argmax()) == 0 and float(probs[0, 0, r["first"], 0]) > 0.85      # e^10 / (e^10 + 3071)
    assert float(s[r["equal"]].abs().max()) == 0.0
    assert 99.0 < float(s[r["huge"]].max()) < 101.0 and -101.0 < float(s[r["huge"]].min()) < -99.0
    assert int(s[r["spike"]].argmax()) == c.spike_key == 3008 and float(probs[0, 0, r["spike"], c.spike_key]) > 0.8
    for shape in G.DECONV_SHAPES:
        G.deconv_case(*shape).e32()
    imp = G.impulse_case()
    assert int((imp.want[:, 0] != 0).sum()) == 4 * 9 + 12 + 16       # corners reach 3 x 3 outputs, the edge 3 x 4, the centre 4 x 4
    for (h, w) in G.NORM_MAPS:
        for affine in (False, True):
            n = G.norm_case(h, w, affine)
            n.e32()
            n.e32(slice(G.OFFSET_CHANNEL, G.OFFSET_CHANNEL + 1))
            const = n.want[:, G.CONSTANT_CHANNEL]
            # (torch's mean of a constant is a rounding off it; the kernel's fp64 sum of a constant is exact)
            assert float(const.max() - const.min()) < 1e-12 and (affine or float(const.abs().max()) < 1e-12)


# ---- an identity directory -----------------------------------------------------------------------------------------------------
def test_geometry_identity_writes_what_read_identity_loads(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from instag_amd import dataset as DS
    from tests import dataset_helpers as D
    root, a = str(tmp_path), D.make_arrays()
    D.write_identity(root, a)
    ids_all = D.TRAIN_IDS + D.VAL_IDS
    for j, i in enumerate(ids_all):            # lossless data under the name the reference opens, as bc.jpg above
        Image.fromarray(a["gt"][j], "RGB").save(f"{root}/gt_imgs/{i}.jpg", format="PNG")
    Image.fromarray(a["gt"][0], "RGB").save(f"{root}/gt_imgs/notes.jpg", format="PNG")       # not a frame: skipped
    nw, dw = G.weights("T", "normal"), G.weights("U", "depth")
    ids, normal, depth = S.geometry_identity(root, nw, dw, "cpu", limit=4, model_name="sapiens_z", batch=3)
    assert ids.tolist() == [0, 1, 2, 3] and tuple(normal.shape) == (4, 3, D.H, D.W) and tuple(depth.shape) == (4, D.H, D.W)
    frames = torch.from_numpy(a["gt"][:4])
    # (the right frames in the right order: the statement on all four at once differs from the chunks of three by the
    # CPU library's batch-dependent rounding alone)
    assert float((normal - S.sapiens_torch(nw, frames, "normal")).abs().max()) < 1e-3
    assert float((depth - S.sapiens_torch(dw, frames)).abs().max()) < 1e-3 * float(depth.abs().max())
    on_disk = np.load(f"{root}/sapiens/normal/sapiens_z/2.npy")
    assert on_disk.shape == (D.H, D.W, 3) and on_disk.dtype == np.float32
    assert np.load(f"{root}/sapiens/depth/sapiens_z/2.npy").shape == (D.H, D.W)
    kw = dict(n_views=2, extension=".png")
    d = DS.read_identity(root, "train", **kw)                     # sapiens_z is the latest folder
    assert d["meta"]["img_id"].tolist() == [0, 1]
    assert np.array_equal(d["normal"], normal[:2].numpy()) and np.array_equal(d["depth"], depth[:2].numpy())
    # the priors= route: the same arrays, and the same store contents
    pri = dict(ids=ids, normal=normal, depth=depth)
    p = DS.read_identity(root, "train", priors=pri, **kw)
    assert torch.equal(torch.as_tensor(p["normal"]), normal[:2]) and torch.equal(torch.as_tensor(p["depth"]), depth[:2])
    from_files, _ = DS.open_identity(root, "train", "cpu", **kw)
    from_priors, _ = DS.open_identity(root, "train", "cpu", priors=pri, **kw)
    assert len(from_files) == len(from_priors) == 2
    for i in range(2):
        u, v = from_files.unpack_torch(i, priors=True), from_priors.unpack_torch(i, priors=True)
        assert set(u) == set(v)
        for k in u:
            assert torch.equal(torch.as_tensor(u[k]), torch.as_tensor(v[k])), k
        assert torch.equal(v["normal"], normal[i]) and torch.equal(v["depth"], depth[i])
    # with None nothing changes; an uncovered id is a KeyError naming it; one network only gives one tree
    assert np.array_equal(DS.read_identity(root, "train", priors=None, **kw)["normal"], d["normal"])
    with pytest.raises(KeyError, match="train frame 4"):
        DS.read_identity(root, "train", priors=pri, n_views=5, extension=".png")
    with pytest.raises(ValueError, match="normal and depth come together"):
        DS.read_identity(root, "train", priors=dict(ids=ids, normal=normal, depth=None), **kw)
    ids1, n1, d1 = S.geometry_identity(root, None, dw, "cpu", limit=2, write=False)
    assert ids1.tolist() == [0, 1] and n1 is None and float((d1 - depth[:2]).abs().max()) < 1e-3 * float(depth.abs().max())
    assert DS.read_identity(root, "val", priors=pri, extension=".png").get("normal") is None


# ---- the C entries without a GPU --------------------------------------------------------------------------------------------
def test_argument_errors_of_the_c_entries():
    from instag_amd import _lib
    L, E = _lib.lib(), _lib.E_ARG
    err = lambda: L.instag_last_error().decode()                     # noqa: E731
    assert _lib.SAPIENS["INSTAG_SAPIENS_MAX_TOKENS"] == 4096 and _lib.SAPIENS["INSTAG_SAPIENS_MAX_LAYERS"] == 48
    t = G.weights("T", "normal")
    s = t.fill_dims(_lib.SapiensStruct())
    one = L.instag_sapiens_workspace_bytes(C.byref(s), 1)
    assert one > 0 and L.instag_sapiens_workspace_bytes(C.byref(s), 3) > 2 * one
    # the features, then the larger of the backbone's pieces and the head's: its two largest maps (64 x 48 x 32 both), raw
    # and the fp64 sums of 3 chunks x 64 channels and of 64 channels (every piece here is a multiple of 64 floats)
    T_, hid = 12, 128
    backbone = T_ * (768 + 3 * hid + 3 * hid + 256)
    head = 2 * 64 * 48 * 32 + 64 * 48 * 4 + 3 * 64 * 4 + 64 * 4
    assert one == 4 * (T_ * hid + max(backbone, head))
    taps = L.instag_sapiens_taps_floats(C.byref(s), 2)
    assert taps == 2 * ((2 + 4) * T_ * hid + 8 * 6 * 64 + 16 * 12 * 32 + 32 * 24 * 32 + 2 * 64 * 48 * 32 + 64 * 48 * 4)

    def refused(match, **fields):
        bad = t.fill_dims(_lib.SapiensStruct())
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(bad, k)[v[0]] = v[1]
            else:
                setattr(bad, k, v)
        assert L.instag_sapiens_workspace_bytes(C.byref(bad), 1) == 0 and match in err(), (match, err())
        assert L.instag_sapiens_taps_floats(C.byref(bad), 1) == 0
        assert L.instag_sapiens_forward(C.byref(bad), None, 1, 8, 8, 0, None, None, None, None, 0, 0, None, None) == E

    refused("hidden / heads must be 64", heads=3)
    refused("hidden must be at most 1024", hidden=1280, heads=20)
    refused("intermediate", intermediate=100)
    refused("INSTAG_SAPIENS_MAX_LAYERS", layers=49)
    refused("INSTAG_SAPIENS_MAX_TOKENS", in_h=1040, in_w=1024)              # 65 x 64 = 4160 tokens
    refused("deconv width", deconv_c=(1, 48))
    refused("conv width", conv_c=(0, 8192))
    refused("n_deconv", n_deconv=0)
    refused("out_channels", out_channels=2)
    refused("std must be positive", std=(1, 0.0))
    assert L.instag_sapiens_workspace_bytes(C.byref(s), 0) == 0 and "batch" in err()
    assert L.instag_sapiens_workspace_bytes(None, 1) == 0 and "NULL weights" in err()
    # forward: a refused tensor, mode, size or tile comes before the weights and the workspace
    p = C.c_void_p(4096)                                            # never read: every call below is refused first
    fwd = lambda *a: L.instag_sapiens_forward(C.byref(s), *a)       # noqa: E731
    assert fwd(None, 1, 8, 8, 0, p, None, None, p, 1 << 30, 0, None, None) == E and "NULL tensor" in err()
    assert fwd(p, 1, 8, 8, 3, p, None, None, p, 1 << 30, 0, None, None) == E and "mode" in err()
    assert fwd(p, 1, 8, 8, 2, p, None, None, p, 1 << 30, 0, None, None) == E and "NULL tensor" in err()
    assert fwd(p, 1, 0, 8, 0, p, None, None, p, 1 << 30, 0, None, None) == E and "H and W" in err()
    assert fwd(p, 1, 8, 8, 0, p, None, None, p, 1 << 30, 4, None, None) == E and "tile" in err()
    assert fwd(p, 1, 8, 8, 1, None, None, p, p, 1 << 30, 0, p, None) == E and "taps go with mode 0" in err()
    assert fwd(p, 1, 8, 8, 0, p, C.c_void_p(4100), None, p, 1 << 30, 0, None, None) == E and "16-byte" in err()
    assert fwd(p, 1, 8, 8, 0, p, None, None, p, 1 << 30, 0, None, None) == E and "NULL weight" in err()
    # the stages
    three = (C.c_float * 3)(1, 1, 1)
    assert L.instag_sapiens_patch_rows(None, 1, 8, 8, 64, 48, three, three, p, None) == E and "NULL tensor" in err()
    assert L.instag_sapiens_patch_rows(p, 1, 8, 8, 11, 48, three, three, p, None) == E and "in_h and in_w" in err()
    assert L.instag_sapiens_patch_rows(p, 1, 0, 8, 64, 48, three, three, p, None) == E and "H and W" in err()
    assert L.instag_sapiens_patch_rows(p, 1, 8, 8, 64, 48, three, (C.c_float * 3)(1, 0, 1), p, None) == E and "std" in err()
    assert L.instag_sapiens_attention(p, p, 1, 4097, 1, None) == E and "INSTAG_SAPIENS_MAX_TOKENS" in err()
    assert L.instag_sapiens_attention(p, p, 1, 0, 1, None) == E
    assert L.instag_sapiens_attention(p, C.c_void_p(4100), 1, 8, 1, None) == E and "16-byte" in err()
    assert L.instag_sapiens_attention(None, p, 1, 8, 1, None) == E and "NULL tensor" in err()
    assert L.instag_sapiens_deconv_workspace_bytes(1, 3, 5, 32, 48) == 0 and "multiples of 32" in err()
    need = L.instag_sapiens_deconv_workspace_bytes(2, 3, 5, 32, 64)
    assert need == 4 * (2 * 5 * 7 * 32 + 64)
    assert L.instag_sapiens_deconv(p, p, p, 2, 3, 5, 32, 64, p, need, 5, None) == E and "tile" in err()
    assert L.instag_sapiens_deconv(p, p, p, 2, 3, 5, 40, 64, p, need, 0, None) == E and "multiples of 32" in err()
    assert L.instag_sapiens_deconv(p, None, p, 2, 3, 5, 32, 64, p, need, 0, None) == E and "NULL tensor" in err()
    assert L.instag_sapiens_deconv(p, p, p, 2, 3, 5, 32, 64, p, need - 1, 0, None) == _lib._CONSTANTS["INSTAG_E_SPACE"]
    assert L.instag_sapiens_norm_workspace_bytes(1, 0, 5, 32) == 0
    need = L.instag_sapiens_norm_workspace_bytes(3, 64, 48, 32)
    assert need == 4 * (3 * 3 * 32 * 4 + 3 * 32 * 4)
    assert L.instag_sapiens_instance_norm_silu(p, 3, 64, 48, 32, p, None, p, need, None) == E and "both or neither" in err()
    assert L.instag_sapiens_instance_norm_silu(None, 3, 64, 48, 32, None, None, p, need, None) == E
    assert L.instag_sapiens_instance_norm_silu(p, 3, 64, 48, 5000, None, None, p, need, None) == E and "channels" in err()
    assert L.instag_sapiens_instance_norm_silu(p, 3, 64, 48, 32, None, None, p, need - 1, None) == _lib._CONSTANTS["INSTAG_E_SPACE"]
    assert L.instag_sapiens_finish(p, 1, 4, 4, 2, 8, 8, p, None) == E and "channels must be 1 or 3" in err()
    assert L.instag_sapiens_finish(p, 1, 4, 4, 3, 0, 8, p, None) == E
    assert L.instag_sapiens_finish(None, 1, 4, 4, 3, 8, 8, p, None) == E and "NULL tensor" in err()
