"""GPU tests of the Sapiens normal / depth operator (csrc/sapiens.hip): every stage's kernel alone through its own entry
-- the patch rows bit for bit against the loop statement, the attention at the lengths that take another path and on
crafted rows at 3072 tokens, the transposed convolution on impulses and seeded maps, InstanceNorm + SiLU on a constant
channel, a channel with a large mean, with and without gain -- then the network against golden G21 and the fp64 CPU
statement, every stage through the debug taps, batch, chunk, tile and call independence bit for bit, the kept
workspace, the token bound, and an identity directory against the CPU route.

Tolerance: that of test_hubert_gpu.py.  e32 = max|fp32 torch statement on the CPU - fp64| / max|fp64| is measured on
each test's own inputs and must lie in (1e-8, 1e-4); the operator must be within 8 x e32 of the fp64 result (relative
to its largest entry).  Where the result is exact in any precision (one key, an impulse, a constant channel) e32 is 0
and the operator has to be exact.  Every test prints the operator's error beside e32 and the bar before it asserts.
The conditions on the inputs are tests/test_sapiens_host.py's, on the same cached cases.

Observed on an MI355X (profiles/sapiens_parity.json).  Patch rows: equal to the loop statement on all 18,432 / 18,432 /
23,040 values.  Attention alone: e32 5.4e-7 .. 9.4e-7, operator 4.4e-7 .. 1.4e-6, 0.8 .. 1.5 x e32 (the largest at
T = 3072); one key exact; the crafted rows at T = 3072 at 0.7 .. 4.2 x their own row's e32 (rising 0.9, first 0.7, equal
4.2, huge 3.8, spike 1.2).  Deconv: the 64 impulse outputs placed and exact; seeded maps 1.0 .. 1.1 x e32.  InstanceNorm +
SiLU: 7.5e-8 .. 1.4e-7 against an e32 of 4.3e-6 .. 1.7e-5 (0.01 .. 0.02 x: the fp64 sums), the channel with a mean of 100
at 0.02 .. 0.09 x.  Finish: 1.0 x.  Network: G21 normal e32 1.8e-5, operator 2.1e-5 (1.2 x; short normals magnify both),
depth 2.3e-6 / 3.0e-6 (1.3 x); stage by stage T at 0.8 .. 3.0 x and U at 1.1 .. 2.5 x the stage's own e32 (the largest:
the embedded tokens, whose K = 768 sum is one chain); the chunked call 0.5 x; an identity directory differs from the CPU
route by 1.3e-5 (normal, bound 1.5e-4) and 1.8e-6 (depth, bound 1.2e-5).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sapiens_helpers as G

pytestmark = pytest.mark.gpu

FACTOR = 8.0
GUARD = 4096


def _check(name, got, want, e32, scale):
    err = float((got.detach().double().cpu() - want).abs().max()) / scale
    print(f"{name}: operator {err:.3e} e32 {e32:.3e} bar {FACTOR * e32:.3e} scale {scale:.3e} ratio {err / max(e32, 1e-30):.2f}")
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    assert err <= FACTOR * e32, (name, err, e32)


# ---- the front end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,size", G.PATCH_ROWS_CASES)
def test_patch_rows_equal_the_loop_statement(src, size):
    from instag_amd import sapiens as S
    frames = G.frames_of(2, *src, seed=src[0])
    want = G.slow_patch_rows(frames, size)
    got = S.patch_rows(frames.cuda(), size)
    diff = float((got.cpu() - want).abs().max())
    print(f"patch_rows {src} -> {size}: max difference {diff:.3e} over {want.numel()} values")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(S.patch_rows(frames[1:].cuda(), size)[0], got[1])


# ---- the attention ---------------------------------------------------------------------------------------------------------
def _attention_with_guards(case):
    from instag_amd import _lib
    qkv = case.qkv.cuda()
    before = qkv.clone()
    B, T, H = case.B, case.T, 64 * case.heads
    buf = torch.full((GUARD + B * T * H + GUARD,), -7.25, dtype=torch.float32, device="cuda")
    ctx = buf[GUARD:GUARD + B * T * H].view(B, T, H)
    _lib.check_arg(_lib.lib().instag_sapiens_attention(_lib.ptr(qkv), _lib.ptr(ctx), B, T, case.heads, _lib.current_stream()),
                   "sapiens_attention")
    torch.cuda.synchronize()
    assert torch.equal(qkv, before)
    assert bool((buf[:GUARD] == -7.25).all()) and bool((buf[GUARD + B * T * H:] == -7.25).all())
    return ctx


@pytest.mark.parametrize("T,heads,B", G.ATTENTION_SHAPES)
def test_attention_matches_fp64(T, heads, B):
    from instag_amd.sapiens import attention
    case = G.attention_case(T, heads, B)
    e32, scale = case.e32()
    ctx = _attention_with_guards(case)
    _check(f"attention T={T} heads={heads} B={B}", ctx, case.want, e32, scale)
    if T == 1:
        assert torch.equal(ctx.cpu(), case.qkv[:, :, 2 * 64 * heads:])          # one key: the output is v
    assert torch.equal(attention(case.qkv.cuda(), heads), ctx)
    if B == 2:
        assert torch.equal(attention(case.qkv[1:].cuda(), heads)[0], ctx[1])
    if T <= 1024:                                                               # the kernel HuBERT runs: the same bits
        from instag_amd.hubert import attention as hubert_attention
        assert torch.equal(hubert_attention(case.qkv.cuda(), heads), ctx)


def test_attention_crafted_rows_at_3072():
    case = G.crafted_attention(3072)
    e32, scale = case.e32()
    ctx = _attention_with_guards(case)
    _check("crafted T=3072", ctx, case.want, e32, scale)
    for name, r in case.rows.items():
        row_scale = float(case.want[0, r].abs().max())
        row_e32 = max(float((case.got32[0, r] - case.want[0, r]).abs().max()) / row_scale, 2.0 ** -24)
        err = float((ctx[0, r].double().cpu() - case.want[0, r]).abs().max()) / row_scale
        print(f"  {name} (row {r}): operator {err:.3e} row e32 {row_e32:.3e} bar {FACTOR * row_e32:.3e}")
        assert err <= FACTOR * row_e32, (name, err, row_e32)


def test_attention_beyond_the_token_bound_is_an_argument_error():
    from instag_amd.sapiens import attention
    with pytest.raises(ValueError, match="INSTAG_SAPIENS_MAX_TOKENS"):
        attention(torch.zeros(1, 4097, 192, device="cuda"), 1)


# ---- the transposed convolution --------------------------------------------------------------------------------------------
def _deconv(case, tile=0, rows=slice(None)):
    from instag_amd.sapiens import deconv
    y = deconv(case.x[rows].permute(0, 2, 3, 1).contiguous().cuda(), case.weight.cuda(), tile)
    return y.permute(0, 3, 1, 2)


def test_deconv_places_impulses_exactly():
    """A one at a corner, an edge or the centre of a 3 x 5 map under sixteen distinct taps: the outputs that are not zero
    are conv_transpose2d's, and each is a weight itself -- one product with 1 and sums with 0, exact in any precision."""
    case = G.impulse_case()
    got = _deconv(case).cpu()
    assert tuple(got.shape) == (len(G.IMPULSES), 32, 6, 10)
    assert torch.equal(got != 0, case.want != 0)
    assert torch.equal(got.double(), case.want)
    print(f"impulses: {int((got[:, 0] != 0).sum())} outputs of channel 0 placed, all exact")


@pytest.mark.parametrize("h,w,cin,cout", G.DECONV_SHAPES)
def test_deconv_matches_fp64(h, w, cin, cout):
    case = G.deconv_case(h, w, cin, cout)
    e32, scale = case.e32()
    got = _deconv(case)
    _check(f"deconv {h}x{w} {cin}->{cout}", got, case.want, e32, scale)
    assert torch.equal(_deconv(case, rows=slice(1, 2))[0], got[1])              # a frame's bits: not its batch's
    for tile in (1, 2, 3):
        assert torch.equal(_deconv(case, tile), got), tile


# ---- InstanceNorm + SiLU -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("h,w", G.NORM_MAPS)
def test_instance_norm_silu_matches_fp64(h, w, affine):
    from instag_amd.sapiens import instance_norm_silu
    case = G.norm_case(h, w, affine)
    x = case.x.permute(0, 2, 3, 1).contiguous().cuda()
    gb = (case.gamma.cuda(), case.beta.cuda()) if affine else (None, None)
    got = instance_norm_silu(x, *gb).permute(0, 3, 1, 2)
    e32, scale = case.e32()
    _check(f"norm {h}x{w} affine={affine}", got, case.want, e32, scale)
    # a constant channel: exactly 0 in front of the gain, so exactly SiLU(beta) behind it
    const = got[:, G.CONSTANT_CHANNEL].cpu()
    if affine:
        b = case.beta[G.CONSTANT_CHANNEL]
        assert bool((const == const[0, 0, 0]).all()) and abs(float(const[0, 0, 0]) - float(b / (1 + torch.exp(-b)))) < 1e-7
    else:
        assert float(const.abs().max()) == 0.0
    # a mean of 100 beside a spread of 1: within the bar of that channel alone
    ch = slice(G.OFFSET_CHANNEL, G.OFFSET_CHANNEL + 1)
    e32c, scalec = case.e32(ch)
    _check(f"  large mean {h}x{w}", got[:, ch], case.want[:, ch], e32c, scalec)
    # a frame alone and inside a batch of three: the same bits
    alone = instance_norm_silu(x[1:2], *gb).permute(0, 3, 1, 2)
    assert torch.equal(alone[0], got[1])


# ---- the finish ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,h,w,H,W", [(3, 10, 6, 25, 31), (1, 10, 6, 7, 5), (3, 64, 48, 40, 56)])
def test_finish_matches_fp64(Cn, h, w, H, W):
    from instag_amd import sapiens as S
    raw = torch.randn(2, Cn, h, w, generator=torch.Generator().manual_seed(h * W)) + 0.5
    want = S.finish_torch(raw.double(), H, W)
    e32, scale = G.relative(S.finish_torch(raw, H, W), want)
    assert G.E32_WINDOW[0] < e32 < G.E32_WINDOW[1], e32
    nhwc = torch.zeros(2, h, w, 4)
    nhwc[..., :Cn] = raw.permute(0, 2, 3, 1)
    got = S.finish(nhwc.cuda(), Cn, H, W)
    _check(f"finish C={Cn} {h}x{w} -> {H}x{W}", got if Cn == 3 else got[:, 0], want, e32, scale)


# ---- the network -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from instag_amd.sapiens import GeometryNet
    return {(name, kind): GeometryNet(G.weights(name, kind), "cuda", kind)
            for name, kind in (("T", "normal"), ("T", "depth"), ("U", "depth"))}


@pytest.mark.parametrize("kind", ["normal", "depth"])
def test_output_matches_g21(golden_dir, ops, kind):
    from instag_amd import sapiens as S
    g21 = np.load(f"{golden_dir}/g21_sapiens.npz")
    assert int(g21["weights_seed"]) == G.G21_SEED
    frame = G.frames_of(1, *G.G21_FRAME, int(g21["frame_seed"]))
    want = torch.from_numpy(g21[kind])[None]
    e32, scale = G.relative(S.sapiens_torch(G.weights("T", kind), frame, kind), want)
    assert G.E32_WINDOW[0] < e32 < G.E32_WINDOW[1], e32
    got = ops[("T", kind)].predict(frame.cuda())
    assert got.is_cuda and not got.requires_grad
    _check(f"g21 {kind}", got, want, e32, scale)


@pytest.mark.parametrize("name,kind,B,H,W", [("T", "normal", 2, 40, 56), ("T", "depth", 1, 64, 48), ("U", "depth", 2, 50, 38)])
def test_every_stage_matches_fp64(ops, name, kind, B, H, W):
    """The operator's debug taps against the statement's, stage by stage: each within 8 x that stage's own e32."""
    case = G.case(name, kind, B, H, W)
    op = ops[(name, kind)]
    got = []
    out = op.predict(case.frames.cuda(), taps=got)
    assert [k for k, _ in got] == [k for k in case.taps if k != "out"]
    assert torch.equal(out, op.predict(case.frames.cuda()))
    for k, g in got + [("out", out)]:
        e32, scale = case.e32(k)
        _check(f"{name} {kind} {k}", g, case.taps[k], e32, scale)
    e32, scale = case.e32("raw")
    _check(f"{name} {kind} raw()", op.raw(case.frames.cuda()), case.taps["raw"], e32, scale)
    feats = op.features(case.frames.cuda())
    assert torch.equal(feats, dict(got)["features"])
    assert torch.equal(op.head(feats, H, W), out)


def test_bits_do_not_depend_on_call_operator_batch_or_tile():
    """Two calls and a second operator give the same bits; frame b of a chunked call over max_batch + 1 frames
    (max_batch = 2) equals the single-frame call bit for bit; so does every GEMM tile."""
    from instag_amd.sapiens import GeometryNet
    case = G.case("T", "normal", 3, 40, 56)
    w, frames = case.w, case.frames.cuda()
    op = GeometryNet(w, "cuda", max_batch=2)
    first = op.predict(frames).clone()
    assert torch.equal(first, op.predict(frames)) and float(first.abs().max()) > 0
    assert torch.equal(first, GeometryNet(w, "cuda").predict(frames))
    for b in range(3):
        assert torch.equal(op.predict(frames[b:b + 1])[0], first[b]), b
    assert not torch.equal(first[0], first[2])
    for tile in (1, 2, 3):
        assert torch.equal(GeometryNet(w, "cuda", tile=tile).predict(frames), first), tile
    e32, scale = case.e32()
    _check("chunked", first, case.want, e32, scale)


def test_a_smaller_call_keeps_the_workspace():
    from instag_amd.sapiens import GeometryNet
    w = G.weights("U", "depth")
    big, small = G.frames_of(3, 50, 38, seed=5).cuda(), G.frames_of(1, 20, 24, seed=6).cuda()
    op = GeometryNet(w, "cuda", "depth", max_batch=2)
    first = op.predict(big).clone()
    where, size = op._ws.data_ptr(), op._ws.numel()
    second = op.predict(small)
    assert op._ws.data_ptr() == where and op._ws.numel() == size
    assert tuple(first.shape) == (3, 50, 38) and tuple(second.shape) == (1, 20, 24) and float(second.abs().max()) > 0
    assert torch.equal(first, GeometryNet(w, "cuda", "depth", max_batch=2).predict(big))
    assert torch.equal(second, GeometryNet(w, "cuda", "depth").predict(small))


def test_too_many_tokens_is_an_argument_error(ops):
    from instag_amd import _lib
    from instag_amd.sapiens import SapiensWeights
    bound = _lib.SAPIENS["INSTAG_SAPIENS_MAX_TOKENS"]
    sd = G.weights("U", "depth").state_dict()
    sd["backbone.pos_embed"] = torch.zeros(1, 65 * 64, 64)
    with pytest.raises(ValueError, match=f"{65 * 64} tokens, at most {bound}"):
        SapiensWeights.from_state_dict(sd, grid=(65, 64))
    op = ops[("U", "depth")]
    s = _lib.SapiensStruct.from_buffer_copy(op._struct)
    s.in_h, s.in_w = 16 * 65, 16 * 64
    one = torch.full((64,), 3.0, device="cuda")
    frame = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().instag_sapiens_forward(C.byref(s), _lib.ptr(frame), 1, 8, 8, 0, _lib.ptr(one), None, None, _lib.ptr(one),
                                           4 * one.numel(), 0, None, _lib.current_stream())
    assert rc == _lib.E_ARG and "INSTAG_SAPIENS_MAX_TOKENS" in _lib.lib().instag_last_error().decode()
    rc = _lib.lib().instag_sapiens_forward(C.byref(op._struct), _lib.ptr(frame), 1, 8, 8, 0, _lib.ptr(one), None, None,
                                           _lib.ptr(one), 4 * one.numel(), 0, None, _lib.current_stream())
    assert rc == _lib._CONSTANTS["INSTAG_E_SPACE"]                       # a short workspace
    torch.cuda.synchronize()
    assert bool((one == 3.0).all())                                      # nothing was launched


def test_geometry_identity_matches_the_cpu_route(tmp_path):
    """Both networks over four frames of a directory, on the GPU and through the torch statement on the CPU: both are
    within 8 x e32 (the operator, tested above) and e32 (the statement) of the fp64 maps, so they differ by at most
    9 e32 scale per entry."""
    pytest.importorskip("PIL")
    from PIL import Image
    from instag_amd import sapiens as S
    from tests import dataset_helpers as D
    root, a = str(tmp_path), D.make_arrays()
    D.write_identity(root, a)
    for j, i in enumerate(D.TRAIN_IDS + D.VAL_IDS):
        Image.fromarray(a["gt"][j], "RGB").save(f"{root}/gt_imgs/{i}.jpg", format="PNG")
    nw, dw = G.weights("T", "normal"), G.weights("U", "depth")
    ids_g, n_g, d_g = S.geometry_identity(root, nw, dw, "cuda", limit=4, model_name="sapiens_z")
    ids_c, n_c, d_c = S.geometry_identity(root, nw, dw, "cpu", limit=4, write=False)
    assert ids_g.tolist() == ids_c.tolist() == [0, 1, 2, 3] and n_g.is_cuda and d_g.is_cuda
    frames = torch.from_numpy(a["gt"][:4])
    for name, g, c, w in (("normal", n_g, n_c, nw), ("depth", d_g, d_c, dw)):
        e32, scale = G.Case(w, frames).e32()
        diff = float((g.cpu() - c).abs().max())
        print(f"identity {name}: diff {diff:.3e} bound {(FACTOR + 1) * e32 * scale:.3e} (e32 {e32:.3e} scale {scale:.3e})")
        assert diff <= (FACTOR + 1) * e32 * scale and float(c.abs().max()) > 0
    assert np.array_equal(np.load(f"{root}/sapiens/normal/sapiens_z/3.npy"), n_g[3].permute(1, 2, 0).cpu().numpy())
    assert np.array_equal(np.load(f"{root}/sapiens/depth/sapiens_z/0.npy"), d_g[0].cpu().numpy())
