"""GPU: csrc/metrics.hip (frame metrics, inference epilogue) and instag_amd.metrics on top of it, against the fp64
plain-torch statement on the same fp32 inputs.

The bound follows tests/test_lpips_gpu.py: the yardstick of a figure is the error of the fp32 torch statement on the CPU
against the same statement in fp64; the HIP path may be 4x that far from the fp64 value, with a floor of one fp32 unit in
the last place of the value for the cases where the CPU happens to be exact.  (Both paths round the same fp32 pixels;
anything beyond the margin is a defect in the window or the reduction, not rounding.)  For the composed image the
operands are O(1) and every rounding is that of an O(1) term, so the yardstick is the CPU's largest error over the image.

The kernel carries its sums in fp64, so l1 / mse / both PSNR forms are the correctly rounded fp32 of the fp64 statement.
Its SSIM window is the product of two fp32 1-D weights where the statement rounds that product to fp32 (`g @ g.t()`);
a CPU emulation of the kernel's arithmetic on these inputs puts its SSIM 1.1e-8 .. 2.1e-8 (about two fp32 units) from
the fp64 statement, the fp32 CPU statement 3e-9 .. 2.9e-7.  INSTAG_METRICS_PARITY_OUT=<file> records every case's figures.
"""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from instag_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 37, 53), (1, 7, 9), (2, 64, 64), (1, 16, 16)]
_RECORD = {}


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _within(hip, cpu32, ref64):
    """The rule of the module docstring for one figure (python floats)."""
    if math.isinf(ref64) or math.isnan(ref64):
        return hip == ref64 or (math.isnan(ref64) and math.isnan(hip))
    return abs(hip - ref64) <= 4 * abs(cpu32 - ref64) + _ulp32(ref64)


def _pairs(B, H, W):
    """Seeded uniform [-0.1, 1.1] (the clamp matters).  B = 3: [random, pred == gt, constant pred]; B = 2: [random,
    pred == gt]; the 16x16 single frame is the constant one."""
    g = torch.Generator().manual_seed(100 * H + W)
    pred = torch.rand(B, 3, H, W, generator=g) * 1.2 - 0.1
    gt = torch.rand(B, 3, H, W, generator=g) * 1.2 - 0.1
    if B >= 2:
        gt[1].clamp_(0, 1)               # (identical under every flag combination: the clamp touches pred only)
        pred[1] = gt[1]
    if B == 3 or (H, W) == (16, 16):
        pred[B - 1] = 0.4
    return pred, gt


_REF = {}


def _reference(shape, clamp, quantize):
    """(pred, gt, fp64 statement, fp32 CPU statement), computed once per case."""
    key = (shape, clamp, quantize)
    if key not in _REF:
        pred, gt = _pairs(*shape)
        _REF[key] = (pred, gt, M.frame_metrics_torch(pred, gt, clamp, quantize, dtype=torch.float64),
                     M.frame_metrics_torch(pred, gt, clamp, quantize, dtype=torch.float32).double())
    return _REF[key]


@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frame_metrics_match_the_fp64_statement(shape, clamp, quantize):
    pred, gt, ref, cpu = _reference(shape, clamp, quantize)
    got = M.frame_metrics(pred.to(DEV), gt.to(DEV), clamp=clamp, quantize=quantize)
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], 5)
    got = got.cpu().double()
    rec = {}
    for b in range(shape[0]):
        for j, name in enumerate(M.COLUMNS):
            r, c, h = float(ref[b, j]), float(cpu[b, j]), float(got[b, j])
            rec[f"frame{b}_{name}"] = dict(value=r, err_fp32_cpu=abs(c - r) if math.isfinite(r) else 0.0,
                                           err_hip=abs(h - r) if math.isfinite(r) else 0.0, ulp=_ulp32(r))
    name = f"{'x'.join(map(str, shape))}_clamp{int(clamp)}_quant{int(quantize)}"
    _RECORD[name] = rec
    print(f"\n[metrics parity] {name}: {json.dumps(rec)}")
    out = os.environ.get("INSTAG_METRICS_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)
    for b in range(shape[0]):
        for j, col in enumerate(M.COLUMNS):
            assert _within(float(got[b, j]), float(cpu[b, j]), float(ref[b, j])), (b, col, rec[f"frame{b}_{col}"])
    if shape[0] >= 2:                    # pred == gt: mse = 0, psnr = +inf (both forms), ssim = 1 to rounding
        assert float(got[1, 0]) == 0 and float(got[1, 1]) == 0
        assert float(got[1, 2]) == math.inf and float(got[1, 3]) == math.inf
        assert abs(float(got[1, 4]) - 1) <= 2.0 ** -23
    assert float(ref[0, 1]) > 1e-3       # (the other frames differ)


def test_frame_metrics_runs_and_graph_replays_give_the_same_bits():
    from instag_amd import _lib
    pred, gt = (t.to(DEV) for t in _pairs(3, 37, 53))
    meter = M.Meter(DEV)
    a = M.frame_metrics(pred, gt, quantize=True, meter=meter).clone()
    b = M.frame_metrics(pred, gt, quantize=True, meter=meter).clone()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # meter after two calls == the fp64 sum of the per_frame rows (the +inf of the identical frame included)
    want = torch.cat([(a.double().sum(0) + b.double().sum(0)), torch.tensor([6.0], dtype=torch.float64, device=DEV)])
    assert torch.equal(meter.state[:6], want) and float(meter.state[6:].abs().sum()) == 0
    eager_state = meter.state.clone()
    meter.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _lib.graph_capture(graph):
        c = M.frame_metrics(pred, gt, quantize=True, meter=meter)
    meter.clear()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c.view(torch.int32), a.view(torch.int32))
    assert torch.equal(meter.state, eager_state)


def test_n_valid_leaves_the_padded_frame_out():
    pred, gt = (t.to(DEV) for t in _pairs(3, 37, 53))
    pred[1] = pred[0].flip(-1)                                   # (no +inf in the sums of this test)
    meter = M.Meter(DEV)
    rows = M.frame_metrics(pred, gt, meter=meter, n_valid=2)
    assert tuple(rows.shape) == (3, 5)                           # every frame is scored, two are counted
    assert torch.equal(meter.state[:5], rows[:2].double().sum(0)) and float(meter.state[5]) == 2
    rep = meter.report()
    assert rep["frames"] == 2 and rep["psnr"] == float(rows[:2, 2].double().mean())
    M.frame_metrics(pred, gt, meter=meter, n_valid=0)
    assert meter.report()["frames"] == 2
    with pytest.raises(RuntimeError, match="n_valid"):
        from instag_amd import _lib
        _lib.check(_lib.lib().instag_frame_metrics(_lib.ptr(pred), _lib.ptr(gt), 3, 37, 53, 0, _lib.ptr(pred),
                                                   _lib.ptr(rows), None, 4, _lib.current_stream()))


# ---- inference epilogue ----------------------------------------------------------------------------------------------
def _compose_inputs(H, W, corner, seed):
    g = torch.Generator().manual_seed(seed)
    a_face = torch.rand(1, H, W, generator=g)
    if corner:
        a_mouth = torch.zeros(1, H, W)
        a_mouth[0, H - 1, 0] = 0.75                              # a single non-zero pixel in a corner
    else:
        a_mouth = torch.rand(1, H, W, generator=g) ** 3
    face = torch.rand(3, H, W, generator=g) * 1.1
    mouth = torch.rand(3, H, W, generator=g)
    scene = torch.rand(3, H, W, generator=g)
    return face, a_face, mouth, a_mouth, scene


@pytest.mark.parametrize("dilate", [1, 3, 13])
@pytest.mark.parametrize("H,W", [(37, 53), (16, 16)])
def test_infer_compose_matches_the_torch_lines(H, W, dilate):
    for corner in (True, False):
        face, a_face, mouth, a_mouth, scene = _compose_inputs(H, W, corner, seed=H + dilate)
        # the running maximum has no rounding: mouth = 0, bg = 0, scene = 1, a = 0 -> image = 1 - a_d exactly
        z3, one3 = torch.zeros(3, H, W, device=DEV), torch.ones(3, H, W, device=DEV)
        img, _ = M.infer_compose(z3, torch.zeros(1, H, W, device=DEV), z3, a_mouth.to(DEV), torch.zeros(3, device=DEV),
                                 one3, dilate)
        a_d = F.max_pool2d(a_mouth[None], dilate, 1, dilate // 2)[0]
        assert torch.equal(img.cpu(), (1.0 - a_d).expand(3, H, W))
        if corner and dilate > 1:
            r = dilate // 2
            assert int((a_d > 0).sum()) == (r + 1) ** 2          # the window is cut at the border, not wrapped
        for bg in (torch.zeros(3), torch.tensor([0.0, 1.0, 0.0])):
            for sc in (scene, None):
                ref, _ = M.infer_compose_torch(*(t.double() for t in (face, a_face, mouth, a_mouth, bg)),
                                               None if sc is None else sc.double(), dilate)
                cpu, _ = M.infer_compose_torch(face, a_face, mouth, a_mouth, bg, sc, dilate)
                got, u8 = M.infer_compose(face.to(DEV), a_face.to(DEV), mouth.to(DEV), a_mouth.to(DEV), bg.to(DEV),
                                          None if sc is None else sc.to(DEV), dilate, as_uint8=True)
                assert got.dtype == torch.float32 and float(got.min()) >= 0 and float(got.max()) <= 1
                assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W, 3)
                assert torch.equal(u8, (got.permute(1, 2, 0) * 255).to(torch.uint8))
                e_cpu = float((cpu.double() - ref).abs().max())
                e_hip = (got.cpu().double() - ref).abs()
                floor = torch.from_numpy(np.spacing(ref.abs().float().numpy())).double()
                assert bool((e_hip <= 4 * e_cpu + floor).all()), (corner, bg.tolist(), sc is None,
                                                                  float(e_hip.max()), e_cpu)
                only, none = M.infer_compose(face.to(DEV), a_face.to(DEV), mouth.to(DEV), a_mouth.to(DEV), bg.to(DEV),
                                             None if sc is None else sc.to(DEV), dilate)
                assert none is None and torch.equal(only, got)


# ---- end to end on a small synthetic head ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def head():
    """A few thousand Gaussians, 64 x 64, 5 frames, as test_stages_gpu.py builds its fuse scenes."""
    from tests.test_stages_gpu import _frames, _mouth_setup
    dev = torch.device("cuda")
    pc, net, pcm, netm = _mouth_setup(dev, n_face=3000, n_mouth=800, seed=21)
    with torch.no_grad():                # (random-init fields move nothing visible: scale the output layers up)
        for mod in (net.sigma_net, netm.sigma_net, pc.neural_motion_grid.sigma_net, pc.neural_motion_grid.align_net,
                    pcm.neural_motion_grid.sigma_net, pcm.neural_motion_grid.align_net):
            mod.net[-1].weight.mul_(30.0)
    frames = _frames(64, 5, dev, background=True)
    bg = torch.zeros(3, device=dev)
    return dict(models=(pc, net, pcm, netm), frames=frames, bg=bg, gts=[f.original_image for f in frames],
                scenes=[f.talking_dict["background"] for f in frames])


def test_default_renderer_is_the_parent_path(head):
    from instag_amd.infer import FuseRenderer
    from instag_amd.renderer import render_fuse
    pc, net, pcm, netm = head["models"]
    r = FuseRenderer(pc, net, pcm, netm, head["bg"], dilate=1, as_uint8=False)
    for f, sb in zip(head["frames"][:2], head["scenes"]):
        with torch.no_grad():
            want = render_fuse(f, pc, net, pcm, netm, None, head["bg"], scene_background=sb, personalized=False,
                               inference=True)["image"].clamp(0, 1)
        got = r.render(f, sb)
        assert torch.is_tensor(got) and torch.equal(got, want)
    # the epilogue kernel composes the same frame (its own rounding), and writes the bytes of its own image
    r8 = FuseRenderer(pc, net, pcm, netm, head["bg"], as_uint8=True)
    image, u8 = r8.render(head["frames"][0], head["scenes"][0])
    assert float((image - r.render(head["frames"][0], head["scenes"][0])).abs().max()) <= 2e-6
    assert torch.equal(u8, (image.permute(1, 2, 0) * 255).to(torch.uint8)) and tuple(u8.shape) == (64, 64, 3)


def test_evaluator_graph_mode_equals_eager_and_the_torch_loop(head):
    from instag_amd import diff_gauss
    from instag_amd.infer import FuseRenderer
    pc, net, pcm, netm = head["models"]
    frames, gts, scenes = head["frames"], head["gts"], head["scenes"]
    r = FuseRenderer(pc, net, pcm, netm, head["bg"])
    try:
        eager = M.Evaluator(r, group=2).evaluate(frames, gts, scenes)
        images = [r.render(f, sb).cpu() for f, sb in zip(frames, scenes)]
        r.enable_graph(frames[0], frames_per_replay=2)
        assert r.frames_per_replay == 2
        graph = M.Evaluator(r).evaluate(frames, gts, scenes)     # 2 + 2 + (1 and one padded frame)
        assert not r.check_overflow()
    finally:
        r.close()
        diff_gauss.set_capacity_plan(None)
    assert graph["frames"] == 5 and eager["frames"] == 5
    assert graph == eager, (graph, eager)
    ref = torch.cat([M.frame_metrics_torch(im[None], gt[None].cpu(), True, True, dtype=torch.float64)
                     for im, gt in zip(images, gts)]).mean(0)
    cpu = torch.cat([M.frame_metrics_torch(im[None], gt[None].cpu(), True, True, dtype=torch.float32)
                     for im, gt in zip(images, gts)]).double().mean(0)
    print(f"\n[evaluate] {graph}")
    for j, k in enumerate(M.COLUMNS):
        assert _within(graph[k], float(cpu[j]), float(ref[j])), (k, graph[k], float(cpu[j]), float(ref[j]))
    assert 3 < graph["psnr"] < 40 and graph["lpips"] is None


def test_dilated_uint8_renderer_captured_equals_eager(head):
    from instag_amd import diff_gauss
    from instag_amd.infer import FuseRenderer
    pc, net, pcm, netm = head["models"]
    frames, scenes = head["frames"], head["scenes"]
    r = FuseRenderer(pc, net, pcm, netm, head["bg"], dilate=13, as_uint8=True)
    plain = FuseRenderer(pc, net, pcm, netm, head["bg"])
    try:
        want_img, want_u8 = r.render_batch(frames[:3], scenes[:3])
        assert tuple(want_u8.shape) == (3, 64, 64, 3) and want_u8.dtype == torch.uint8
        assert float((want_img[0] - plain.render(frames[0], scenes[0])).abs().max()) > 1e-3       # dilation shows
        r.enable_graph(frames[0], frames_per_replay=2)
        got_img, got_u8 = r.render_batch(frames[:3], scenes[:3])
        assert not r.check_overflow()
    finally:
        r.close()
        diff_gauss.set_capacity_plan(None)
    assert torch.equal(got_img, want_img) and torch.equal(got_u8, want_u8)
    assert torch.equal(got_u8, (got_img.permute(0, 2, 3, 1) * 255).to(torch.uint8))


def test_frame_lpips_matches_the_torch_statement_and_rejects_other_shapes():
    from instag_amd import lpips as LP
    w = LP.LPIPSWeights.random(0)
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(2, 3, 64, 64, generator=g)
    pred = (gt + 0.05 * torch.randn(2, 3, 64, 64, generator=g)).clamp(0, 1)
    v64 = LP.lpips_torch(2 * gt.double() - 1, 2 * pred.double() - 1, w).reshape(-1)
    v32 = LP.lpips_torch(2 * gt - 1, 2 * pred - 1, w).reshape(-1).double()
    meter = M.Meter(DEV)
    op = M.FrameLPIPS(w, 64, 64)
    got = op(pred.to(DEV), gt.to(DEV), meter=meter, n_valid=1)
    assert tuple(got.shape) == (2,) and got.dtype == torch.float32
    vh = got.cpu().double()
    for i in range(2):                   # the forward-value bound of tests/test_lpips_gpu.py
        assert float(v64[i]) > 1e-4
        assert float((vh[i] - v64[i]).abs()) <= 4 * float((v32[i] - v64[i]).abs()) + 64 * 2.0 ** -23 * float(v64[i])
    rep = meter.report()
    assert rep["lpips"] == float(got[0]) and rep["frames"] == 0
    assert torch.equal(op(pred.to(DEV), gt.to(DEV)), got)
    with pytest.raises(ValueError, match="1024"):
        M.FrameLPIPS(w, 64, 48)(pred[:, :, :, :48].to(DEV), gt[:, :, :, :48].to(DEV))


def test_face_validation_is_the_reference_loop(head):
    from instag_amd import losses
    from instag_amd.renderer import render_motion
    pc, net, _, _ = head["models"]
    frames, gts = head["frames"][:3], head["gts"][:3]
    bg = torch.tensor([0.0, 1.0, 0.0], device=DEV)
    got = M.face_validation(pc, net, frames, gts, bg)
    assert set(got) == {"l1", "psnr"}
    # train_face.py:830-874 in plain torch, on the same renders; in fp32 (the yardstick) and in fp64
    sums = {torch.float32: [0.0, 0.0], torch.float64: [0.0, 0.0]}
    with torch.no_grad():
        for viewpoint, gt in zip(frames, gts):
            render_pkg = render_motion(viewpoint, pc, net, None, bg, return_attn=True, frame_idx=0, align=True)
            for dt, acc in sums.items():
                image = torch.clamp(render_pkg["render"], 0.0, 1.0).cpu().to(dt)
                alpha = render_pkg["alpha"].cpu().to(dt)
                background = viewpoint.talking_dict["background"].cpu().to(dt)
                image = image - bg.cpu().to(dt)[:, None, None] * (1.0 - alpha) + background * (1.0 - alpha)
                gt_image = torch.clamp(gt.cpu().to(dt), 0.0, 1.0)
                acc[0] += losses.l1_loss(image, gt_image).mean().double()
                acc[1] += losses.psnr(image, gt_image).mean().double()
    l1_32, psnr_32 = (float(v) / 3 for v in sums[torch.float32])
    l1_64, psnr_64 = (float(v) / 3 for v in sums[torch.float64])
    print(f"\n[face validation] {got} fp64 l1 {l1_64} psnr {psnr_64}")
    # the composition of :847 runs in fp32 on the device before the metrics kernel reads it: one more rounding per
    # pixel than the fp64 lines, the same as the fp32 lines
    assert _within(got["l1"], l1_32, l1_64), (got["l1"], l1_32, l1_64)
    assert _within(got["psnr"], psnr_32, psnr_64), (got["psnr"], psnr_32, psnr_64)
