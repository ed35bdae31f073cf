"""GPU: the HIP LPIPS patch loss (csrc/lpips.hip) against the fp64 plain-torch statement, its determinism and its replay
from one captured graph across patch sizes.

Tolerances are not fixed in advance: the yardstick of a case is the error of ``patch_lpips_torch`` in fp32 on the CPU
against the same function in fp64 on the same inputs, and the HIP path -- which only reorders fp32 sums -- gets 4x that,
plus a floor for figures near zero: 64 eps32 relative to the value (the gradient: to its largest entry), the rounding
a random walk over the longest contraction of the network (K = 3456, sqrt(K) ~ 59 roundings) leaves in an fp32 sum.

Measured on an MI355X (profiles/r06_lpips_parity.json holds all twelve cases):

  * value: both fp32 paths sit at the fp32 quantum of the value, 5e-9 .. 1.1e-7 relative (HIP and fp32 CPU mostly the
    same float);
  * gradient, max |error| / max |gradient| over the whole [3,H,W] tensor: fp32 CPU 2.1e-6 .. 2.6e-6, HIP 1.0e-6 ..
    1.7e-6 -- except where an fp32 evaluation routes the gradient through another unit than fp64 does (two pool inputs
    within rounding of each other, a pre-activation within rounding of zero): the gradient is discontinuous there and
    the error is 0.5 .. 2 % of the largest entry inside that unit's receptive field.  The fp32 CPU statement does so
    for p = 96 (1.7e-2) and p = 42 (4.5e-3 / 6.2e-3); the HIP path for p = 42 only, with the CPU's figures;
  * gradient, root mean square of the errors below each path's 99th percentile, relative to the largest entry: fp32
    CPU 1.7e-7 .. 3.1e-7, HIP 0.95e-7 .. 1.5e-7.

  With one FMA chain over the whole K the convolutions of conv2..5 were 2.5 - 3x less accurate than the library's
  (activation error 1.1e-5 against 4e-6) and the 512x512, p = 80 case without rectangle took another pool branch
  (gradient error 8.9e-3, bound 1e-5); the blocked summation of csrc/lpips.hip brought the activations to the
  library's error or below and that case to 1.3e-6.
"""
import json
import os

import pytest
import torch

from instag_amd import lpips as LP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23
CASES = [(512, 512, 64), (512, 512, 80), (512, 512, 96), (512, 512, 32), (512, 512, 42), (450, 500, 64)]
RANGES = {64: (64, 96), 80: (64, 96), 96: (64, 96), 32: (32, 42), 42: (32, 42)}
_RECORD = {}


def _images(H, W, seed=0):
    """Smooth images plus noise; image and target differ by a few percent (non-trivial ReLU patterns)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 9, H), torch.linspace(0, 9, W), indexing="ij")
    base = torch.stack([0.5 + 0.35 * torch.sin(2 * yy + xx), 0.5 + 0.35 * torch.cos(yy - 2 * xx),
                        0.5 + 0.3 * torch.sin(3 * xx) * torch.cos(yy)])
    image = (base + 0.06 * torch.randn(3, H, W, generator=g)).clamp(0.01, 0.99)
    gt = (image + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return image, gt


def _statement(image, gt, p, w, rect, bg, dtype):
    x = image.to(dtype).requires_grad_(True)
    v = LP.patch_lpips_torch(x, gt.to(dtype), p, w, rect, None if bg is None else bg.to(dtype))
    g, = torch.autograd.grad(v, x)
    return v.detach().double(), g.double()


def _hip(op, image, gt, p, rect, bg):
    x = image.to(DEV).requires_grad_(True)
    r = None if rect is None else torch.tensor(rect, dtype=torch.int32, device=DEV)
    v = op(x, gt.to(DEV), p, r, None if bg is None else bg.to(DEV))
    g, = torch.autograd.grad(v, x)
    return v.detach(), g


@pytest.mark.parametrize("with_rect", [False, True])
@pytest.mark.parametrize("H,W,p", CASES)
def test_value_and_gradient_match_the_fp64_statement(H, W, p, with_rect):
    w = LP.LPIPSWeights.random(5)
    image, gt = _images(H, W, seed=p)
    bg = torch.tensor([0.0, 1.0, 0.0]) if with_rect else None
    rect = (H // 2 - 40, H // 2 + 37, W // 2 - 75, W // 2 + 70) if with_rect else None
    v64, g64 = _statement(image, gt, p, w, rect, bg, torch.float64)
    v32, g32 = _statement(image, gt, p, w, rect, bg, torch.float32)
    lo, hi = RANGES[p]
    op = LP.PatchLPIPS(w, H, W, lo, hi)
    vh, gh = _hip(op, image, gt, p, rect, bg)
    vh, gh = vh.cpu().double(), gh.cpu().double()

    ev_ref, ev_hip = float((v32 - v64).abs()), float((vh - v64).abs())
    eg_ref, eg_hip = float((g32 - g64).abs().max()), float((gh - g64).abs().max())
    gmax = float(g64.abs().max())
    rec = dict(value=float(v64), grad_max=gmax, value_err_fp32_cpu=ev_ref, value_err_hip=ev_hip,
               grad_err_fp32_cpu=eg_ref, grad_err_hip=eg_hip)
    _RECORD[f"{H}x{W}_p{p}_{'rect' if with_rect else 'plain'}"] = rec
    print(f"\n[lpips parity] {H}x{W} p={p} rect={with_rect}: {json.dumps(rec)}")
    out = os.environ.get("INSTAG_LPIPS_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)

    assert float(v64) > 1e-4 and gmax > 0
    assert ev_hip <= 4 * ev_ref + 64 * EPS32 * float(v64)
    assert eg_hip <= 4 * eg_ref + 64 * EPS32 * gmax          # (max over EVERY element of the [3,H,W] gradient)
    # Where the fp32 CPU statement takes another ReLU / pool branch than fp64, its largest error is that one unit's
    # receptive field and the bound above is loose for every other pixel.  The same yardstick on the error norm a single
    # unit cannot move keeps those cases meaningful: the root mean square over the elements that are not among the 1 %
    # largest errors of the respective path (the 1 % covers a 51 x 51 field of one 512 x 512 image with room to spare).
    def trimmed_rms(e):
        e = e.reshape(-1).abs().sort().values[: int(0.99 * e.numel())]
        return float(e.pow(2).mean().sqrt())
    er_ref, er_hip = trimmed_rms(g32 - g64), trimmed_rms(gh - g64)
    rec.update(grad_trimmed_rms_fp32_cpu=er_ref, grad_trimmed_rms_hip=er_hip)
    print(f"[lpips parity] trimmed rms: fp32 cpu {er_ref:.3e} hip {er_hip:.3e}")
    if out:
        with open(out, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)
    assert er_hip <= 4 * er_ref + 64 * EPS32 * gmax / 59       # (floor: one rounding of the largest entry, not sqrt(K))

    # exact zeros in the dropped remainder and inside the filled rectangle, and only where the statement has them
    live = torch.zeros(H, W, dtype=torch.bool)
    live[:H // p * p, :W // p * p] = True
    if rect is not None:
        live[rect[0]:rect[1], rect[2]:rect[3]] = False
    assert torch.equal(gh[:, ~live], torch.zeros_like(gh[:, ~live]))
    assert torch.equal(gh == 0, g64 == 0)
    if p % 4 == 0:           # (conv1's last window ends on the patch's last pixel: every live pixel is seen)
        assert bool((gh[:, live] != 0).all())


def test_criterion_on_cut_patches_equals_the_patch_operator():
    w = LP.LPIPSWeights.random(6)
    image, gt = _images(512, 512, seed=1)
    p = 64
    x = LP.patchify(image * 2 - 1, p).to(DEV).requires_grad_(True)
    y = LP.patchify(gt * 2 - 1, p).to(DEV)
    d = LP.LPIPS(w)(x, y)
    assert tuple(d.shape) == (64, 1, 1, 1)
    img = image.to(DEV).requires_grad_(True)
    v = LP.PatchLPIPS(w, 512, 512, 64, 96)(img, gt.to(DEV), p)
    want = LP.lpips_torch(x.detach().cpu().double(), y.cpu().double(), w)
    assert torch.allclose(d.detach().cpu().double(), want, rtol=2e-4, atol=1e-7)
    # same kernels, same order: only the `* 2 - 1` is applied in another place (exact in fp32 for these inputs or
    # one rounding), and the mean is one more ordered sum
    assert torch.allclose(d.mean(), v, rtol=1e-5, atol=0)
    gx, = torch.autograd.grad(d.mean(), x)
    gi, = torch.autograd.grad(v, img)
    # (the patch gradients folded back into the image's layout; d(x * 2 - 1) / d image = 2)
    folded = torch.nn.functional.fold((gx * 2).reshape(1, 64, -1).permute(0, 2, 1), (512, 512), p, stride=p)[0]
    assert torch.allclose(folded, gi, rtol=1e-4, atol=1e-6 * float(gi.abs().max()))


def test_a_backward_behind_another_forward_raises():
    """One operator keeps the activations of its last forward only: a backward of an earlier one must not run on them."""
    w = LP.LPIPSWeights.random(6)
    image, gt = _images(128, 128, seed=4)
    x = LP.patchify(image * 2 - 1, 64).to(DEV).requires_grad_(True)
    y = LP.patchify(gt * 2 - 1, 64).to(DEV)
    crit = LP.LPIPS(w)
    first = crit(x, y).mean()
    second = crit(x, y.flip(0)).mean()
    with pytest.raises(RuntimeError, match="another forward"):
        first.backward()
    second.backward()                                            # (the last forward's backward is fine)
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    # two terms of one loss: one operator each
    a, b = LP.LPIPS(w), LP.LPIPS(w)
    (a(x, y).mean() + b(x, y.flip(0)).mean()).backward()


def test_two_eager_runs_are_bit_identical():
    w = LP.LPIPSWeights.random(7)
    image, gt = _images(512, 512, seed=2)
    bg = torch.tensor([1.0, 1.0, 1.0])
    op = LP.PatchLPIPS(w, 512, 512, 64, 96)
    a = _hip(op, image, gt, 72, (210, 300, 150, 340), bg)
    _hip(op, image, gt, 96, None, None)                          # (another size in between: no state leaks)
    b = _hip(op, image, gt, 72, (210, 300, 150, 340), bg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_one_captured_graph_serves_every_patch_size():
    from instag_amd import _lib
    w = LP.LPIPSWeights.random(8)
    image, gt = _images(512, 512, seed=3)
    bg = torch.tensor([0.0, 1.0, 0.0]).to(DEV)
    op = LP.PatchLPIPS(w, 512, 512, 64, 96)
    x = image.to(DEV).requires_grad_(True)
    y = gt.to(DEV)
    rect = torch.tensor([200, 280, 160, 330], dtype=torch.int32, device=DEV)
    p_dev = op.stage(64, DEV)
    _hip(op, image, gt, 64, (200, 280, 160, 330), bg)            # (code objects loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _lib.graph_capture(graph):
        v = op(x, y, p_dev, rect, bg)
        g, = torch.autograd.grad(v, x)
    for p, r in ((64, (200, 280, 160, 330)), (78, (100, 190, 300, 420)), (96, (200, 280, 160, 330)), (66, (0, 0, 0, 0))):
        op.stage(p, DEV)
        rect.copy_(torch.tensor(r, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        got_v, got_g = v.clone(), g.clone()
        want_v, want_g = _hip(op, image, gt, p, r, bg)
        assert torch.equal(got_v, want_v), (p, r)
        assert torch.equal(got_g, want_g), (p, r)


# ---- trainers ---------------------------------------------------------------------------------------------------------
def _frames(size, n, dev, **kw):
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    from instag_amd.train import make_frame
    cams = toy_cameras(size)
    return [make_frame(cams[i].to(dev), synthetic_frame(size, i, dev, **kw)) for i in range(n)]


def _face_trainer(dev, w, seed=2, n=3000):
    from types import SimpleNamespace
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, PersonalizedMotionNetwork
    from instag_amd.scene_synth import synthetic_gaussians
    from instag_amd.train import FaceTrainer
    torch.manual_seed(seed)
    args = SimpleNamespace(audio_extractor="deepspeech", type="face")
    pmf = PersonalizedMotionNetwork(args=args).to(dev)
    umf = MotionNetwork(args=args).to(dev)
    g = GaussianModel(1, neural_motion_grid=pmf)
    g.load_raw(synthetic_gaussians(n, sh_degree=1, seed=seed), dev)
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    return FaceTrainer(g, umf, bg, densify=False, seed=seed, schedule="reference", lpips=w)


def _grads(tr):
    out = {k: p.grad.detach().clone() for k, p in tr.g._p.items() if p.grad is not None}
    for name, net in (("umf", tr.motion_net), ("pmf", tr.g.neural_motion_grid)):
        for n_, p_ in net.named_parameters():
            if p_.grad is not None:
                out[f"{name}.{n_}"] = p_.grad.detach().clone()
    return out


def test_face_trainer_step_matches_the_torch_statement_of_the_late_phase():
    """One FaceTrainer(schedule="reference", lpips=w) step above iteration 7,500 == train_face.py:333-335 (closed mouth
    mask), :415-575 (loss block, priors) and :596-620 (lips fill, patches, 0.01 * lpips) written with plain torch ops
    behind the same render; tolerances of test_stages_gpu.py's face-step comparison."""
    from instag_amd.deferred import deferred_grads
    from instag_amd.losses import face_loss_torch, normalize
    from instag_amd.renderer import render_motion
    from instag_amd.train import face_phase
    dev = torch.device("cuda")
    w = LP.LPIPSWeights.random(9)
    it, p = 7600, 64
    frame = _frames(128, 1, dev, priors=True)[0]
    tr = _face_trainer(dev, w)
    assert tr.lpips_on(it) and not tr.lpips_on(7500)
    phase = face_phase(it)
    tr._lpips_p = p
    pkg, loss, l1 = tr._forward_backward(frame, phase)
    got = _grads(tr)
    tr._zero_grad()

    pkg2 = render_motion(frame, tr.g, tr.motion_net, None, tr.bg, return_attn=True, personalized=False, align=phase.align)
    td = frame.talking_dict
    face, hair = td["face_mask"], td["hair_mask"]
    max_pool = torch.nn.MaxPool2d(kernel_size=3, stride=1, padding=1)
    mouth = (-max_pool(-max_pool(td["mouth_mask"][None].float())))[0].bool()
    m, pm = pkg2["motion"], pkg2["p_motion"]
    extra = (m["d_xyz"].abs().mean() + m["d_rot"].abs().mean() + m["d_opa"].abs().mean()
             + m["d_scale"].abs().mean() + pm["p_xyz"].abs().mean())
    want, want_l1 = face_loss_torch(pkg2["render"], frame.original_image, face, hair, mouth, tr.bg, alpha=pkg2["alpha"],
                                    attn=pkg2["attn"], lips_rect=td["lips_rect"], extra=extra, hair_mask_iter=False)
    head = face + hair
    want = want + 0.01 * (1 - td["normal"] * pkg2["normal"]).sum(0)[head ^ mouth].mean()
    sel = face ^ mouth
    want = want + 1e-2 * (normalize(pkg2["depth"][0])[sel] - normalize(td["depth"])[sel]).abs().mean()
    gt_white = frame.original_image * head + tr.bg[:, None, None] * ~head
    gt_white[:, mouth] = tr.bg[:, None]
    term = LP.patch_lpips_torch(pkg2["render"], gt_white, p, w, td["lips_rect"], tr.bg)
    assert 0.01 * float(term) > 20 * 2e-6          # (the term is far above the tolerance of the loss comparison below)
    want = want + 0.01 * term
    with deferred_grads(dev):
        want.backward()
    ref = _grads(tr)
    print(f"\n[face step] loss {float(loss):.8f} want {float(want):.8f} lpips term {float(term):.6f}")
    assert abs(float(loss) - float(want)) <= 2e-6 * max(1.0, abs(float(want))), (float(loss), float(want))
    assert abs(float(l1) - float(want_l1)) <= 2e-6
    assert set(got) == set(ref), set(got) ^ set(ref)
    for k in ref:
        scale = float(ref[k].abs().max())
        err = float((got[k] - ref[k]).abs().max())
        assert err <= 2e-4 * scale + 1e-9, (k, err, scale)


def test_face_trainer_captured_step_matches_eager_across_patch_sizes():
    from instag_amd import diff_gauss
    dev = torch.device("cuda")
    w = LP.LPIPSWeights.random(9)
    frames = _frames(128, 2, dev, priors=True)

    def run(graph):
        tr = _face_trainer(dev, w, seed=1)
        tr.iteration = 7600
        try:
            if graph:
                tr.enable_graph(frames[0], warmup_steps=1, keep_state=True)
                assert tr.iteration == 7600
            outs = []
            for i in range(2):                   # (a captured step hands out the same loss tensor every replay: read now)
                o = tr.step(frames[i])
                outs.append(dict(loss=float(o["loss"]), patch=o["patch"]))
                if graph:                        # the scalar the captured kernels read holds THIS step's patch size
                    assert tr.optimizers.combined.extra_i64() is not None
                    assert int(tr._p_dev.view(torch.int32)[0]) == o["patch"] == int(tr._p_dev[0])
            if graph:
                assert tr._graph is not None and tr.recaptures == 0          # one graph, two patch sizes
        finally:
            diff_gauss.set_capacity_plan(None)
        vec = torch.cat([tr.g._p[k].detach().reshape(-1) for k in ("f_dc", "opacity", "xyz")])
        return [float(o["loss"]) for o in outs], [o["patch"] for o in outs], vec

    le, pe, ve = run(False)
    lg, pg, vg = run(True)
    assert pe == pg and pe[0] != pe[1] and all(64 <= q <= 96 and q % 2 == 0 for q in pe), (pe, pg)
    for a_, b_ in zip(le, lg):
        assert abs(a_ - b_) <= 2e-6 * max(1.0, abs(a_)), (le, lg)
    assert float((ve - vg).abs().max()) <= 2e-4


def _fuse_setup(dev, seed):
    from tests.test_stages_gpu import _mouth_setup
    return _mouth_setup(dev, n_face=2000, n_mouth=900, seed=seed)


def test_fuse_trainer_step_matches_the_torch_statement_of_the_second_half():
    from instag_amd.losses import l1_loss, ssim
    from instag_amd.train_stages import FuseTrainer
    from tests.test_stages_gpu import SmallOpt
    dev = torch.device("cuda")
    w = LP.LPIPSWeights.random(10)
    Opt = type("Opt", (SmallOpt,), {"iterations": 100000})
    pc_face, face_net, pc_mouth, mouth_net = _fuse_setup(dev, 6)
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    tr = FuseTrainer(pc_face, face_net, pc_mouth, mouth_net, bg, opt=Opt, lpips=w)
    assert not tr._lpips_on(50000) and tr._lpips_on(50001)
    frame = _frames(128, 1, dev, background=True)[0]
    p = 36
    out, loss, l1 = tr.forward(frame, p)
    image, gt = out["image"], frame.original_image
    term = LP.patch_lpips_torch(image, gt, p, w)
    want = l1_loss(image, gt) + 0.2 * (1.0 - ssim(image, gt)) + 0.05 * term
    params = [pc_face._p["f_dc"], pc_face._p["opacity"], pc_mouth._p["f_dc"]]
    got = torch.autograd.grad(loss, params, retain_graph=True)
    ref = torch.autograd.grad(want, params)
    print(f"\n[fuse step] loss {float(loss):.8f} want {float(want):.8f} lpips term {float(term):.6f}")
    assert 0.05 * float(term) > 20 * 2e-6          # (the term is far above the tolerance of the loss comparison)
    assert abs(float(loss) - float(want)) <= 2e-6 * max(1.0, abs(float(want)))
    for a_, b_ in zip(got, ref):
        scale = float(b_.abs().max())
        assert float((a_ - b_).abs().max()) <= 2e-4 * scale + 1e-9


def test_fuse_trainer_captured_step_matches_eager_across_patch_sizes():
    from instag_amd import diff_gauss
    from instag_amd.train_stages import FuseTrainer
    from tests.test_stages_gpu import SmallOpt
    dev = torch.device("cuda")
    w = LP.LPIPSWeights.random(10)
    Opt = type("Opt", (SmallOpt,), {"iterations": 100000})
    bg = torch.tensor([0.0, 1.0, 0.0], device=dev)
    frames = _frames(128, 3, dev, background=True)

    def run(graph):
        pc_face, face_net, pc_mouth, mouth_net = _fuse_setup(dev, 7)
        tr = FuseTrainer(pc_face, face_net, pc_mouth, mouth_net, bg, opt=Opt, seed=3, lpips=w)
        tr.iteration = 60000
        try:
            if graph:
                tr.enable_graph(frames[0], warmup_steps=2)          # 4 real steps on frame 0
                assert tr.iteration == 60004 and tr._graph is not None
            else:
                for _ in range(4):
                    tr.step(frames[0])
            outs = []
            for i in range(4):                   # (a captured step hands out the same loss tensor every replay: read now)
                o = tr.step(frames[i % 3])
                outs.append(dict(loss=float(o["loss"]), patch=o["patch"]))
                if graph:                        # the scalar the captured kernels read holds THIS step's patch size
                    assert tr.optimizers.combined.extra_i64() is not None
                    assert int(tr._p_dev.view(torch.int32)[0]) == o["patch"] == int(tr._p_dev[0])
            if graph:
                assert tr._graph is not None and not tr._graph.check_overflow()
        finally:
            diff_gauss.set_capacity_plan(None)
        vec = torch.cat([tr.g._p["f_dc"].detach().reshape(-1), tr.g._p["opacity"].detach().reshape(-1)])
        return [float(o["loss"]) for o in outs], [o["patch"] for o in outs], vec

    le, pe, ve = run(False)
    lg, pg, vg = run(True)
    assert pe == pg and len(set(pe)) > 1 and all(32 <= q <= 42 and q % 2 == 0 for q in pe), (pe, pg)
    for a_, b_ in zip(le, lg):
        assert abs(a_ - b_) <= 1e-4 * max(1.0, abs(a_)), (le, lg)
    assert float((ve - vg).abs().max()) <= 2e-4
