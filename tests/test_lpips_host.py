"""CPU: the plain-torch statement of the LPIPS patch loss, its weights container, the late-phase schedule, the mouth-mask
closing and the C ABI's argument checks."""
import ctypes
import random

import pytest
import torch
import torch.nn.functional as F

from instag_amd import lpips as LP
from instag_amd.gaussian_model import OptimizationParams


def _images(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 3, W), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(2 * yy + xx), 0.5 + 0.4 * torch.cos(yy - 2 * xx), 0.5 + 0.3 * torch.sin(3 * xx)])
    image = (base + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gt = (image + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return image, gt


def test_lpips_torch_is_a_distance_of_the_declared_shape():
    w = LP.LPIPSWeights.random(1)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(3, 3, 64, 64, generator=g) * 2 - 1
    y = torch.rand(3, 3, 64, 64, generator=g) * 2 - 1
    d = LP.lpips_torch(x, y, w)
    assert tuple(d.shape) == (3, 1, 1, 1)
    assert torch.all(d > 0)
    assert torch.equal(LP.lpips_torch(x, x, w), torch.zeros(3, 1, 1, 1))
    assert torch.allclose(d, LP.lpips_torch(y, x, w), rtol=1e-6, atol=0)
    # per-sample: a batch is its rows
    assert torch.allclose(d[1:2], LP.lpips_torch(x[1:2], y[1:2], w), rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("H,W,p", [(512, 512, 64), (450, 500, 64)])
def test_patch_lpips_torch_is_unfold_then_lpips(H, W, p):
    w = LP.LPIPSWeights.random(2)
    image, gt = _images(H, W)
    bg = torch.tensor([0.0, 1.0, 0.0])
    rect = (200, 260, 180, 300)
    a, b = image.clone(), gt.clone()
    a[:, 200:260, 180:300] = bg[:, None, None]
    b[:, 200:260, 180:300] = bg[:, None, None]
    for (i, t, r) in ((image, gt, None), (a, b, rect)):
        px = F.unfold((i * 2 - 1)[None], p, stride=p).permute(0, 2, 1).reshape(-1, 3, p, p)
        py = F.unfold((t * 2 - 1)[None], p, stride=p).permute(0, 2, 1).reshape(-1, 3, p, p)
        assert px.shape[0] == (H // p) * (W // p)
        want = LP.lpips_torch(px, py, w).mean()
        got = LP.patch_lpips_torch(image, gt, p, w, r, bg if r else None)
        assert got.dim() == 0 and torch.equal(got, want)
    # the CPU path of the operators is the statement
    assert torch.equal(LP.PatchLPIPS(w, H, W, 64, 96)(image, gt, p, rect, bg), LP.patch_lpips_torch(image, gt, p, w, rect, bg))
    assert torch.equal(LP.LPIPS(w)(px, py), LP.lpips_torch(px, py, w))


def test_weights_load_from_both_key_spellings(tmp_path):
    w = LP.LPIPSWeights.random(3)
    alex = {}
    for i, (cw, cb) in zip(LP.FEATURES, w.conv):
        alex[f"features.{i}.weight"], alex[f"features.{i}.bias"] = cw, cb
    alex["classifier.1.weight"] = torch.zeros(2, 2)               # (what else the file holds is ignored)
    package = {f"lin{l}.model.1.weight": w.lin[l].view(1, -1, 1, 1) for l in range(5)}
    renamed = {f"{l}.1.weight": w.lin[l].view(1, -1, 1, 1) for l in range(5)}
    a = LP.LPIPSWeights.from_state_dicts(alex, package)
    b = LP.LPIPSWeights.from_state_dicts(alex, renamed)
    for x in (a, b):
        for (cw, cb), (rw, rb) in zip(x.conv, w.conv):
            assert torch.equal(cw, rw) and torch.equal(cb, rb)
        for l in range(5):
            assert torch.equal(x.lin[l], w.lin[l])
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(package, tmp_path / "alex.pth")
    c = LP.LPIPSWeights.load(tmp_path / "alexnet.pth", tmp_path / "alex.pth")
    assert all(torch.equal(c.lin[l], w.lin[l]) for l in range(5))
    del renamed["3.1.weight"]
    with pytest.raises(KeyError):
        LP.LPIPSWeights.from_state_dicts(alex, renamed)
    del alex["features.6.bias"]
    with pytest.raises(KeyError):
        LP.LPIPSWeights.from_state_dicts(alex, package)


def test_schedule_and_patch_sizes():
    opt = OptimizationParams
    assert LP.face_lpips_start(opt) == 7500
    assert not LP.face_lpips_on(7500, opt) and LP.face_lpips_on(7501, opt)
    assert LP.fuse_lpips_start(opt) == opt.iterations // 2
    assert not LP.fuse_lpips_on(opt.iterations // 2, opt) and LP.fuse_lpips_on(opt.iterations // 2 + 1, opt)
    rng = random.Random(0)
    assert {LP.draw_face_patch(rng) for _ in range(4000)} == set(range(64, 97, 2))
    assert {LP.draw_fuse_patch(rng) for _ in range(4000)} == set(range(32, 43, 2))
    assert LP.FACE_PATCH_RANGE == (64, 96) and LP.FUSE_PATCH_RANGE == (32, 42)
    assert LP.FACE_LPIPS_WEIGHT == 0.01 and LP.FUSE_LPIPS_WEIGHT == 0.05


def test_mask_closing_is_the_double_pool():
    g = torch.Generator().manual_seed(4)
    mask = torch.rand(97, 113, generator=g) > 0.6
    max_pool = torch.nn.MaxPool2d(kernel_size=3, stride=1, padding=1)
    want = (-max_pool(-max_pool(mask[None].float())))[0].bool()
    got = LP.close_mask(mask)
    assert got.dtype == torch.bool and torch.equal(got, want)
    assert not torch.equal(got, mask)


def test_argument_errors_do_not_need_a_gpu():
    from instag_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(64)
    s = _lib.LpipsWeights()
    for l in range(5):
        s.wf[l] = s.bias[l] = s.wb[l] = s.lin[l] = 64
    w = ctypes.byref(s)

    def fwd(image=one, p_dev=one, p_host=64, H=512, W=512, p_min=64, p_max=96, weights=w, rect=None, bg=None):
        return lib.instag_lpips_forward(weights, image, one, p_dev, p_host, rect, bg, H, W, p_min, p_max, 0, one, 1 << 40,
                                        one, one, None)

    assert fwd(image=None) != 0 and b"NULL" in lib.instag_last_error()
    assert fwd(p_dev=None) != 0 and b"NULL" in lib.instag_last_error()
    assert fwd(weights=ctypes.byref(_lib.LpipsWeights())) != 0 and b"NULL" in lib.instag_last_error()
    assert fwd(rect=one) != 0 and b"NULL background" in lib.instag_last_error()
    assert fwd(p_host=98) != 0 and b"outside the declared range" in lib.instag_last_error()
    assert fwd(p_host=62) != 0 and b"outside the declared range" in lib.instag_last_error()
    assert fwd(H=60, p_host=64) != 0 and b"smaller than one patch" in lib.instag_last_error()
    assert fwd(H=80, p_host=90) != 0 and b"smaller than one patch" in lib.instag_last_error()
    assert fwd(p_min=30, p_host=30) != 0 and b"below 31" in lib.instag_last_error()
    assert fwd(p_min=96, p_max=64) != 0 and b"range" in lib.instag_last_error()
    rc = lib.instag_lpips_backward(w, one, 64, None, None, 0, 512, 512, 64, 96, 0, one, 1 << 40, one, None)
    assert rc != 0 and b"NULL" in lib.instag_last_error()
    rc = lib.instag_lpips_backward(w, one, 100, None, one, 0, 512, 512, 64, 96, 0, one, 1 << 40, one, None)
    assert rc != 0 and b"outside the declared range" in lib.instag_last_error()
    rc = lib.instag_lpips_backward(w, one, 64, None, one, 0, 512, 512, 64, 96, 0, one, 16, one, None)
    assert rc != 0 and b"workspace too small" in lib.instag_last_error()
    assert lib.instag_lpips_workspace_bytes(512, 512, 30, 96, 0) == 0 and b"below 31" in lib.instag_last_error()
    assert lib.instag_lpips_workspace_bytes(512, 512, 64, 96, 0) > 0
    assert lib.instag_lpips_max_patches(512, 512, 64, 96, 0) == 64
    assert lib.instag_lpips_max_patches(450, 500, 64, 64, 0) == 49
    with pytest.raises(ValueError):
        LP.PatchLPIPS(LP.LPIPSWeights.random(0), 512, 512, 30, 96)
    with pytest.raises(ValueError):
        LP.PatchLPIPS(LP.LPIPSWeights.random(0), 80, 512, 64, 96)
    with pytest.raises(ValueError):
        LP.PatchLPIPS(LP.LPIPSWeights.random(0), 512, 512, 64, 96)(torch.zeros(3, 512, 512), torch.zeros(3, 512, 512), 98)


def test_trainers_own_a_seeded_patch_generator():
    """Two trainers with one seed draw the same patch sizes; the term is opt-in and bound to the reference schedule."""
    from types import SimpleNamespace
    from oracle.grid_torch import GridEncoder as CpuGrid
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, PersonalizedMotionNetwork
    from instag_amd.scene_synth import synthetic_gaussians
    from instag_amd.train import FaceTrainer, face_phase, FacePhase
    w = LP.LPIPSWeights.random(0)

    def make(seed, **kw):
        torch.manual_seed(0)
        args = SimpleNamespace(audio_extractor="deepspeech", type="face")
        g = GaussianModel(1, neural_motion_grid=PersonalizedMotionNetwork(args=args, encoder_cls=CpuGrid))
        g.load_raw(synthetic_gaussians(64, sh_degree=1, seed=0), torch.device("cpu"))
        return FaceTrainer(g, MotionNetwork(args=args, encoder_cls=CpuGrid), torch.tensor([0.0, 1.0, 0.0]), densify=False,
                           seed=seed, **kw)

    a, b, c = make(5, schedule="reference", lpips=w), make(5, schedule="reference", lpips=w), make(6, schedule="reference", lpips=w)
    sa = [LP.draw_face_patch(a.rng) for _ in range(50)]
    assert sa == [LP.draw_face_patch(b.rng) for _ in range(50)]
    assert sa != [LP.draw_face_patch(c.rng) for _ in range(50)]
    assert a.lpips_on(7501) and not a.lpips_on(7500)
    assert not make(5, schedule="reference").lpips_on(9000)            # no weights: off
    assert not make(5, lpips=w).lpips_on(9000)                          # the C3 schedule has no late phase
    # the phase description is untouched by the term
    assert face_phase(7600) == FacePhase(align=True, warm=True, hair_mask_iter=False, priors=True, prior_depth=True)
