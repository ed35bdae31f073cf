"""Shared by the tests of the two segmentation networks (face parsing, teeth): seeded frames, the fp64 reference, and
the logits check of the GPU tests."""
import torch

FACTOR = 8.0                  # the operator's logits are within FACTOR x e32 of the fp64 statement's


def seeded_frames(B: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """u8 [B,H,W,3]: a smooth ramp per channel plus blocks of noise, every frame different, both 0 and 255 present."""
    g = torch.Generator().manual_seed(4321 + seed)
    y = torch.linspace(0, 1, H).view(1, H, 1, 1)
    x = torch.linspace(0, 1, W).view(1, 1, W, 1)
    phase = torch.rand(B, 1, 1, 3, generator=g) * 6.28
    ramp = 0.5 + 0.5 * torch.sin(6.28 * (y * (1 + torch.arange(3).view(1, 1, 1, 3)) + x * 2) + phase)
    noise = torch.rand(B, H, W, 3, generator=g)
    img = (255 * (0.6 * ramp + 0.4 * noise)).round().clamp(0, 255).to(torch.uint8)
    img[:, 0, 0, :] = 0
    img[:, -1, -1, :] = 255
    return img


def liveness(taps):
    """Fraction of positive units per stage output."""
    return [float((t > 0).double().mean()) for t in taps]


def top_two_margin(full):
    """[B,C,H,W] -> [B,H,W]: the largest minus the second largest entry over C."""
    top = full.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def reference_fp64(module, net_torch, weights_, frames_u8):
    """The fp64 statement of ``module`` (instag_amd.parsing or .teeth) on the CPU: the network's logits, the full-size
    logits, the labels, e32 of the fp32 statement against it (relative to the largest fp64 logit), and that largest
    logit."""
    H, W = frames_u8.shape[1:3]
    with torch.no_grad():
        want = net_torch(weights_, module.normalise(frames_u8, torch.float64))
        full = module.upsample_torch(want, H, W)
        got32 = net_torch(weights_, module.normalise(frames_u8, torch.float32))
    scale = float(want.abs().max())
    e32 = float((got32.double() - want).abs().max()) / scale
    return want, full, module.first_argmax(full), e32, scale


def case(reference, weights, frames):
    """A GPU test's case: ``reference(weights, frames)`` (a helper module's ``reference_fp64``) and the flip-risk
    pixels, whose top-two margin is below 2 x FACTOR x e32 x scale."""
    want, full, labels, e32, scale = reference(weights, frames)
    assert 1e-8 < e32 < 2e-5, e32
    risk = top_two_margin(full) < 2.0 * FACTOR * e32 * scale
    return dict(weights=weights, frames=frames, want=want, labels=labels, e32=e32, scale=scale, risk=risk)


def check_logits(name, got, c):
    err = float((got.detach().double().cpu() - c["want"]).abs().max()) / c["scale"]
    print(f"{name}: operator {err:.3e} e32 {c['e32']:.3e} bar {FACTOR * c['e32']:.3e} scale {c['scale']:.3e}")
    assert tuple(got.shape) == tuple(c["want"].shape) and got.dtype == torch.float32 and got.is_cuda
    assert err <= FACTOR * c["e32"], (name, err, c["e32"])
