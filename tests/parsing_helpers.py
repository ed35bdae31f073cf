"""Shared by the face-parsing tests and tests/golden/make_golden_parsing.py (golden G14).

G14 stores no weights (BiSeNet has 13.3 M of them).  One seeded rule -- ``BiSeNetWeights.random``: He-scaled
convolutions, BatchNorm gamma and variance in [0.5, 1.5], beta and running mean of about 0.2 -- gives the state dict
under the keys of 79999_iter.pth; the generator loads it into the reference's own module, the tests into
``BiSeNetWeights``.  Under it between a fifth and four fifths of every stage's units are active and at least five labels
occur in a 64 x 96 frame."""
import numpy as np
import torch

SEED = 14
G14_H, G14_W = 64, 96


def state_dict(seed: int = SEED):
    from instag_amd.parsing import BiSeNetWeights
    return BiSeNetWeights.random(seed).state_dict()


def weights(seed: int = SEED):
    from instag_amd.parsing import BiSeNetWeights
    return BiSeNetWeights.from_state_dict(state_dict(seed))


def weights_with_background(offset: float = 0.01, seed: int = SEED):
    """The seeded rule with ``offset`` added to the background row of the classifier: its inputs are all positive, so
    class 0 gains everywhere and wins about two thirds of a frame -- what extract_background needs (pixels farther than
    5 from any foreground) and the centred rule does not give."""
    from instag_amd.parsing import BiSeNetWeights
    sd = state_dict(seed)
    w = sd["conv_out.conv_out.weight"].clone()
    w[0] += offset
    sd["conv_out.conv_out.weight"] = w
    return BiSeNetWeights.from_state_dict(sd)


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


def reference_fp64(weights_, frames_u8):
    """The fp64 statement on the CPU: logits at 1/8 resolution, the full-size logits, the labels, and e32 of the fp32
    statement against it (relative to the largest fp64 logit)."""
    from instag_amd import parsing as P
    H, W = frames_u8.shape[1:3]
    with torch.no_grad():
        want8 = P.bisenet_torch(weights_, P.normalise(frames_u8, torch.float64))
        full = P.upsample_torch(want8, H, W)
        got32 = P.bisenet_torch(weights_, P.normalise(frames_u8, torch.float32))
    scale = float(want8.abs().max())
    e32 = float((got32.double() - want8).abs().max()) / scale
    return want8, full, P.first_argmax(full), e32, scale


def top_two_margin(full):
    """[B,C,H,W] -> [B,H,W]: the largest minus the second largest entry over C."""
    top = full.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def numpy_resize_index(n_dst: int, n_src: int):
    return np.minimum((np.arange(n_dst, dtype=np.int64) * n_src) // n_dst, n_src - 1)
