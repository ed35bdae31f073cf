"""Shared by the face-parsing tests and tests/golden/make_golden_parsing.py (golden G14).

G14 stores no weights (BiSeNet has 13.3 M of them).  One seeded rule -- ``BiSeNetWeights.random``: He-scaled
convolutions, BatchNorm gamma and variance in [0.5, 1.5], beta and running mean of about 0.2 -- gives the state dict
under the keys of 79999_iter.pth; the generator loads it into the reference's own module, the tests into
``BiSeNetWeights``.  Under it between a fifth and four fifths of every stage's units are active and at least five labels
occur in a 64 x 96 frame."""
import numpy as np

from tests import segnet_helpers as S
from tests.segnet_helpers import liveness, seeded_frames, top_two_margin  # noqa: F401 (re-exported)

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


def reference_fp64(weights_, frames_u8):
    """segnet_helpers.reference_fp64 of the parser: logits at 1/8 resolution."""
    from instag_amd import parsing as P
    return S.reference_fp64(P, P.bisenet_torch, weights_, frames_u8)


def numpy_resize_index(n_dst: int, n_src: int):
    return np.minimum((np.arange(n_dst, dtype=np.int64) * n_src) // n_dst, n_src - 1)
