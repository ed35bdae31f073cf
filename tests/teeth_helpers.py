"""Shared by the teeth-segmentation tests and tests/golden/make_golden_teeth.py (golden G15).

G15 stores no weights (the fpn-fp segmentor has 28.6 M of them).  One seeded rule -- ``FPNWeights.random``: He-scaled
convolutions, ``conv3`` of every bottleneck halved, the neck's convolutions at 0.7 with biases of 0.1, BatchNorm gamma
and variance in [0.5, 1.5], beta and running mean of about 0.2, ``conv_seg``'s rows centred -- gives the state dict
under the keys of fpn-fp-512.pth; the generator loads it into the reference's own modules, the tests into
``FPNWeights``.  Under it between a fifth and four fifths of every stage's units are active, at least five labels occur
in a 64 x 96 frame and class 7 (teeth) takes between 0.2 % and 50 % of its pixels."""
from tests import segnet_helpers as S
from tests.segnet_helpers import liveness, seeded_frames, top_two_margin  # noqa: F401 (re-exported)

SEED = 15
G15_H, G15_W = 64, 96


def state_dict(seed: int = SEED):
    from instag_amd.teeth import FPNWeights
    return FPNWeights.random(seed).state_dict()


def weights(seed: int = SEED):
    from instag_amd.teeth import FPNWeights
    return FPNWeights.from_state_dict(state_dict(seed))


def reference_fp64(weights_, frames_u8):
    """segnet_helpers.reference_fp64 of the segmenter: logits at 1/4 resolution."""
    from instag_amd import teeth as T
    return S.reference_fp64(T, T.fpn_torch, weights_, frames_u8)
