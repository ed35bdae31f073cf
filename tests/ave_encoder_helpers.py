"""Shared by the AudioEncoder tests and tests/golden/make_golden_ave_encoder.py (golden G9).

G9 stores no weights (the encoder has 2.8 M of them).  One seeded rule -- ``AudioEncoderWeights.random``: He-scaled
convolutions, biases of about 0.1, BatchNorm gamma and variance in [0.5, 1.5], beta and running mean of about 0.2 --
gives the state dict in the keys of audio_visual_encoder.pth; the generator loads it into the reference's module through
the reference's own key mapping, the tests into ``AudioEncoderWeights``.  Under it about half of every layer's units are
active and fp32 torch on the CPU is within 1e-6 of the fp64 result, relative to the largest output."""
import torch

SEED = 9
G9_T = 40                     # mel frames of golden G9: n = 9 windows, the last one clamped to start 24


def state_dict(seed: int = SEED):
    from instag_amd.ave_encoder import AudioEncoderWeights
    return AudioEncoderWeights.random(seed).state_dict()


def weights(seed: int = SEED):
    from instag_amd.ave_encoder import AudioEncoderWeights
    return AudioEncoderWeights.from_state_dict(state_dict(seed))


def seeded_mel(T: int, seed: int = 0) -> torch.Tensor:
    """[T,80] fp32 spread over the whole normalized range [-4, 4] with both clip values present, in quarter-integers
    (exact in fp16)."""
    g = torch.Generator().manual_seed(1234 + seed)
    mel = ((torch.rand(T, 80, generator=g) * 9.0 - 4.5) * 4).round() / 4
    mel = mel.clamp(-4.0, 4.0)
    assert float(mel.min()) == -4.0 and float(mel.max()) == 4.0
    return mel


def reference_starts(T: int):
    """AudDataset.__init__ / crop_audio_window (utils/audio_utils.py:125, 135-141) transcribed: the first mel frame of
    every window of a [T, 80] mel."""
    data_len = int((T - 16) / 80. * float(25)) + 2
    starts = []
    for start_frame_num in range(data_len):
        start_idx = int(80. * (start_frame_num / float(25)))
        end_idx = start_idx + 16
        if end_idx > T:
            end_idx = T
            start_idx = end_idx - 16
        starts.append(start_idx)
    return starts


def reference_windows(mel: torch.Tensor) -> torch.Tensor:
    """AudDataset.__getitem__ for every index: [n,1,80,16]."""
    return torch.stack([mel[s:s + 16, :].T.unsqueeze(0) for s in reference_starts(mel.shape[0])])


def liveness(taps):
    """Fraction of positive units per block output."""
    return [float((t > 0).double().mean()) for t in taps]
