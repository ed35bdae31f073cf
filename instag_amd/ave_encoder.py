"""From a wav to the frames of an 'ave' head: the mel front end and the AudioEncoder of the 'ave' audio extractor.

What scene/dataset_readers.py:111-142 does for every clip it synthesizes: the mel spectrogram of the 16 kHz audio
(utils/audio_utils.py:86-117), one [1,80,16] window per video frame (utils/audio_utils.py:120-155), the frozen
``AudioEncoder`` (scene/motion_net.py:8-25, 102-129; weights ``data_utils/audio_visual_encoder.pth``) on every window,
the first and last row repeated twice, and per frame the eight rows around it (utils/audio_utils.py:38-73).

    w = AudioEncoderWeights.load("audio_visual_encoder.pth")      # the file a user of the reference already has
    feats = ave_features(load_wav16k("aud.wav"), w, "cuda")        # [n+4, 512, 1], what the reference saves as aud_ave.npy
    auds = frame_window(feats, idx)                                # [8, 1, 512]: talking_dict["auds"] of frame idx

On the GPU the encoder runs in csrc/ave_encoder.hip (inference only, as the reference runs it); ``audio_encoder_torch``
is the plain-torch statement of the same arithmetic (any dtype, CPU or GPU) that the tests compare against and the CPU
path uses.  The mel front end is plumbing and runs in torch on either device.  The project ships no weights and
fetches none.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import convnet
from .convnet import BN_EPS
from .device_op import DeviceOperator

# (cin, cout, kernel, (stride_h, stride_w), padding, residual): scene/motion_net.py:106-123
LAYERS = (
    (1, 32, 3, (1, 1), 1, False), (32, 32, 3, (1, 1), 1, True), (32, 32, 3, (1, 1), 1, True),
    (32, 64, 3, (3, 1), 1, False), (64, 64, 3, (1, 1), 1, True), (64, 64, 3, (1, 1), 1, True),
    (64, 128, 3, (3, 3), 1, False), (128, 128, 3, (1, 1), 1, True), (128, 128, 3, (1, 1), 1, True),
    (128, 256, 3, (3, 2), 1, False), (256, 256, 3, (1, 1), 1, True),
    (256, 512, 3, (1, 1), 0, False), (512, 512, 1, (1, 1), 0, False),
)
N_MELS, WINDOW, DIM_OUT = 80, 16, 512
FPS, MEL_PER_SECOND = 25., 80.                       # utils/audio_utils.py:125,135
MACS_PER_WINDOW = sum(ci * co * k * k * ho * wo for (ci, co, k, _, _, _), (ho, wo) in zip(
    LAYERS, ((80, 16),) * 3 + ((27, 16),) * 3 + ((9, 6),) * 3 + ((3, 3),) * 2 + ((1, 1),) * 2))

# convnet's table: block i is ``{i}.conv_block.0`` (convolution, with a bias) and ``{i}.conv_block.1`` (BatchNorm)
_TABLE = tuple((f"{i}.conv_block.0", f"{i}.conv_block.1", True, ci, co, k, stride)
               for i, (ci, co, k, stride, _, _) in enumerate(LAYERS))


# ---- weights ----------------------------------------------------------------------------------------------------------
class AudioEncoderWeights(convnet.ConvWeights):
    """The frozen parameters: per layer the convolution's weight and bias and BatchNorm's gamma, beta, running mean and
    running variance (convnet.ConvWeights).  On the device the first layer stays as stored, [32][9]."""

    TABLE, LABEL, STRUCT, COUT_MAJOR = _TABLE, "AudioEncoder weights", "AveEncoderWeights", (0,)

    @staticmethod
    def _layer_name(l):
        return f"layer {l}"

    @classmethod
    def from_state_dict(cls, sd) -> "AudioEncoderWeights":
        """``sd``: the keys of audio_visual_encoder.pth as shipped, ``{i}.conv_block.{0,1}.*``, or the
        ``audio_encoder.``-prefixed form dataset_readers.py:118 builds (``AudioEncoder().state_dict()``)."""
        prefix = "audio_encoder." if any(k.startswith("audio_encoder.") for k in sd) else ""
        return cls._read({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, lambda l, key: KeyError(
            f"AudioEncoder weights: layer {l} misses {prefix + key!r}"))

    @classmethod
    def random(cls, seed: int = 0) -> "AudioEncoderWeights":
        """Seeded stand-ins with the scale of trained ones (tests, benches; convnet.draw_layer), so that the fold is
        exercised and about half of every layer's units are active."""
        g = torch.Generator().manual_seed(seed)
        return cls([convnet.draw_layer(g, row) for row in _TABLE])

    def state_dict(self, prefix: str = ""):
        """The keys of the shipped file (``prefix="audio_encoder."``: those of the reference module)."""
        return {f"{prefix}{key}": lay[f].clone() for lay, row in zip(self.layers, _TABLE) for f, key in convnet.keys(row)}

    def to(self, device=None, dtype=None):
        """The list of per-layer dicts as tensors of ``device`` / ``dtype`` for the torch statement."""
        return list(super().to(device, dtype).values())


# ---- plain-torch statement -------------------------------------------------------------------------------------------
def audio_encoder_torch(weights: AudioEncoderWeights, windows, taps=None):
    """AudioEncoder.forward in eval mode for ``windows`` [B,1,80,16] -> [B,512]: every block is
    ReLU(BatchNorm(conv(x) + b) [+ x]), BatchNorm not folded.  ``taps``: a list that receives every block's output."""
    x = windows
    for lay, (_, _, _, stride, pad, residual) in zip(weights.to(x.device, x.dtype), LAYERS):
        y = F.conv2d(x, lay["weight"], lay["bias"], stride=stride, padding=pad)
        y = F.batch_norm(y, lay["mean"], lay["var"], lay["gamma"], lay["beta"], training=False, eps=BN_EPS)
        x = F.relu(y + x if residual else y)
        if taps is not None:
            taps.append(x)
    return x.squeeze(2).squeeze(2)


# ---- windows ---------------------------------------------------------------------------------------------------------
def window_starts(T: int) -> torch.Tensor:
    """First mel frame of every window of a [T,80] mel (AudDataset, utils/audio_utils.py:120-155): int32 [n] with
    n = int((T - 16) / 80 * 25) + 2, start_i = int(80 * (i / 25)), moved back to T - 16 where the window would pass the
    end.  Window i is mel[start_i : start_i + 16, :].T."""
    T = int(T)
    if T < WINDOW:
        raise ValueError(f"a mel of {T} frames holds no window of {WINDOW}")
    n = int((T - WINDOW) / MEL_PER_SECOND * float(FPS)) + 2
    starts = np.floor(MEL_PER_SECOND * (np.arange(n, dtype=np.float64) / float(FPS))).astype(np.int64)
    starts = np.where(starts + WINDOW > T, T - WINDOW, starts)
    return torch.from_numpy(starts.astype(np.int32))


def cut_windows(mel, starts=None):
    """[n,1,80,16] windows of mel [T,80] (materialised: the torch path; the HIP operator reads the mel in place)."""
    if starts is None:
        starts = window_starts(mel.shape[0])
    idx = starts.to(mel.device).long()[:, None] + torch.arange(WINDOW, device=mel.device)[None]
    return mel[idx].permute(0, 2, 1).unsqueeze(1)


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class AudioEncoder(DeviceOperator):
    """``encode(mel [T,80]) -> [n,512]`` and ``encode_windows([B,1,80,16]) -> [B,512]``, fp32 on ``device``, on
    torch's current stream; inference only (no autograd node), as the reference runs the network.  On the GPU the windows
    go through csrc/ave_encoder.hip in chunks of at most ``max_batch`` with the one kept workspace of
    device_op.DeviceOperator, so memory does not grow with the clip; on the CPU both are the torch statement.  The
    workspace's size depends on the batch alone and never decreases as it grows (two buffers of ``buffer_floats`` of
    csrc/ave_encoder.hip: the batch times a constant, rounded up to 64 floats), so a workspace kept by its bytes is
    replaced exactly when one kept by its batch would have been too small."""

    CHECK = "check"

    def __init__(self, weights: AudioEncoderWeights, device="cuda"):
        super().__init__(weights, device)
        if self.device.type == "cuda":
            self.max_batch = int(self._L.instag_ave_encoder_max_batch())

    def _forward(self, src, T, starts, n):
        from . import _lib
        out = torch.empty(n, DIM_OUT, dtype=torch.float32, device=self.device)
        nbytes = _lib.workspace_bytes(self._L.instag_ave_encoder_workspace_bytes(min(n, self.max_batch)))
        self._each_chunk(n, nbytes, lambda c, m, ws, size: self._L.instag_ave_encoder_forward(
            C.byref(self._struct), _lib.ptr(src if starts is not None else src[c]), int(T),
            _lib.ptr(None if starts is None else starts[c]), m, _lib.ptr(out[c]), ws, size, _lib.current_stream()),
            "ave_encoder_forward")
        return out

    @torch.no_grad()
    def encode_windows(self, windows):
        if windows.dim() != 4 or tuple(windows.shape[1:]) != (1, N_MELS, WINDOW):
            raise ValueError(f"AudioEncoder: windows [B,1,{N_MELS},{WINDOW}], got {tuple(windows.shape)}")
        windows = windows.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if self.device.type != "cuda":
            return audio_encoder_torch(self.weights, windows)
        if windows.shape[0] == 0:
            return torch.empty(0, DIM_OUT, dtype=torch.float32, device=self.device)
        return self._forward(windows, 0, None, windows.shape[0])

    @torch.no_grad()
    def encode(self, mel):
        if mel.dim() != 2 or mel.shape[1] != N_MELS:
            raise ValueError(f"AudioEncoder: mel [T,{N_MELS}], got {tuple(mel.shape)}")
        starts = window_starts(mel.shape[0])
        mel = mel.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if self.device.type != "cuda":
            return audio_encoder_torch(self.weights, cut_windows(mel, starts))
        return self._forward(mel, mel.shape[0], starts.to(self.device), starts.numel())


# ---- features and frames ---------------------------------------------------------------------------------------------
def ave_features(mel_or_wav, weights: AudioEncoderWeights, device="cuda", encoder=None) -> np.ndarray:
    """The array dataset_readers.py:129-142 saves as aud_ave.npy, fp32 [n+4, 512, 1]: the encoder on every window, the
    first and the last row repeated twice.  ``mel_or_wav``: a normalized mel [T,80] or 16 kHz samples [L] (numpy or
    torch).  ``encoder`` (default: the torch statement) is called as ``encoder(weights, windows)`` in place of the HIP
    operator -- the tests' comparand."""
    x = torch.as_tensor(mel_or_wav)
    device = torch.device(device)
    mel = melspectrogram(x.to(device)) if x.dim() == 1 else x.to(device=device, dtype=torch.float32)
    if encoder is not None:
        with torch.no_grad():
            out = encoder(weights, cut_windows(mel))
    else:
        out = AudioEncoder(weights, device).encode(mel)
    out = out.float().cpu()
    feats = torch.cat([out[:1].repeat(2, 1), out, out[-1:].repeat(2, 1)], dim=0)
    return feats.unsqueeze(0).permute(1, 2, 0).contiguous().numpy()


def frame_window(features, idx: int) -> torch.Tensor:
    """``get_audio_features(features.permute(0, 2, 1), 2, idx)`` (utils/audio_utils.py:38-73) for ``features``
    [N,512,1] (ave_features' array): the eight rows idx - 4 .. idx + 3, zeros where they fall outside -> [8,1,512],
    the window make_frame / frame_codes take as ``auds``."""
    f = torch.as_tensor(features).float().permute(0, 2, 1)
    left, right = idx - 4, idx + 4
    pad_left, pad_right = max(0, -left), max(0, right - f.shape[0])
    auds = f[max(left, 0):min(right, f.shape[0])]
    if pad_left > 0:
        auds = torch.cat([torch.zeros_like(auds[:pad_left]), auds], dim=0)
    if pad_right > 0:
        auds = torch.cat([auds, torch.zeros_like(auds[:pad_right])], dim=0)
    return auds


# ---- mel front end (utils/audio_utils.py:82-117) ----------------------------------------------------------------------
SAMPLE_RATE, N_FFT, HOP = 16000, 800, 200
FMIN, FMAX = 55.0, 7600.0
PREEMPHASIS = 0.97
_F_SP, _MIN_LOG_HZ, _LOGSTEP = 200.0 / 3, 1000.0, math.log(6.4) / 27.0


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_HZ / _F_SP + np.log(np.maximum(f, 1e-30) / _MIN_LOG_HZ) / _LOGSTEP,
                    f / _F_SP)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= _MIN_LOG_HZ / _F_SP, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_HZ / _F_SP)), _F_SP * m)


def mel_basis() -> np.ndarray:
    """librosa.filters.mel(sr=16000, n_fft=800, n_mels=80, fmin=55, fmax=7600) restated, fp64 [80,401]: the Slaney mel
    scale, triangles between neighbouring band centres over the bins linspace(0, 8000, 401), each scaled by
    2 / (its width in Hz) (Slaney's area normalisation)."""
    freqs = np.linspace(0.0, SAMPLE_RATE / 2, N_FFT // 2 + 1)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(FMIN), _hz_to_mel(FMAX), N_MELS + 2))
    ramps = pts[:, None] - freqs[None, :]
    diff = np.diff(pts)
    lower = -ramps[:-2] / diff[:-1, None]
    upper = ramps[2:] / diff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (pts[2:] - pts[:-2]))[:, None]


def melspectrogram(wav16k, pad_mode: str = "constant") -> torch.Tensor:
    """utils/audio_utils.py:86-117 for 16 kHz samples [L] -> the normalized mel [T = 1 + L // 200, 80], fp32 on the
    samples' device: pre-emphasis 0.97, the centred STFT (n_fft = win = 800, hop 200, periodic Hann; ``pad_mode`` is
    librosa.stft's, "constant" since librosa 0.10, "reflect" before), |D| through the mel basis,
    20 log10(max(1e-5, .)) - 20, clip(8 (S + 100) / 100 - 4, -4, 4).  Computed in fp64."""
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"melspectrogram: pad_mode 'constant' or 'reflect', got {pad_mode!r}")
    x = torch.as_tensor(wav16k)
    if x.dim() != 1 or x.numel() == 0:
        raise ValueError(f"melspectrogram: samples [L], got {tuple(x.shape)}")
    x = x.double()
    y = x.clone()
    y[1:] -= PREEMPHASIS * x[:-1]
    window = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64, device=x.device)
    D = torch.stft(y, N_FFT, hop_length=HOP, win_length=N_FFT, window=window, center=True, pad_mode=pad_mode,
                   return_complex=True)                                            # [401, T]
    S = torch.from_numpy(mel_basis()).to(x.device) @ D.abs()
    S = 20.0 * torch.log10(torch.clamp(S, min=1e-5)) - 20.0
    return torch.clamp(8.0 * ((S + 100.0) / 100.0) - 4.0, -4.0, 4.0).t().contiguous().float()


def load_wav16k(path) -> torch.Tensor:
    """The samples of a 16 kHz PCM wav (8, 16, 24 or 32 bit) as fp32 [L] in [-1, 1], the channels averaged.  Any
    other rate raises: resampling is not provided (the reference's preprocessing writes aud.wav at 16 kHz)."""
    import wave
    with wave.open(str(path), "rb") as f:
        rate, width, channels = f.getframerate(), f.getsampwidth(), f.getnchannels()
        if rate != SAMPLE_RATE:
            raise ValueError(f"{path}: sample rate {rate} Hz, expected {SAMPLE_RATE} Hz (resample the audio first)")
        raw = f.readframes(f.getnframes())
    if width == 1:
        data = (np.frombuffer(raw, dtype=np.uint8).astype(np.float64) - 128.0) / 128.0
    elif width == 2:
        data = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        data = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float64) / float(1 << 23)
    elif width == 4:
        data = np.frombuffer(raw, dtype="<i4").astype(np.float64) / float(1 << 31)
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples are not PCM this reader knows")
    return torch.from_numpy(data.reshape(-1, channels).mean(axis=1).astype(np.float32))
