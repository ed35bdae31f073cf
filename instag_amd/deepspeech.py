"""From a wav to the audio features of a 'deepspeech' head: DeepSpeech 0.1.0 and the procedure around it.

What data_utils/deepspeech_features/ of the reference does with TensorFlow 1.x, python_speech_features and the frozen
graph ``deepspeech-0_1_0-b90017e8.pb``: the 16 kHz audio becomes 26 MFCCs per 10 ms, every second frame with nine
frames of context on each side is one input row [494], normalised over the whole array; the network (three clipped-ReLU
layers, one bidirectional LSTM of 2048 cells, one more clipped-ReLU layer, a linear layer) gives 29 raw logits per row,
50 rows a second; they are interpolated to the video's 50 frames a second and cut into windows of 16 around every
second row, which it saves as aud_ds.npy.

    w = DeepSpeechWeights.load("deepspeech-0_1_0-b90017e8.pb")      # the file a user of the reference already has
    feats = deepspeech_features(load_wav16k("aud.wav"), w, "cuda")  # fp64 [W, 16, 29]
    store, meta = open_identity("data/May", "train", "cuda", audio_extractor="deepspeech", audio_features=feats)

On the GPU the network runs in csrc/deepspeech.hip (fp32, inference only): the dense layers on the MFMA GEMM of the
wav2vec network, the recurrence as one launch per time step.  ``deepspeech_torch`` is the plain-torch statement of the
same arithmetic (any dtype, CPU or GPU) that the tests compare against and a CPU device runs.  The project ships no
weights and fetches none.

What is said here about the graph -- the layers, the gate order i, j, f, o, the forget bias of 1, the clip at 20, the
names of its constants -- is written from knowledge of the model, not read from the file: neither the .pb nor
TensorFlow was at hand, and no test compares with a TensorFlow run.  The MFCC front end restates
``python_speech_features.mfcc`` from its published source for the same reason.
"""
from __future__ import annotations

import ctypes as C
import math
import mmap
import os
from dataclasses import asdict, dataclass

import numpy as np
import torch

from .device_op import DeviceOperator

SAMPLE_RATE = 16000
FRAME_LEN, FRAME_STEP, N_FFT = 400, 160, 512             # mfcc: winlen 0.025 s, winstep 0.01 s, nfft 512
N_FILT, N_CEP, PREEMPHASIS, LIFTER = 26, 26, 0.97, 22
N_CONTEXT = 9
NET_RATE = VIDEO_RATE = 50
WINDOW, WINDOW_PAD, WINDOW_STRIDE = 16, 8, 2
WORKSPACE_LIMIT = 1 << 30
EPS = float(np.finfo(np.float64).eps)

DENSE_NAMES = ("h1", "b1", "h2", "b2", "h3", "b3", "h5", "b5", "h6", "b6")
LSTM_NAMES = ("fw_kernel", "fw_bias", "bw_kernel", "bw_bias")


# ---- the procedure (deepspeech_features.py), host arithmetic ---------------------------------------------------------
def n_frames(n_samples: int) -> int:
    """F of ``mfcc_features``: 1 if L <= 400, else 1 + ceil((L - 400) / 160)."""
    L = int(n_samples)
    return 1 if L <= FRAME_LEN else 1 + -(-(L - FRAME_LEN) // FRAME_STEP)


def n_steps(n_samples: int) -> int:
    """S of ``input_vectors``: every second MFCC frame, ceil(F / 2)."""
    return -(-n_frames(n_samples) // 2)


def n_rows(n_samples: int) -> int:
    """N of ``interpolate``: int(round(seconds * 50)) with Python's round (half to even)."""
    return int(round(float(int(n_samples)) / SAMPLE_RATE * VIDEO_RATE))


def n_windows(n_samples: int) -> int:
    """W of ``windows`` on N rows: ceil((N - 1) / 2)."""
    return max(0, -(-(n_rows(n_samples) - 1) // 2))


def mel_bins() -> np.ndarray:
    """The 28 FFT bins of the filterbank's corners: equally spaced in mel = 2595 log10(1 + f / 700) over 0 .. 8000 Hz,
    bin = floor(513 hz / 16000)."""
    high = 2595.0 * np.log10(1.0 + (SAMPLE_RATE / 2) / 700.0)
    mel = np.linspace(0.0, high, N_FILT + 2)
    return np.floor((N_FFT + 1) * (700.0 * (10.0 ** (mel / 2595.0) - 1.0)) / SAMPLE_RATE)


def filterbank() -> np.ndarray:
    """fp64 [26, 257]: filter j rises (i - bin[j]) / (bin[j+1] - bin[j]) on [bin[j], bin[j+1]) and falls
    (bin[j+2] - i) / (bin[j+2] - bin[j+1]) on [bin[j+1], bin[j+2])."""
    b = mel_bins()
    fb = np.zeros((N_FILT, N_FFT // 2 + 1))
    for j in range(N_FILT):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def dct_matrix(n: int = N_FILT) -> np.ndarray:
    """D [n, n] with x @ D = the DCT-II of x with norm='ortho' (scipy.fftpack.dct(x, type=2, norm='ortho'))."""
    k, m = np.arange(n)[None, :], np.arange(n)[:, None]
    D = 2.0 * np.cos(np.pi * k * (2 * m + 1) / (2.0 * n)) * math.sqrt(1.0 / (2.0 * n))
    D[:, 0] *= math.sqrt(0.5)
    return D


def mfcc_features(wav_int16) -> np.ndarray:
    """``python_speech_features.mfcc(signal, 16000, numcep=26)`` at its defaults, int16 samples [L] -> fp64 [F, 26].
    That package is not a dependency: this restatement is the definition here.  Pre-emphasis 0.97, frames of 400 at
    step 160 with a rectangular window over the zero-padded signal, |rfft(512)|^2 / 512, 26 triangular mel filters,
    zeros -> eps, log, DCT-II 'ortho', the lifter 1 + 11 sin(pi n / 22), and coefficient 0 replaced by the log of the
    frame's energy (the sum of its power spectrum, zeros -> eps)."""
    s = np.asarray(wav_int16)
    if s.ndim != 1 or s.shape[0] < 1:
        raise ValueError(f"mfcc_features: samples [L >= 1], got {s.shape}")
    s = s.astype(np.float64)
    s = np.append(s[0], s[1:] - PREEMPHASIS * s[:-1])
    F = n_frames(s.shape[0])
    padded = np.concatenate([s, np.zeros((F - 1) * FRAME_STEP + FRAME_LEN - s.shape[0])])
    idx = FRAME_STEP * np.arange(F)[:, None] + np.arange(FRAME_LEN)[None, :]
    power = np.abs(np.fft.rfft(padded[idx], N_FFT)) ** 2 / N_FFT
    energy = power.sum(axis=1)
    energy = np.where(energy == 0, EPS, energy)
    feat = power @ filterbank().T
    feat = np.log(np.where(feat == 0, EPS, feat)) @ dct_matrix(N_FILT)
    feat = feat[:, :N_CEP] * (1.0 + (LIFTER / 2.0) * np.sin(np.pi * np.arange(N_CEP) / LIFTER))
    feat[:, 0] = np.log(energy)
    return feat


def input_vectors(wav_int16) -> np.ndarray:
    """``conv_audio_to_deepspeech_input_vector``: every second MFCC row, nine zero rows in front and behind, row t =
    rows t .. t + 18 flattened, minus the mean and over the population standard deviation of the whole array ->
    fp32 [S, 494] (the arithmetic in fp64, one rounding)."""
    feat = mfcc_features(wav_int16)[::2]
    S = feat.shape[0]
    pad = np.zeros((N_CONTEXT, N_CEP))
    feat = np.concatenate([pad, feat, pad])
    rows = feat[np.arange(S)[:, None] + np.arange(2 * N_CONTEXT + 1)[None, :]].reshape(S, -1)
    return ((rows - rows.mean()) / rows.std()).astype(np.float32)


def interpolate(logits, n_samples: int) -> np.ndarray:
    """``interpolate_features`` as process.py reaches it (no frame count given, both rates 50): [S, V] ->
    fp64 [N, V], N = int(round(n_samples / 16000 * 50)), by np.interp, which repeats the end rows outside."""
    y = np.asarray(logits, dtype=np.float64)
    N = n_rows(n_samples)
    xp, x = np.arange(y.shape[0]) / float(NET_RATE), np.arange(N) / float(VIDEO_RATE)
    out = np.zeros((N, y.shape[1]))
    for v in range(y.shape[1]):
        out[:, v] = np.interp(x, xp, y[:, v])
    return out


def windows(rows) -> np.ndarray:
    """Both windowing loops of the reference as they stand, [N, V] -> fp64 [W, 16, V]: the size-1, stride-1 loop keeps
    the first N - 1 rows; eight zero rows go on each end; windows of 16 start at range(0, (N - 1 + 16) - 16, 2)."""
    r = np.asarray(rows, dtype=np.float64)
    r = r[:max(r.shape[0] - 1, 0)]
    pad = np.zeros((WINDOW_PAD, r.shape[1]))
    r = np.concatenate([pad, r, pad])
    starts = np.arange(0, r.shape[0] - WINDOW, WINDOW_STRIDE)
    return r[starts[:, None] + np.arange(WINDOW)[None, :]]


def to_int16(wav16k) -> np.ndarray:
    """What the reference holds after ``wavfile.read(...).astype(np.float32).astype(np.int16)``, from samples in
    [-1, 1] as ``load_wav16k`` gives them: times 32768, clamped to [-32768, 32767], truncated towards zero (exact for
    a 16-bit wav)."""
    x = np.asarray(torch.as_tensor(wav16k).detach().cpu().numpy(), dtype=np.float64) * 32768.0
    return np.clip(x, -32768.0, 32767.0).astype(np.int16)


# ---- dimensions and weights -------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class DeepSpeechDims:
    """The dimensions of the network.  The default is DeepSpeech 0.1.0."""
    n_in: int = 494
    hidden: int = 2048
    cell: int = 2048
    n_out: int = 29
    clip: float = 20.0
    forget_bias: float = 1.0

    def check(self) -> "DeepSpeechDims":
        """The shapes csrc/deepspeech.hip takes (include/instag_deepspeech.h); ValueError naming the field otherwise."""
        from . import _lib
        max_cell = _lib.DEEPSPEECH["INSTAG_DEEPSPEECH_MAX_CELL"]
        rules = (
            ("n_in", 1 <= self.n_in <= 4096, "in [1, 4096]"),
            ("hidden", 32 <= self.hidden <= 4096 and self.hidden % 32 == 0, "a multiple of 32 in [32, 4096] (the GEMM's K tile)"),
            ("cell", 256 <= self.cell <= max_cell and self.cell % 256 == 0,
             f"a multiple of 256 in [256, {max_cell}] (a lane of the step kernel loads 16 bytes of every 256 floats)"),
            ("n_out", 1 <= self.n_out <= 1024, "in [1, 1024]"),
            ("clip", self.clip > 0, "positive"),
        )
        for field, ok, rule in rules:
            if not ok:
                raise ValueError(f"DeepSpeech dims: {field} = {getattr(self, field)} is not supported: {rule}")
        return self

    def shapes(self) -> dict:
        d = self
        out = {"h1": (d.n_in, d.hidden), "h2": (d.hidden, d.hidden), "h3": (d.hidden, d.hidden),
               "h5": (2 * d.cell, d.hidden), "h6": (d.hidden, d.n_out), "b6": (d.n_out,)}
        out.update({b: (d.hidden,) for b in ("b1", "b2", "b3", "b5")})
        for p in ("fw", "bw"):
            out[p + "_kernel"], out[p + "_bias"] = (d.hidden + d.cell, 4 * d.cell), (4 * d.cell,)
        return out


# -- a reader of the protobuf wire format, as much of it as a frozen GraphDef of Const nodes needs
def _varint(buf, pos):
    value, shift = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        value |= (b & 0x7F) << shift
        if b < 0x80:
            return value, pos
        shift += 7


def _fields(buf, pos, end):
    """(field number, wire type, value) of a message in buf[pos:end]: an int for varints, (start, end) for the others."""
    while pos < end:
        key, pos = _varint(buf, pos)
        number, kind = key >> 3, key & 7
        if kind == 0:
            value, pos = _varint(buf, pos)
        elif kind == 1:
            value, pos = (pos, pos + 8), pos + 8
        elif kind == 2:
            n, pos = _varint(buf, pos)
            value, pos = (pos, pos + n), pos + n
        elif kind == 5:
            value, pos = (pos, pos + 4), pos + 4
        else:
            raise ValueError(f"protobuf: wire type {kind} at byte {pos} is not one a GraphDef holds")
        if pos > end:
            raise ValueError(f"protobuf: field {number} runs past the end of its message at byte {end}")
        yield number, kind, value


def _tensor(buf, pos, end):
    """TensorProto -> (dtype, shape, fp32 array or None): dtype = 1, tensor_shape = 2, tensor_content = 4, float_val = 5."""
    dtype, shape, content, values = 0, [], None, []
    for number, kind, v in _fields(buf, pos, end):
        if number == 1 and kind == 0:
            dtype = v
        elif number == 2 and kind == 2:
            for n2, k2, dim in _fields(buf, *v):
                if n2 == 2 and k2 == 2:                                  # TensorShapeProto.dim, Dim.size = 1
                    shape.append(next((int(s) for n3, k3, s in _fields(buf, *dim) if n3 == 1 and k3 == 0), 0))
        elif number == 4 and kind == 2:
            content = v
        elif number == 5:                                                # packed, or one fixed32 per entry
            values.append(np.frombuffer(buf[v[0]:v[1]], dtype="<f4"))
    if dtype != 1:                                                       # DT_FLOAT
        return dtype, tuple(shape), None
    count = int(np.prod(shape)) if shape else 1
    if content is not None and content[1] - content[0] == 4 * count:
        data = np.frombuffer(buf[content[0]:content[1]], dtype="<f4").astype(np.float32)
    elif values:
        data = np.concatenate(values).astype(np.float32)
        if data.size == 1 and count > 1:                                 # one value stands for all
            data = np.full(count, data[0], dtype=np.float32)
        if data.size != count:
            return dtype, tuple(shape), None
    else:
        return dtype, tuple(shape), None
    return dtype, tuple(shape), data.reshape(shape)


def read_graph_consts(path) -> dict:
    """name -> (shape, fp32 array or None for another dtype) of every ``Const`` node of a frozen GraphDef, read with
    mmap and without TensorFlow: GraphDef.node = 1; NodeDef name = 1, op = 2, attr = 5 (key = 1, value = 2);
    AttrValue.tensor = 8."""
    consts = {}
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        if size == 0:
            raise ValueError(f"{path}: empty file")
        buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    try:
        for number, kind, node in _fields(buf, 0, size):
            if number != 1 or kind != 2:
                continue
            name, op, tensor = "", "", None
            for n2, k2, v in _fields(buf, *node):
                if k2 != 2:
                    continue
                if n2 == 1:
                    name = buf[v[0]:v[1]].decode("utf-8", "replace")
                elif n2 == 2:
                    op = buf[v[0]:v[1]].decode("utf-8", "replace")
                elif n2 == 5:
                    key, value = "", None
                    for n3, k3, e in _fields(buf, *v):
                        if n3 == 1 and k3 == 2:
                            key = buf[e[0]:e[1]].decode("utf-8", "replace")
                        elif n3 == 2 and k3 == 2:
                            value = e
                    if key == "value" and value is not None:
                        tensor = next((t for n4, k4, t in _fields(buf, *value) if n4 == 8 and k4 == 2), None)
            if op == "Const" and tensor is not None:
                _, shape, data = _tensor(buf, *tensor)
                consts[name] = (shape, data)
    finally:
        buf.close()
    return consts


class DeepSpeechWeights:
    """The fourteen constants of the graph as fp32 arrays: the dense ``h1, b1, h2, b2, h3, b3, h5, b5, h6, b6`` (every
    matrix [in, out]) and, per direction, the LSTM's ``fw_kernel`` [hidden + cell, 4 cell] (rows: input then recurrent;
    columns: gates i, j, f, o) and ``fw_bias`` [4 cell], ``bw_kernel``, ``bw_bias``."""

    def __init__(self, dims: DeepSpeechDims, arrays: dict):
        self.dims = dims
        want = dims.shapes()
        missing = [n for n in want if n not in arrays]
        if missing:
            raise ValueError(f"DeepSpeechWeights: missing {missing}")
        self.arrays = {}
        for name, shape in want.items():
            a = np.ascontiguousarray(np.asarray(arrays[name], dtype=np.float32))
            if a.shape != shape:
                raise ValueError(f"DeepSpeechWeights: {name} has shape {a.shape}, the dims say {shape}")
            self.arrays[name] = a
        self._cache = {}

    @classmethod
    def random(cls, dims: DeepSpeechDims = DeepSpeechDims(), seed: int = 0) -> "DeepSpeechWeights":
        """Seeded weights of a size that keeps every layer alive: matrices uniform within sqrt(3 / fan_in) (unit gain),
        biases within 0.1."""
        g = torch.Generator().manual_seed(int(seed))
        arrays = {}
        for name, shape in dims.shapes().items():
            bound = math.sqrt(3.0 / shape[0]) if len(shape) == 2 else 0.1
            arrays[name] = ((torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound).numpy()
        return cls(dims, arrays)

    @classmethod
    def from_arrays(cls, arrays: dict, dims: DeepSpeechDims = None) -> "DeepSpeechWeights":
        """From a dict with the fourteen names; the dims are read off the shapes unless given (clip 20, forget bias 1)."""
        if dims is None:
            missing = [n for n in ("h1", "h6", "fw_bias") if n not in arrays]
            if missing:
                raise ValueError(f"DeepSpeechWeights: missing {missing}")
            h1, h6, fb = (np.asarray(arrays[n]) for n in ("h1", "h6", "fw_bias"))
            if h1.ndim != 2 or h6.ndim != 2 or fb.ndim != 1 or fb.shape[0] % 4:
                raise ValueError("DeepSpeechWeights: h1 and h6 are matrices, fw_bias is a vector of 4 cell entries")
            dims = DeepSpeechDims(n_in=h1.shape[0], hidden=h1.shape[1], cell=fb.shape[0] // 4, n_out=h6.shape[1])
        return cls(dims, arrays)

    def save_npz(self, path):
        """The fourteen arrays under their names, with ``clip`` and ``forget_bias``."""
        np.savez(path, clip=np.float64(self.dims.clip), forget_bias=np.float64(self.dims.forget_bias), **self.arrays)

    @classmethod
    def load(cls, path, dims: DeepSpeechDims = None) -> "DeepSpeechWeights":
        """From an ``.npz`` written by ``save_npz`` (the route for constants exported with one's own TensorFlow), or
        from the frozen graph ``deepspeech-0_1_0-b90017e8.pb`` itself, read without TensorFlow.

        In a graph the dense tensors are the ``Const`` nodes named h1, b1, h2, b2, h3, b3, h5, b5, h6, b6, with or
        without a scope in front; the LSTM's are the ``Const`` nodes whose names contain ``/fw/`` or ``/bw/`` and end in
        ``kernel`` or ``weights``, respectively ``bias`` or ``biases``.  Every shape is checked against ``dims`` (default:
        DeepSpeech 0.1.0).  These names are written from knowledge of the model, not read from the file, which was not
        at hand: where a tensor is missing or misshapen the ValueError lists every Const node with its shape."""
        path = str(path)
        if path.endswith(".npz"):
            with np.load(path) as z:
                arrays = {n: z[n] for n in z.files}
            w = cls.from_arrays(arrays, dims)
            if dims is None and "clip" in arrays:
                w = cls(DeepSpeechDims(**{**asdict(w.dims), "clip": float(arrays["clip"]),
                                          "forget_bias": float(arrays["forget_bias"])}), w.arrays)
            return w
        dims = dims or DeepSpeechDims()
        consts = read_graph_consts(path)
        want, found, problems = dims.shapes(), {}, []

        def role(name):
            base = name.rsplit("/", 1)[-1]
            if base in DENSE_NAMES:
                return base
            for p in ("fw", "bw"):
                if f"/{p}/" in name:
                    if base.endswith(("kernel", "weights")):
                        return p + "_kernel"
                    if base.endswith(("bias", "biases")):
                        return p + "_bias"
            return None

        for name, (shape, data) in consts.items():
            r = role(name)
            if r is None:
                continue
            if shape == want[r] and data is not None:
                if r in found:
                    problems.append(f"{r}: both {found[r][0]!r} and {name!r} fit")
                found[r] = (name, data)
        for r in want:
            if r not in found:
                near = [f"{n} {s}" for n, (s, _) in consts.items() if role(n) == r]
                problems.append(f"{r} {want[r]}: " + ("no Const node by that name" if not near else
                                                      "not the shape of " + ", ".join(near)))
        if problems:
            listing = "\n".join(f"  {n} {list(s)}" for n, (s, _) in consts.items())
            raise ValueError(f"{path}: cannot take the DeepSpeech weights from this graph:\n  " + "\n  ".join(problems) +
                             f"\nits {len(consts)} Const nodes:\n{listing}")
        return cls(dims, {r: data for r, (_, data) in found.items()})

    def to(self, device, dtype) -> dict:
        key = (str(device), dtype)
        if key not in self._cache:
            self._cache = {key: {n: torch.from_numpy(a).to(device=device, dtype=dtype) for n, a in self.arrays.items()}}
        return self._cache[key]

    def lstm_kernels(self, device, dtype):
        """Per direction (wx [hidden, 4 cell], wh [cell, 4 cell], bias [4 cell])."""
        w, H = self.to(device, dtype), self.dims.hidden
        return [(w[p + "_kernel"][:H], w[p + "_kernel"][H:], w[p + "_bias"]) for p in ("fw", "bw")]

    def device_pack(self, device):
        """-> (struct DeepspeechWeights, the device tensors it points to), laid out as include/instag_deepspeech.h says:
        W1's rows zero-padded to a multiple of 32, W6's columns and b6 to a multiple of 4, the LSTM kernels split into
        wx [2, hidden, 4 cell] and the transposed wh [2, cell, 4, cell]."""
        from . import _lib
        d = self.dims.check()
        t = {n: torch.from_numpy(a) for n, a in self.arrays.items()}
        keep = []

        def put(x):
            x = x.to(dtype=torch.float32).contiguous().to(device)
            keep.append(x)
            return x.data_ptr()

        s = _lib.DeepspeechWeights()
        for field, value in asdict(d).items():
            setattr(s, field, value)
        k1, n6 = -(-d.n_in // 32) * 32, -(-d.n_out // 4) * 4
        s.w1 = put(torch.cat([t["h1"], t["h1"].new_zeros(k1 - d.n_in, d.hidden)]))
        s.w6 = put(torch.cat([t["h6"], t["h6"].new_zeros(d.hidden, n6 - d.n_out)], dim=1))
        s.b6 = put(torch.cat([t["b6"], t["b6"].new_zeros(n6 - d.n_out)]))
        s.b1, s.w2, s.b2, s.w3, s.b3, s.w5, s.b5 = (put(t[n]) for n in ("b1", "h2", "b2", "h3", "b3", "h5", "b5"))
        kernels = [t["fw_kernel"], t["bw_kernel"]]
        s.wx = put(torch.stack([k[:d.hidden] for k in kernels]))
        s.bx = put(torch.stack([t["fw_bias"], t["bw_bias"]]))
        # kernel[hidden + k][gate cell + unit] -> wh[unit][gate][k]
        s.wh = put(torch.stack([k[d.hidden:].reshape(d.cell, 4, d.cell).permute(2, 1, 0) for k in kernels]))
        return s, keep


# ---- plain-torch statement -------------------------------------------------------------------------------------------
def recurrence_torch(xz, wh, forget_bias: float):
    """One direction of the BasicLSTMCell on its input projections xz [S, 4 cell] (bias included) with the recurrent
    half wh [cell, 4 cell], from a zero state -> [S, cell]: z = xz_t + h wh split into i, j, f, o;
    c = c sigmoid(f + forget_bias) + sigmoid(i) tanh(j); h = tanh(c) sigmoid(o)."""
    cell = wh.shape[0]
    h, c, out = xz.new_zeros(cell), xz.new_zeros(cell), []
    for t in range(xz.shape[0]):
        i, j, f, o = (xz[t] + h @ wh).split(cell)
        c = c * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * torch.tanh(j)
        h = torch.tanh(c) * torch.sigmoid(o)
        out.append(h)
    return torch.stack(out)


def lstm_torch(weights: DeepSpeechWeights, xp):
    """The bidirectional recurrence on given input projections xp [S, 2, 4 cell] -> [S, 2 cell] (forward | backward):
    the backward direction is the same cell over the reversed sequence, its outputs put back in time order."""
    xp = torch.as_tensor(xp)
    (_, wf, _), (_, wb, _) = weights.lstm_kernels(xp.device, xp.dtype)
    fb = weights.dims.forget_bias
    return torch.cat([recurrence_torch(xp[:, 0], wf, fb), recurrence_torch(xp[:, 1].flip(0), wb, fb).flip(0)], dim=1)


def deepspeech_torch(weights: DeepSpeechWeights, x, taps=None):
    """The network, input rows [S, n_in] -> raw logits [S, n_out], in the rows' dtype on their device.  ``taps``: a list
    that receives (name, tensor) of h1, h2, h3, lstm, h5 and logits."""
    x = torch.as_tensor(x)
    d = weights.dims
    if x.dim() != 2 or x.shape[1] != d.n_in or x.shape[0] < 1:
        raise ValueError(f"deepspeech: input rows [S >= 1, {d.n_in}], got {tuple(x.shape)}")
    w = weights.to(x.device, x.dtype)

    def tap(name, v):
        if taps is not None:
            taps.append((name, v))
        return v

    def layer(v, n):
        return torch.clamp(torch.relu(v @ w["h" + n] + w["b" + n]), max=d.clip)

    h = tap("h1", layer(x, "1"))
    h = tap("h2", layer(h, "2"))
    h = tap("h3", layer(h, "3"))
    xp = torch.stack([h @ wx + b for wx, _, b in weights.lstm_kernels(x.device, x.dtype)], dim=1)
    h = tap("lstm", lstm_torch(weights, xp))
    h = tap("h5", layer(h, "5"))
    return tap("logits", h @ w["h6"] + w["b6"])


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class DeepSpeechEncoder(DeviceOperator):
    """``logits(x [S, n_in]) -> [S, n_out]``, fp32 on ``device``, on torch's current stream; inference only.  On the GPU
    the rows go through csrc/deepspeech.hip in one launch with the kept workspace of device_op.DeviceOperator.  The
    dense layers in front of the recurrence run in time blocks of at most ``max_rows`` steps; the default is the largest
    that keeps the workspace within 1 GiB (the input projections alone are 64 KB a step at the real size), and the
    result does not depend on it by a bit.  On a CPU device it is the torch statement.  ``tile``: 0, or 1..3 to pin the
    GEMM tile (tests)."""

    def __init__(self, weights: DeepSpeechWeights, device="cuda", max_rows=None, tile: int = 0):
        self.max_rows, self.tile = self._at_least_one(max_rows, "max_rows"), int(tile)
        super().__init__(weights, device)

    def rows_per_block(self, S: int) -> int:
        """``max_rows`` where given, else the largest block whose workspace for S steps stays within WORKSPACE_LIMIT."""
        if self.max_rows is not None:
            return self.max_rows
        return default_max_rows(self.weights.dims, S)

    @torch.no_grad()
    def logits(self, x, taps=None):
        """``taps``: a list that receives (name, tensor) of every stage as ``deepspeech_torch``'s does, but for the
        logits."""
        x = torch.as_tensor(x)
        d = self.weights.dims
        if x.dim() != 2 or x.shape[1] != d.n_in or x.shape[0] < 1:
            raise ValueError(f"DeepSpeechEncoder: input rows [S >= 1, {d.n_in}], got {tuple(x.shape)}")
        x = x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if self.device.type != "cuda":
            return self._statement(deepspeech_torch, x, taps, ("logits",))
        from . import _lib
        S = x.shape[0]
        R = self.rows_per_block(S)
        ws = self._workspace(_lib.workspace_bytes(self._L.instag_deepspeech_workspace_bytes(C.byref(self._struct), S, R)))
        out = torch.empty(S, d.n_out, dtype=torch.float32, device=self.device)
        flat = None if taps is None else self._taps_buffer(self._L.instag_deepspeech_taps_floats(C.byref(self._struct), S))
        with torch.cuda.device(self.device):
            _lib.check_arg(self._L.instag_deepspeech_forward(
                C.byref(self._struct), _lib.ptr(x), S, R, _lib.ptr(out), _lib.ptr(ws), ws.numel(), self.tile,
                _lib.ptr(flat), _lib.current_stream()), "deepspeech_forward")
        if taps is not None:
            taps += self._cut(flat, [(name, (S, cols)) for name, cols in (
                ("h1", d.hidden), ("h2", d.hidden), ("h3", d.hidden), ("lstm", 2 * d.cell), ("h5", d.hidden))])
        return out

    @torch.no_grad()
    def recurrence(self, xp):
        """The recurrence alone (instag_deepspeech_lstm): input projections xp [S, 2, 4 cell] -> [S, 2 cell]; on a CPU
        device ``lstm_torch``."""
        xp = torch.as_tensor(xp)
        d = self.weights.dims
        if xp.dim() != 3 or tuple(xp.shape[1:]) != (2, 4 * d.cell) or xp.shape[0] < 1:
            raise ValueError(f"DeepSpeechEncoder: input projections [S >= 1, 2, {4 * d.cell}], got {tuple(xp.shape)}")
        xp = xp.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if self.device.type != "cuda":
            return lstm_torch(self.weights, xp)
        from . import _lib
        S = xp.shape[0]
        out = torch.empty(S, 2 * d.cell, dtype=torch.float32, device=self.device)
        c = torch.empty(2, d.cell, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check_arg(self._L.instag_deepspeech_lstm(C.byref(self._struct), _lib.ptr(xp), _lib.ptr(out), _lib.ptr(c), S,
                                                          _lib.current_stream()), "deepspeech_lstm")
        return out


def default_max_rows(dims: DeepSpeechDims, S: int) -> int:
    """The largest time block for S steps whose workspace stays within WORKSPACE_LIMIT, at least 1: the whole sequence
    where that fits; otherwise a block costs two rows of the dense buffers and one of the input projections a step,
    beside the [S, 2 cell] output of the recurrence that is always held whole."""
    S = int(S)
    k1, n6 = -(-dims.n_in // 32) * 32, -(-dims.n_out // 4) * 4
    dense = k1 + dims.hidden + max(dims.hidden, n6)
    held = 4 * (2 * dims.cell * (S + 1) + 6 * 64)                    # the output, the cell states, the pieces' alignment
    if held + 4 * S * (dense + 8 * dims.cell) <= WORKSPACE_LIMIT:
        return S
    return max(1, min(S - 1, (WORKSPACE_LIMIT - held) // (4 * (2 * dense + 8 * dims.cell))))


# ---- the features -----------------------------------------------------------------------------------------------------
def deepspeech_features(wav16k, weights: DeepSpeechWeights, device="cuda", encoder=None,
                        sample_rate: int = SAMPLE_RATE) -> np.ndarray:
    """The array the reference saves as aud_ds.npy for 16 kHz samples [L] in [-1, 1] (``load_wav16k``), fp64
    [W, 16, n_out].  The samples become int16 as in the reference (``to_int16``).  Any other ``sample_rate`` raises:
    resampling is not provided.  ``encoder`` is called as ``encoder(weights, input_rows)`` in place of the HIP operator
    -- the tests' comparand."""
    if int(sample_rate) != SAMPLE_RATE:
        raise ValueError(f"deepspeech_features: sample rate {sample_rate} Hz, expected {SAMPLE_RATE} Hz (resample the "
                         "audio first)")
    x = torch.as_tensor(wav16k)
    if x.dim() != 1 or x.numel() < 1:
        raise ValueError(f"deepspeech_features: samples [L >= 1], got {tuple(x.shape)}")
    device = torch.device(device)
    rows = torch.from_numpy(input_vectors(to_int16(x))).to(device)
    if encoder is None:
        op = DeepSpeechEncoder(weights, device)
        encoder = lambda _, values: op.logits(values)              # noqa: E731
    with torch.no_grad():
        logits = encoder(weights, rows).detach().double().cpu().numpy()
    return windows(interpolate(logits, x.numel()))
