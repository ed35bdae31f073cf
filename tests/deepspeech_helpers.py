"""Shared by the DeepSpeech tests: the small configs and their seeded weights, a writer of synthetic frozen graphs (a few
lines of protobuf wire format), the remapping of the LSTM's weights to ``torch.nn.LSTM``, a literal transcription of the
reference's two windowing loops, and the fp64 references of the network and of the recurrence alone (computed once per
case and left unchanged) with the bar the GPU tests derive from them."""
import functools
import struct

import numpy as np
import torch

from instag_amd.deepspeech import DeepSpeechDims, DeepSpeechWeights, deepspeech_torch, lstm_torch

# the smallest shapes at which the kernels can go wrong: one and two 16-byte loads per lane of the step kernel (cell),
# a GEMM tile edge (hidden 64 fills a 64-column tile, 96 ends inside the second), the padded n_in and n_out
CONFIGS = {"A": DeepSpeechDims(n_in=494, hidden=64, cell=256, n_out=29),
           "B": DeepSpeechDims(n_in=494, hidden=96, cell=512, n_out=29)}
TINY = DeepSpeechDims(n_in=494, hidden=16, cell=8, n_out=29)        # CPU only: no kernel takes cell = 8
STEPS = (1, 2, 5, 67)           # no previous state, one hand-over, an odd length, more rows than one 64-row GEMM tile
EPS32 = 2.0 ** -23
FACTOR = 4.0


REAL = DeepSpeechDims()


@functools.lru_cache(maxsize=None)
def weights(name: str, seed: int = 3) -> DeepSpeechWeights:
    """Seeded weights of config "A" or "B", of TINY ("T") or of the real size ("R")."""
    return DeepSpeechWeights.random({**CONFIGS, "T": TINY, "R": REAL}[name], seed)


def seeded_rows(S: int, n_in: int, seed: int = 5) -> torch.Tensor:
    """Input rows as ``input_vectors`` gives them in size: zero mean, unit deviation; fp32 [S, n_in]."""
    return torch.randn(S, n_in, generator=torch.Generator().manual_seed(seed + 1000 * S), dtype=torch.float32)


def bar(got32: torch.Tensor, want: torch.Tensor):
    """-> (e32, bar): e32 the largest absolute error of the fp32 CPU statement against the fp64 one, the bar
    4 max(e32, eps32 max|fp64|): the factor covers the other summation order of the MFMA tiles and of the wave's
    reduction over K = cell; the clip and the bounded gates keep the recurrence from amplifying it."""
    e32 = float((got32.double() - want).abs().max())
    return e32, FACTOR * max(e32, EPS32 * float(want.abs().max()))


class Case:
    """Input rows with the fp64 statement's stages and the fp32 CPU statement's."""

    def __init__(self, w: DeepSpeechWeights, x: torch.Tensor):
        self.w, self.x = w, x
        taps, taps32 = [], []
        self.want = deepspeech_torch(w, x.double(), taps)
        self.got32 = deepspeech_torch(w, x.float(), taps32)
        self.taps, self.taps32 = dict(taps), dict(taps32)
        w._cache = {}                                                # (the fp64 copy of the real size is 0.5 GB)

    def bar(self, stage="logits"):
        return bar(self.taps32[stage], self.taps[stage])


@functools.lru_cache(maxsize=None)
def case(name: str, S: int) -> Case:
    w = weights(name)
    return Case(w, seeded_rows(S, w.dims.n_in))


class LstmCase:
    """Input projections [S, 2, 4 cell] with the fp64 recurrence and the fp32 CPU one."""

    def __init__(self, w: DeepSpeechWeights, xp: torch.Tensor):
        self.w, self.xp = w, xp
        self.want = lstm_torch(w, xp.double())
        self.got32 = lstm_torch(w, xp.float())


def seeded_xp(S: int, cell: int, seed: int = 9) -> torch.Tensor:
    """[67, 2, 4 cell] of unit deviation, cut to S steps: every length shares its prefix."""
    full = torch.randn(67, 2, 4 * cell, generator=torch.Generator().manual_seed(seed + cell), dtype=torch.float32)
    return full[:S].contiguous()


@functools.lru_cache(maxsize=None)
def lstm_case(name: str, S: int) -> LstmCase:
    w = weights(name)
    return LstmCase(w, seeded_xp(S, w.dims.cell))


def mirrored(w: DeepSpeechWeights) -> DeepSpeechWeights:
    """The weights with the forward direction's LSTM copied into the backward one."""
    arrays = dict(w.arrays)
    arrays["bw_kernel"], arrays["bw_bias"] = arrays["fw_kernel"], arrays["fw_bias"]
    return DeepSpeechWeights(w.dims, arrays)


def scaled(w: DeepSpeechWeights, name: str, factor: float) -> DeepSpeechWeights:
    arrays = dict(w.arrays)
    arrays[name] = arrays[name] * np.float32(factor)
    return DeepSpeechWeights(w.dims, arrays)


# ---- torch.nn.LSTM with the weights remapped --------------------------------------------------------------------------
def torch_lstm(w: DeepSpeechWeights) -> torch.nn.LSTM:
    """``torch.nn.LSTM(hidden, cell, bidirectional=True)`` in fp64 computing the BasicLSTMCell pair: the gate order
    i, j, f, o becomes torch's i, f, g, o; the forget bias is folded into the bias; the kernel's rows are split into
    weight_ih and weight_hh (torch keeps [4 cell, in])."""
    d = w.dims
    net = torch.nn.LSTM(d.hidden, d.cell, bidirectional=True).double()
    order = [0, 2, 1, 3]                                             # torch's gate g (i, f, g, o) <- ours (i, j, f, o)
    with torch.no_grad():
        for p, suffix in (("fw", ""), ("bw", "_reverse")):
            kernel = torch.from_numpy(w.arrays[p + "_kernel"]).double().reshape(d.hidden + d.cell, 4, d.cell)[:, order]
            bias = torch.from_numpy(w.arrays[p + "_bias"]).double().reshape(4, d.cell)[order].clone()
            bias[1] += d.forget_bias
            getattr(net, "weight_ih_l0" + suffix).copy_(kernel[:d.hidden].reshape(d.hidden, -1).t())
            getattr(net, "weight_hh_l0" + suffix).copy_(kernel[d.hidden:].reshape(d.cell, -1).t())
            getattr(net, "bias_ih_l0" + suffix).copy_(bias.reshape(-1))
            getattr(net, "bias_hh_l0" + suffix).zero_()
    return net


def torch_chain(w: DeepSpeechWeights, device, dtype=torch.float32):
    """x [S, n_in] -> logits through ``torch.nn.LSTM`` and linear layers on ``device``: the comparand of
    scripts/bench_deepspeech.py."""
    d = w.dims
    net = torch_lstm(w).to(device=device, dtype=dtype)
    t = {n: torch.from_numpy(a).to(device=device, dtype=dtype) for n, a in w.arrays.items()}

    @torch.no_grad()
    def run(x):
        h = x
        for n in "123":
            h = torch.clamp(torch.relu(h @ t["h" + n] + t["b" + n]), max=d.clip)
        h = net(h[:, None])[0][:, 0]
        h = torch.clamp(torch.relu(h @ t["h5"] + t["b5"]), max=d.clip)
        return h @ t["h6"] + t["b6"]

    return run


# ---- the reference's two windowing loops, transcribed -----------------------------------------------------------------
def reference_windows(network_output: np.ndarray) -> np.ndarray:
    """pure_conv_audio_to_deepspeech's loop with audio_window_size = audio_window_stride = 1, then
    conv_audios_to_deepspeech's with win_size = 16, written out as they stand."""
    audio_window_size, audio_window_stride = 1, 1
    zero_pad = np.zeros((int(audio_window_size / 2), network_output.shape[1]))
    network_output = np.concatenate((zero_pad, network_output, zero_pad), axis=0)
    first = []
    for window_index in range(0, network_output.shape[0] - audio_window_size, audio_window_stride):
        first.append(network_output[window_index:window_index + audio_window_size])
    ds_features = np.array(first)
    net_output = ds_features.reshape(-1, network_output.shape[1])
    win_size = 16
    zero_pad = np.zeros((int(win_size / 2), net_output.shape[1]))
    net_output = np.concatenate((zero_pad, net_output, zero_pad), axis=0)
    second = []
    for window_index in range(0, net_output.shape[0] - win_size, 2):
        second.append(net_output[window_index:window_index + win_size])
    return np.array(second)


# ---- a synthetic frozen graph ------------------------------------------------------------------------------------------
def _varint(n: int) -> bytes:
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def _field(number: int, payload: bytes) -> bytes:
    """A length-delimited field."""
    return _varint(number << 3 | 2) + _varint(len(payload)) + payload


def _const(name: str, array: np.ndarray, mode: str, dtype: int = 1) -> bytes:
    """A NodeDef of op Const with attrs dtype and value (a TensorProto: dtype = 1, tensor_shape = 2, and the values
    as tensor_content = 4, as packed float_val = 5, or as one fixed32 float_val per entry)."""
    a = np.ascontiguousarray(array, dtype="<f4")
    shape = b"".join(_field(2, _varint(1 << 3) + _varint(n)) for n in a.shape)
    tensor = _varint(1 << 3) + _varint(dtype) + _field(2, shape)
    if mode == "content":
        tensor += _field(4, a.tobytes())
    elif mode == "float_val":
        tensor += _field(5, a.tobytes())
    else:                                                            # "unpacked"
        tensor += b"".join(_varint(5 << 3 | 5) + struct.pack("<f", v) for v in a.reshape(-1))
    attrs = _field(5, _field(1, b"dtype") + _field(2, _varint(6 << 3) + _varint(dtype)))
    attrs += _field(5, _field(1, b"value") + _field(2, _field(8, tensor)))
    return _field(1, name.encode()) + _field(2, b"Const") + attrs


def _node(name: str, op: str, inputs=()) -> bytes:
    return _field(1, name.encode()) + _field(2, op.encode()) + b"".join(_field(3, i.encode()) for i in inputs)


GRAPH_NAMES = {"fw_kernel": "bidirectional_rnn/fw/basic_lstm_cell/kernel", "fw_bias": "bidirectional_rnn/fw/basic_lstm_cell/bias",
               "bw_kernel": "bidirectional_rnn/bw/basic_lstm_cell/kernel", "bw_bias": "bidirectional_rnn/bw/basic_lstm_cell/bias"}


def write_graph(path, w: DeepSpeechWeights, mode="content", scope="", names=GRAPH_NAMES, leave_out=(), reshape=None):
    """A GraphDef with the weights as Const nodes, non-Const nodes between them and two unrelated Consts (one of them an
    int32).  ``leave_out``: roles not written; ``reshape``: {role: shape} written with another shape."""
    nodes = [_node("input_node", "Placeholder"), _const(scope + "unrelated/ones", np.ones((3, 2)), mode)]
    for role, a in w.arrays.items():
        if role in leave_out:
            continue
        if reshape and role in reshape:
            a = a.reshape(reshape[role])
        nodes.append(_const(scope + names.get(role, role), a, mode))
        nodes.append(_node(scope + role + "/read", "Identity", [scope + names.get(role, role)]))
    nodes.append(_const(scope + "Reshape/shape", np.zeros(2), "content", dtype=3))
    nodes.append(_node("logits", "Add", ["MatMul_5", scope + "b6/read"]))
    with open(path, "wb") as f:
        f.write(b"".join(_field(1, n) for n in nodes) + _varint(3 << 3) + _varint(27))       # (GraphDef.version)
