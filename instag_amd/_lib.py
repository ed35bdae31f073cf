"""ctypes binding of libinstag_hip.so (the C ABI declared in include/instag_hip.h).

There is no CPU fallback: if the shared library cannot be loaded (and cannot be built with
hipcc), importing any operator raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from . import _cabi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libinstag_hip.so")

_lib = None
_lock = threading.Lock()

vp = C.c_void_p
i32 = C.c_int32
f32 = C.c_float

# The C ABI is stated once, in include/instag_hip.h: the struct classes, the prototypes and the constants are read from
# its text here, and a declaration _cabi cannot read raises.  struct instag_raster_args is the class RasterArgs, and so
# on: FaceLossCfg, LpipsWeights, AveEncoderWeights, ParsingWeights, TeethWeights, FrameUnpackArgs, TrackArgs,
# MeshSettings, WgradJob.
_STRUCTS, _PROTOTYPES, _CONSTANTS = _cabi.read()
globals().update((cls.__name__, cls) for cls in _STRUCTS.values())
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)
ABI_VERSION = _CONSTANTS["INSTAG_ABI_VERSION"]     # a stale libinstag_hip.so must not be driven with these prototypes
E_ARG = _CONSTANTS["INSTAG_E_ARG"]
FACE_LOSS = {k[len("INSTAG_FACE_LOSS_"):]: v for k, v in _CONSTANTS.items() if k.startswith("INSTAG_FACE_LOSS_")}

# The wav2vec network's part of the ABI has a header of its own, include/instag_wav2vec.h, read by the same reader:
# struct Wav2vecWeights, instag_wav2vec_workspace_bytes / instag_wav2vec_forward and the INSTAG_WAV2VEC_* bounds.
_WAV2VEC_STRUCTS, _WAV2VEC_PROTOTYPES, WAV2VEC = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_wav2vec.h"))
globals().update((cls.__name__, cls) for cls in _WAV2VEC_STRUCTS.values())

# The HuBERT encoder's part, include/instag_hubert.h, likewise: it declares no struct of its own and takes the wav2vec
# header's weights, which the reader is told of; instag_hubert_* and the INSTAG_HUBERT_MAX_FRAMES bound.
_HUBERT_STRUCTS, _HUBERT_PROTOTYPES, HUBERT = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_hubert.h"),
                                                         _WAV2VEC_STRUCTS)

# The per-frame codes of a 'hubert' head, include/instag_frame_code_wide.h: the three instag_frame_code_wide_* entry
# points (instag_amd/audio.py), no struct and no constant.
_, _FRAME_CODE_WIDE_PROTOTYPES, _ = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_frame_code_wide.h"))

# The DeepSpeech network's part, include/instag_deepspeech.h (instag_amd/deepspeech.py): struct DeepspeechWeights, the
# four instag_deepspeech_* entry points and the INSTAG_DEEPSPEECH_* bounds.
_DEEPSPEECH_STRUCTS, _DEEPSPEECH_PROTOTYPES, DEEPSPEECH = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER),
                                                                              "instag_deepspeech.h"))
globals().update((cls.__name__, cls) for cls in _DEEPSPEECH_STRUCTS.values())

# The face landmark network's part, include/instag_landmarks.h (instag_amd/landmarks.py): struct LandmarksWeights, the
# four instag_landmarks_* entry points and the INSTAG_LANDMARKS_* bounds.
_LANDMARKS_STRUCTS, _LANDMARKS_PROTOTYPES, LANDMARKS = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER),
                                                                             "instag_landmarks.h"))
globals().update((cls.__name__, cls) for cls in _LANDMARKS_STRUCTS.values())

# The face detector's part, include/instag_face_detect.h (instag_amd/face_detect.py): struct FaceDetectWeights, the
# instag_face_detect* entry points and the INSTAG_FACE_DETECT_* bounds.
_FACE_DETECT_STRUCTS, _FACE_DETECT_PROTOTYPES, FACE_DETECT = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER),
                                                                                   "instag_face_detect.h"))
globals().update((cls.__name__, cls) for cls in _FACE_DETECT_STRUCTS.values())

# The tri-plane encode fused into the motion fields' forward MLP kernels, include/instag_encode_mlp.h
# (instag_amd/encode_mlp.py): the three instag_triplane_mlp* entry points, no struct and no constant.
_, _ENCODE_MLP_PROTOTYPES, _ = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_encode_mlp.h"))

# The Sapiens normal / depth network's part, include/instag_sapiens.h (instag_amd/sapiens.py): struct SapiensWeights as
# the C side sees it (_lib.SapiensStruct; the name SapiensWeights is the Python class of sapiens.py), the
# instag_sapiens_* entry points and the INSTAG_SAPIENS_* bounds.
_SAPIENS_STRUCTS, _SAPIENS_PROTOTYPES, SAPIENS = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_sapiens.h"))
SapiensStruct = _SAPIENS_STRUCTS["instag_sapiens_weights"]

# The JPEG encoder's part, include/instag_mjpeg.h (instag_amd/mjpeg.py): the three instag_mjpeg_* entry points and the
# INSTAG_MJPEG_* bounds, no struct.
_, _MJPEG_PROTOTYPES, MJPEG = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_mjpeg.h"))

# The JPEG decoder's part, include/instag_jpeg_decode.h (instag_amd/jpeg_decode.py): the four instag_jpeg_decode* entry
# points, the INSTAG_JPEG_DECODE_* bounds and status codes, no struct.
_, _JPEG_DECODE_PROTOTYPES, JPEG_DECODE = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_jpeg_decode.h"))


# ---- streams -------------------------------------------------------------------------------------------------------
# torch.cuda.Stream() does not create a HIP stream: it hands out the next of 32 pooled streams per (device, priority),
# round robin.  A process that asks for more than 32 -- every capture used to take a fresh "capture stream" and a fresh
# warm-up stream, every module kept its own cache of side streams -- therefore gets the SAME HIP stream under two
# Python objects: a forked pass and the lane it forks to, a "leaf" stream and an operator's side lane, two branches of
# one captured step.  Every stream of the package now comes from this registry: one per (device, purpose), created once
# (outside any capture) and guaranteed distinct from every other stream the registry handed out.
_STREAMS = {}


def side_stream(device, tag, priority=0):
    """The persistent HIP stream of purpose ``tag`` on ``device`` (distinct handles for distinct tags)."""
    import torch
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, tag)
    s = _STREAMS.get(key)
    if s is None:
        taken = {v.cuda_stream for (d, _), v in _STREAMS.items() if d == index}
        for _ in range(64):
            s = torch.cuda.Stream(device=torch.device("cuda", index), priority=priority)
            if s.cuda_stream not in taken:
                break
        else:
            raise RuntimeError(f"no distinct HIP stream left for {tag!r} ({len(taken)} in use on device {index})")
        _STREAMS[key] = s
    return s


def capture_stream(device=None):
    """THE stream every step of the package is captured on (one per device, high priority: the side streams operators
    fork from it keep the default priority, so the nodes of the step's critical chain win the arbitration where they
    share the chip -- C3 step 0.5-2.5 % faster).  One stream for all captures, because the autograd engine runs a
    parameter's AccumulateGrad on the stream that was current when the node was created: with a stream per capture a
    node kept alive across captures made the engine hop to the EARLIER capture's stream inside the open capture (an
    un-announced fork; PyTorch's "AccumulateGrad node's stream does not match" warning)."""
    import torch
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return side_stream(device, "capture", priority=-1)


def warmup_stream(device):
    """Side stream for the eager capacity-mode warm-up steps in front of a capture."""
    return side_stream(device, "warmup")


# ---- stream capture bookkeeping -------------------------------------------------------------------------------------
# A fork of a fork inside ONE stream capture (origin stream -> stream A -> stream B, B joined back into A, A into the
# origin) crashes hipStreamEndCapture on ROCm 7.2 (segmentation fault inside capture_end; bisected with
# scripts/probes/infer_capture_probe2.py: any operator that forks internally -- the rasterizer's depth-sort stream, a
# motion network's per-frame branch -- breaks a capture when it is itself called on a forked stream, the same
# operators on the origin stream, or without their internal fork, capture fine).  So while a capture is open,
# operators fork only from the capture's ORIGIN stream, which the owners of our captures announce here.
_CAPTURE_ORIGIN = None


class graph_capture:
    """Stream capture of one graph on the package's capture stream; records the capture's origin stream for may_fork()
    and releases the cross-stream tensors held for the capture (_keepalive) when it has ended -- whether it succeeded
    or raised.  The default form is ``torch.cuda.graph`` (device synchronisation + allocator cache flush in front: right
    for a first capture).  ``light=True`` is for re-captures inside a train loop: ``torch.cuda.graph.__enter__`` costs a
    device synchronisation and an ``empty_cache()`` (3 ms of hipFree, and every eager allocation after it pays hipMalloc
    again); here the capture simply begins -- the private pool is kept open by a GraphPool, nothing of the current
    stream's pending work is touched by recording launches."""

    def __init__(self, graph, light: bool = False, **kw):
        import torch
        if "stream" not in kw:
            kw = dict(kw, stream=capture_stream())
        self._light = bool(light)
        self._graph = graph
        if self._light:
            self._stream_ctx = torch.cuda.stream(kw["stream"])
            self._begin = {k: v for k, v in kw.items() if k in ("pool", "capture_error_mode")}
        else:
            self._ctx = torch.cuda.graph(graph, **kw)

    def __enter__(self):
        global _CAPTURE_ORIGIN
        import torch
        if self._light:
            self._stream_ctx.__enter__()
            try:
                self._graph.capture_begin(**self._begin)
            except BaseException:
                self._stream_ctx.__exit__(None, None, None)
                raise
            r = None
        else:
            r = self._ctx.__enter__()
        self._prev = _CAPTURE_ORIGIN
        _CAPTURE_ORIGIN = torch.cuda.current_stream()
        return r

    def __exit__(self, *exc):
        global _CAPTURE_ORIGIN
        _CAPTURE_ORIGIN = self._prev
        try:
            if self._light:
                try:
                    self._graph.capture_end()
                finally:
                    self._stream_ctx.__exit__(*exc)
                return None
            return self._ctx.__exit__(*exc)
        finally:
            from . import _keepalive
            _keepalive.release()


class GraphPool:
    """A private memory pool that outlives the graphs captured into it.  torch frees a graph pool when the last graph
    using it is destroyed (and asserts if its handle is used again); a trainer that drops every captured step at a
    density-control event and captures again right after would allocate a fresh pool -- hundreds of MB of hipMalloc --
    every time.  A one-node graph captured into the pool and kept here holds it open, so every later capture reuses
    the same blocks."""

    def __init__(self, device):
        import torch
        self.handle = torch.cuda.graph_pool_handle()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph, pool=self.handle, stream=capture_stream(device)):
            self._anchor = torch.zeros(64, device=device)


def may_fork(device=None) -> bool:
    """May an operator fork work onto a second stream from the current stream?  Outside a capture: unless the current
    stream carries a whole forked pass (leaf_stream); inside one only from the capture's origin stream (a capture
    somebody else opened: origin unknown -> no)."""
    import torch
    if _LEAF_STREAMS and any(torch.cuda.current_stream(device) == s for s in _LEAF_STREAMS):
        return False
    if not torch.cuda.is_current_stream_capturing():
        return True
    return _CAPTURE_ORIGIN is not None and torch.cuda.current_stream(device) == _CAPTURE_ORIGIN


# streams that carry a whole forked pass (renderer.render_fuse): operators running on them never fork further, eagerly
# or captured, so that the pass is the same chain of launches in both modes
_LEAF_STREAMS = []


def leaf_stream(stream):
    if all(stream != s for s in _LEAF_STREAMS):
        _LEAF_STREAMS.append(stream)


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            from . import build as _build
            _build.build(verbose=False)          # raises if hipcc is missing: no silent fallback
        # torch first: its wheel bundles its own libamdhip64; loaded before ours, the dynamic linker resolves our
        # DT_NEEDED entry to that same runtime (one HIP runtime per process).  The other order gives two runtimes and
        # "no ROCm-capable device is detected" from the second one.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in {**_PROTOTYPES, **_WAV2VEC_PROTOTYPES, **_HUBERT_PROTOTYPES,
                                  **_FRAME_CODE_WIDE_PROTOTYPES, **_DEEPSPEECH_PROTOTYPES,
                                  **_LANDMARKS_PROTOTYPES, **_FACE_DETECT_PROTOTYPES,
                                  **_ENCODE_MLP_PROTOTYPES, **_SAPIENS_PROTOTYPES, **_MJPEG_PROTOTYPES,
                                  **_JPEG_DECODE_PROTOTYPES}.items():
            if not hasattr(handle, name):
                raise RuntimeError(f"{LIB_PATH} does not export {name}: rebuild it (python -m instag_amd.build)")
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.instag_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {handle.instag_abi_version()}, the bindings expect "
                               f"{ABI_VERSION}: rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
        _lib = handle
    return _lib


def check(code: int, what: str = ""):
    """Turn a non-zero C-ABI return code into RuntimeError (the reference raises from C++)."""
    if code != 0:
        msg = lib().instag_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what}: {msg}" if what else msg)


def check_arg(code: int, what: str):
    """``check`` for the entry points whose callers tell a refused argument from a failure: ValueError for
    INSTAG_E_ARG, RuntimeError for every other non-zero code."""
    if code != 0:
        msg = lib().instag_last_error().decode("utf-8", "replace")
        raise (ValueError if code == E_ARG else RuntimeError)(f"{what}: {msg}")


def workspace_bytes(nbytes: int) -> int:
    """The result of a ``*_workspace_bytes`` entry point: 0 says the shape was refused -> ValueError with its text."""
    if nbytes == 0:
        raise ValueError(lib().instag_last_error().decode("utf-8", "replace"))
    return int(nbytes)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
