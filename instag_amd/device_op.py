"""What every pretrained network's operator shares on the host, whatever it takes in: frames (convnet.FrameOperator),
audio segments (wav2vec.SegmentEncoder), input rows (deepspeech.DeepSpeechEncoder) or mel windows
(ave_encoder.AudioEncoder).

``DeviceOperator`` owns the frozen weights' device copy, the one kept workspace, the chunk loop on torch's current
stream and the debug taps.  The workspace rule, the only one: a uint8 tensor that is replaced when a call needs more
bytes than it holds and is kept otherwise, whatever the shape of the call; the old one is released before the new one
is allocated.  It is the operator's: use one operator per stream.
"""
from __future__ import annotations

import contextlib
import math

import torch


class DeviceOperator:
    """``weights`` on ``device``; on a GPU also the library (``_L``) and the weights' C struct with the tensors it points
    into (``_struct``, ``_keep``: ``weights.device_pack``).  A subclass sets ``max_batch`` before it calls ``_chunks``
    and names in ``CHECK`` the function of _lib that turns a launch's return code into an exception."""

    CHECK = "check_arg"

    def __init__(self, weights, device):
        self.weights = weights
        self.device = torch.device(device)
        self._ws = None
        if self.device.type == "cuda":
            from . import _lib
            self._L = _lib.lib()
            self._struct, self._keep = weights.device_pack(self.device)

    @classmethod
    def _at_least_one(cls, value, name="max_batch", got=True):
        """``value`` as an int (None stays None); ValueError below 1, ``got``: with the value in the message."""
        if value is not None and int(value) < 1:
            raise ValueError(f"{cls.__name__}: {name} >= 1" + (f", got {value}" if got else ""))
        return None if value is None else int(value)

    def _workspace(self, nbytes):
        """The kept workspace, of at least ``nbytes`` bytes (module docstring)."""
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._ws

    def _each_chunk(self, B, nbytes, launch, what):
        """``launch(chunk slice, its length, workspace pointer, workspace bytes) -> return code`` for every chunk of at
        most ``max_batch`` of ``B`` items, with a workspace of at least ``nbytes``; ``what`` opens the message."""
        from . import _lib
        if B == 0:
            return
        ws, check = self._workspace(nbytes), getattr(_lib, self.CHECK)
        p, size = _lib.ptr(ws), int(ws.numel())
        with torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext():
            for i in range(0, B, self.max_batch):
                m = min(self.max_batch, B - i)
                check(launch(slice(i, i + m), m, p, size), what)

    # ---- taps: a flat fp32 buffer the entry point fills with every stage's output, for the tests -------------------------
    def _taps_buffer(self, floats, B=None):
        """The buffer of ``floats`` values (a ``*_taps_floats`` result: 0 says the shape was refused); ``B``: the batch
        of a chunked operator, whose taps are for one chunk."""
        from . import _lib
        if B is not None and B > self.max_batch:
            raise ValueError(f"{type(self).__name__}: taps are for one chunk, B = {B} > max_batch = {self.max_batch}")
        return torch.empty(_lib.workspace_bytes(floats), dtype=torch.float32, device=self.device)

    @staticmethod
    def _cut(flat, stages):
        """``flat`` cut into [(name, view of ``shape``)] for ``stages`` = [(name, shape)], which consume it exactly."""
        sizes = [math.prod(shape) for _, shape in stages]
        assert sum(sizes) == flat.numel()
        return [(name, piece.view(*shape)) for (name, shape), piece in zip(stages, flat.split(sizes))]

    @staticmethod
    def _kept(stages, dropped):
        """The (name, tensor) stages of a torch statement, in order, without those an operator does not tap: a name, or
        the part behind its last dot, in ``dropped``."""
        return [(name, v) for name, v in stages if name.rsplit(".", 1)[-1] not in dropped]

    def _statement(self, statement, x, taps, dropped):
        """The CPU path: ``statement(weights, x, stages)``, whose stages go on to ``taps`` through ``_kept``."""
        stages = None if taps is None else []
        out = statement(self.weights, x, stages)
        if taps is not None:
            taps += self._kept(stages, dropped)
        return out
