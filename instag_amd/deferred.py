"""Weight gradients of the fused MLPs, collected during ``loss.backward()`` and computed afterwards in ONE launch.

Only the optimizer reads a weight gradient; the rest of the backward pass needs the input gradient.  A train step has
nine such GEMMs (three MLPs of the universal field, one of the personalised field), each too small to fill the chip.

    with deferred_grads(device):
        loss.backward()            # instag_amd.mlp queues (dZ, input, weight) instead of launching
    # on exit: one instag_linear_weight_grad_batched call on the current stream, results accumulated into weight.grad

The block also lets the rasterizer's auxiliary-image backward run past the end of the rasterizer's own backward
(``diff_gauss.DEFER_AUX_JOIN``): the glue operator that consumes those gradients joins it, the block's exit at the latest.

Autograd receives ``None`` for those weights (it would otherwise copy or add a still-unwritten buffer), so the block
itself performs ``w.grad = dw`` / ``w.grad += dw``.  Outside a block nothing is queued and gradients flow through
autograd as usual.
"""
from __future__ import annotations

import torch

from . import _keepalive, _lib

_STATE = {"active": False, "jobs": [], "streams": {}, "forked": set(), "extra": []}


def flush_async(device):
    """Launch the weight gradients queued so far NOW, on a side stream behind the current stream's tail, and keep
    going: called by the trainer at a point of the backward pass where most jobs are queued and a long chain that
    does not depend on them is about to start (the personalised field's backward).  The block's exit joins.
    (Flushing earlier, right behind the backward of every per-Gaussian MLP, lost on the C3 step: starting sigma_net's
    three GEMMs beside the glue backward doubles that kernel, 33 -> 75 us on the critical path, and the graph executor
    then queues the personalised field's backward behind the next flush: 1.088 ms/step against 1.072.)"""
    if not _STATE["active"] or not _STATE["jobs"]:
        return
    device = torch.device(device)
    jobs, _STATE["jobs"] = _STATE["jobs"], []
    key = (device.type, device.index)
    side = _STATE["streams"].get(key)
    if side is None:
        side = _STATE["streams"][key] = _lib.side_stream(device, "weight_grads")
    main = torch.cuda.current_stream(device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        _flush(jobs)
    for dz, inp, _, virt in jobs:
        for t in (dz, inp) + tuple(virt or ()):
            _keepalive.cross_stream(t, side)
    _STATE["forked"].add(key)


def active() -> bool:
    return _STATE["active"]


def join_at_exit(stream):
    """An operator's backward left work on `stream` that nothing downstream is certain to wait for (the consumer may be
    frozen): the block's exit makes the current stream wait for it.  Only inside an active block."""
    assert _STATE["active"]
    if all(stream is not s for s in _STATE["extra"]):
        _STATE["extra"].append(stream)


def defer_weight_grad(dz, inp, weight, virt=None):
    """Queue dW = dz^T @ inp for the leaf parameter ``weight`` ([O,K]); dz [N,O], inp [N,K] contiguous fp32.
    ``virt`` = (aud, eye_pre, enc_a, enc_e): the input rows were never stored, they are cat(inp, aud * enc_a,
    relu(eye_pre) * enc_e) (glue._GlueSigma; instag_linear_weight_grad_batched_glue assembles them while loading)."""
    _STATE["jobs"].append((dz, inp, weight, virt))


def _flush(jobs):
    from . import mlp
    dws = mlp.weight_grads([(dz, inp, virt) for dz, inp, _, virt in jobs])
    for (_, _, w, _), dw in zip(jobs, dws):
        dw = dw.reshape(w.shape).to(w.dtype)
        w.grad = dw if w.grad is None else w.grad.add_(dw)


_ONE = {}


def root_gradient(loss):
    """The scalar one a backward pass starts from, cached per (device, dtype): no fill launch per step.  A tensor made
    while a capture runs belongs to that graph's memory pool, so it is never cached."""
    key = (loss.device, loss.dtype)
    one = _ONE.get(key)
    if one is None:
        one = torch.ones((), dtype=loss.dtype, device=loss.device)
        if not torch.cuda.is_current_stream_capturing():
            _ONE[key] = one
    return one


def backward(loss, device):
    """loss.backward() with the MLPs' weight-gradient GEMMs batched into one launch behind it; on the device the root
    gradient is root_gradient(loss)."""
    with deferred_grads(device if device.type == "cuda" else None):
        if device.type == "cuda" and loss.dim() == 0:
            loss.backward(gradient=root_gradient(loss))
        else:
            loss.backward()


class deferred_grads:
    def __init__(self, device):
        self.device = None if device is None else torch.device(device)
        self.on = self.device is not None and self.device.type == "cuda"

    def __enter__(self):
        self.prev = _STATE["active"]
        if self.on:
            _STATE["active"] = True
            from . import diff_gauss
            self.prev_aux = diff_gauss.DEFER_AUX_JOIN
            diff_gauss.DEFER_AUX_JOIN = True       # joined by the glue operator, at the latest on exit below
        return self

    def __exit__(self, exc_type, exc, tb):
        _STATE["active"] = self.prev
        if self.on:
            from . import diff_gauss
            diff_gauss.DEFER_AUX_JOIN = self.prev_aux
            diff_gauss.join_pending_aux(final=True)
        if not self.on or self.prev:
            return False
        jobs, _STATE["jobs"] = _STATE["jobs"], []
        if exc_type is None and jobs:
            _flush(jobs)
        for typ, idx in _STATE["forked"]:
            torch.cuda.current_stream(torch.device(typ, idx)).wait_stream(_STATE["streams"][(typ, idx)])
        _STATE["forked"] = set()
        for st in _STATE["extra"]:
            torch.cuda.current_stream(st.device).wait_stream(st)
        _STATE["extra"] = []
        return False
