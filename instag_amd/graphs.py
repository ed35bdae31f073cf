"""The one protocol by which the package captures a step into a hipGraph: the face step (train.GraphedStep), the mouth
and fuse steps (GraphedStage) and the streaming inference renderer (infer.FuseRenderer).  A captured step runs the
rasterizer in its sync-free capacity mode (diff_gauss.CapacityPlan: one fixed instance capacity per rasterizer call):
``measure`` the eager instance counts, size the capacities by the caller's rule, ``install`` a plan, ``warm`` up and
``capture``; on replay the caller looks at the sticky overflow flags every CHECK_EVERY replays (``check_due``).

Rules that answer capture crashes on ROCm 7.2:
  * nothing a captured step allocated is released inside the capture window (frees there intermittently crash
    hipStreamEndCapture): callers drop the step's package after the ``with``;
  * a captured step's outputs are kept DETACHED, and no warm-up step's loss outlives its step: a live loss keeps the
    step's autograd graph, and with it every parameter's AccumulateGrad node, bound to the stream it ran on -- the next
    backward on any other stream (the capture, an eager step, an instrumented pass) then hops to that stream for every
    parameter;
  * no cyclic garbage collection inside the window (``_no_gc``);
  * a body that raises has its traceback printed before the capture is torn down: ending an invalidated capture can
    crash the process, which would hide the message.
"""
from __future__ import annotations

import gc
import sys
import traceback
from contextlib import contextmanager

import torch

from . import _lib, diff_gauss


@contextmanager
def _no_gc(collect: bool = True):
    """No cyclic garbage collection inside a stream-capture window.  The crash this once papered over (a segmentation
    fault in capture_end) is addressed at its cause in instag_amd/_keepalive.py: tensors that cross streams are no
    longer marked with record_stream inside a capture, the capture's owner keeps them alive until it has ended.  The
    collector stays off during the window all the same: a collection there frees an earlier step's blocks into the
    capture's private pool at an arbitrary point of the captured sequence, which makes captures irreproducible.
    ``collect=False`` (re-captures inside a train loop): no full collection in front either -- it costs tens of
    milliseconds, as much as ten train steps."""
    was = gc.isenabled()
    if collect:
        gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


# ---- capacity sizing: each caller's own rule (the capacity also picks the blend kernel, raster_blend.hip) ------------
def face_capacity(counts, headroom: float, min_capacity: int = 0) -> int:
    """Face step, cold capture: both slots get the largest instance count of a step's LAST rasterizer call."""
    return max(int(max(c[-1] for c in counts) * headroom) + 4096, int(min_capacity))


def stage_capacities(counts, headroom: float):
    """Mouth and fuse steps: slot k gets the largest instance count of the step's k-th rasterizer call."""
    return [int(max(col) * headroom) + 4096 for col in zip(*counts)]


def inference_capacities(counts, headroom: float, n_face: int, n_mouth: int, frames: int):
    """Inference, ``frames`` frames of two rasterizer calls each: the last call of a frame renders the mouth; every
    slot is sized for the larger scene from it."""
    cap = int(max(c[-1] for c in counts) * headroom * max(1.0, n_face / max(1, n_mouth))) + 4096
    return [cap, cap] * frames


# ---- the protocol's steps --------------------------------------------------------------------------------------------
def measure(step, steps: int, pre=None):
    """Run ``steps`` eager steps with no plan installed -> per step, the instance count of every rasterizer call.
    ``pre()`` = the host-side part of a step (iteration counter, learning-rate table), run before each."""
    diff_gauss.set_capacity_plan(None)
    counts = []
    for _ in range(steps):
        diff_gauss.RENDERED_LOG.clear()
        if pre is not None:
            pre()
        step()
        counts.append(list(diff_gauss.RENDERED_LOG))
    return counts


def install(capacities, device) -> diff_gauss.CapacityPlan:
    """A plan with one slot per rasterizer call of a step, installed for every subsequent rasterizer call."""
    plan = diff_gauss.CapacityPlan(capacities, device)
    diff_gauss.set_capacity_plan(plan)
    return plan


def warm(plan, step, device, pre=None):
    """Two capacity-mode steps on the warm-up stream, joined back into the current stream; synchronises the device."""
    s = _lib.warmup_stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        for _ in range(2):
            plan.begin_step()
            if pre is not None:
                pre()
            step()
    torch.cuda.current_stream(device).wait_stream(s)
    torch.cuda.synchronize(device)


@contextmanager
def capture(graph, plan, collect: bool = True, **options):
    """Capture ``graph`` on the package's capture stream (_lib.graph_capture with the caller's ``pool`` / ``light`` /
    ``capture_error_mode``); ``collect``: a full garbage collection in front of the window."""
    plan.begin_step()
    with _no_gc(collect), _lib.graph_capture(graph, **options):
        try:
            yield
        except BaseException:
            traceback.print_exc()
            sys.stderr.flush()
            raise


def begin_eager_step():
    """An eager step while a plan is still installed: its rasterizer calls take the plan's slots from the first."""
    if diff_gauss._CAPACITY_PLAN is not None:
        diff_gauss._CAPACITY_PLAN.begin_step()


def drop_plan(*steps):
    """Clear the installed plan if any of an owner's captured ``steps`` exists (its next steps launch eagerly)."""
    if any(s is not None for s in steps):
        diff_gauss.set_capacity_plan(None)


class CapturedStep:
    """A step captured under ``self.plan``; counts its replays for the periodic look at the overflow flags."""
    CHECK_EVERY = 64         # replays between two looks at the (sticky, device-side) overflow flags
    _replays = 0

    def check_overflow(self):
        """Host-side (synchronising) check that no replayed step exceeded the instance capacity (the device flag is
        sticky: every step since the capture / the last clear counts)."""
        return self.plan.overflowed()

    def check_due(self) -> bool:
        """True every CHECK_EVERY replays -- a function of the replay count alone, hence the same step on every rank."""
        if self._replays < self.CHECK_EVERY:
            return False
        self._replays = 0
        return True


class GraphedStage(CapturedStep):
    """A stage trainer's whole step (forward, loss, backward, statistics, optimizers) in one graph.  ``body(frame) ->
    (outputs..., keepalive)`` must be free of host round trips; ``size(counts)`` is the caller's sizing rule: the
    per-step instance counts of ``warmup_steps`` eager steps -> one capacity per rasterizer call of the step."""

    def __init__(self, body, example, device, size, warmup_steps: int = 2, pre=None):
        assert device.type == "cuda", "graph mode needs the GPU"
        self.static = example.clone_static()
        step = lambda: body(self.static)
        self.capacities = size(measure(step, max(1, warmup_steps), pre))
        self.plan = install(self.capacities, device)
        warm(self.plan, step, device, pre)
        self.graph = torch.cuda.CUDAGraph()
        with capture(self.graph, self.plan):
            out = body(self.static)
        self.out = tuple(o.detach() if torch.is_tensor(o) else o for o in out[:-1])

    def replay(self, frame):
        self.static.copy_from(frame)
        self.graph.replay()
        self._replays += 1
        return self.out

    def overflow_due(self):
        """True every CHECK_EVERY replays if some rasterizer call of a replayed step needed more instances than its
        capacity: the caller drops the graph -- steps run eagerly, or are captured again with larger capacities."""
        return self.check_due() and bool(self.plan.poll_overflow())     # asynchronous: the previous poll's answer
