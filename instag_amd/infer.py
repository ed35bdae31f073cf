"""Forward-only streaming render of the fused head (face + mouth), the inference path of the reference
(synthesize_fuse.py:34-92: per view ``render_motion`` + ``render_motion_mouth_con(inference=True)`` + compositing).

``FuseRenderer.render(frame)`` runs the same operators as training under ``torch.no_grad``; ``enable_graph`` captures
the whole frame (both rasterizer passes in sync-free capacity mode, packed frame inputs) into one hipGraph so that a
frame costs one small copy and one graph launch.

Streaming ("batch frames per launch"): ``enable_graph(frames_per_replay=K)`` captures K frames into ONE
graph, each on a stream of its own.  A frame's kernels are bound by serial chains (one workgroup per populated tile
walking its list, ~400 of them on 256 CUs), so K independent frames overlap almost for free: ``render_batch`` feeds K
frames with K small copies and one launch and returns the K images.
"""
from __future__ import annotations

import torch

from . import _lib, diff_gauss, graphs
from .renderer import render_fuse
from .train import Frame


class FuseRenderer:
    def __init__(self, gaussians, motion_net, gaussians_mouth, motion_net_mouth, background, personalized=False,
                 dilate: int = 1, as_uint8: bool = False):
        """``dilate`` (odd, 1 = off; synthesize_fuse.py --dilate is 13): the scene background shows through the mouth
        pass where the dilate x dilate maximum of its alpha is below one.  ``as_uint8``: ``render`` / ``render_batch``
        also return the frames as the reference writes them, uint8 [H,W,3] (synthesize_fuse.py:76).  With either set
        the frame is composed by metrics.infer_compose (one launch: dilation, composition, clamp, bytes)."""
        self.g, self.net, self.gm, self.netm = gaussians, motion_net, gaussians_mouth, motion_net_mouth
        self.bg = background
        self.personalized = personalized
        self.dilate, self.as_uint8 = int(dilate), bool(as_uint8)
        if self.dilate < 1 or self.dilate > 31 or self.dilate % 2 == 0:
            raise ValueError(f"FuseRenderer: dilate must be odd and in 1 .. 31, got {dilate}")
        self.frames_per_replay = 1
        self._graph = None

    @torch.no_grad()
    def _render(self, frame: Frame, scene_background=None):
        """-> image, or (image, frame_u8) with ``as_uint8``."""
        if self.dilate != 1 or self.as_uint8:
            from .metrics import infer_compose
            out = render_fuse(frame, self.g, self.net, self.gm, self.netm, None, self.bg, personalized=self.personalized,
                              inference=True, compose=False)
            face, mouth = out["face"], out["mouth"]
            image, u8 = infer_compose(face["render"], face["alpha"], mouth["render"], mouth["alpha"], self.bg,
                                      scene_background, self.dilate, self.as_uint8)
            return (image, u8) if self.as_uint8 else image
        out = render_fuse(frame, self.g, self.net, self.gm, self.netm, None, self.bg,
                          scene_background=scene_background, personalized=self.personalized, inference=True)
        return out["image"].clamp(0, 1)

    def render(self, frame: Frame, scene_background=None):
        """-> image [3,H,W] in [0,1] (with ``as_uint8``: (image, frame uint8 [H,W,3])).  With a captured graph the
        returned tensors are the graph's static output buffers (valid until the next call)."""
        if self._graph is None:
            return self._render(frame, scene_background)
        out = self.render_batch([frame], None if scene_background is None else [scene_background])
        return (out[0][0], out[1][0]) if self.as_uint8 else out[0]

    def render_batch(self, frames, scene_backgrounds=None):
        """-> images [len(frames),3,H,W].  With a captured graph of K frames per replay the frames go through in
        groups of K (one launch per group; a short last group is padded with its last frame); the returned tensor
        is a copy only when more than one group was needed.  With ``as_uint8``: (images, frames uint8
        [len(frames),H,W,3])."""
        if self._graph is None:
            outs = [self._render(f, None if scene_backgrounds is None else scene_backgrounds[i])
                    for i, f in enumerate(frames)]
            if self.as_uint8:
                return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
            return torch.stack(outs)
        K = len(self._static)
        outs, outs_u8 = [], []
        for g0 in range(0, len(frames), K):
            group = frames[g0:g0 + K]
            for k in range(K):
                j = min(g0 + k, len(frames) - 1)
                self._static[k].copy_from(frames[j])
                if scene_backgrounds is not None:
                    self._static_bg[k].copy_(scene_backgrounds[j], non_blocking=True)
            self._plan.begin_step()
            self._graph.replay()
            if len(frames) <= K:
                return (self._out[:len(group)], self._out_u8[:len(group)]) if self.as_uint8 else self._out[:len(group)]
            outs.append(self._out[:len(group)].clone())
            if self.as_uint8:
                outs_u8.append(self._out_u8[:len(group)].clone())
        return (torch.cat(outs), torch.cat(outs_u8)) if self.as_uint8 else torch.cat(outs)

    def enable_graph(self, example: Frame, headroom: float = 1.5, frames_per_replay: int = 1):
        dev = self.bg.device
        K = max(1, int(frames_per_replay))
        self._static = [example.clone_static() for _ in range(K)]
        self._static_bg = [torch.zeros(3, example.image_height, example.image_width, device=dev) for _ in range(K)]
        counts = graphs.measure(lambda: self._render(self._static[0], self._static_bg[0]), 2)
        self._plan = graphs.install(graphs.inference_capacities(counts, headroom, self.g.num_points,
                                                                self.gm.num_points, K), dev)
        lanes = [_lib.side_stream(dev, ("infer_lane", k)) for k in range(K)]

        def all_frames():
            """frame k on lane k, forked from / joined into the current stream.  (On a forked lane the operators keep
            their own work on that one stream -- _lib.may_fork: a fork of a fork inside a capture crashes
            hipStreamEndCapture on ROCm 7.2; the lanes provide the concurrency instead.)"""
            if K == 1:
                return [self._render(self._static[0], self._static_bg[0])]
            main = torch.cuda.current_stream(dev)
            outs = []
            for k in range(K):
                lanes[k].wait_stream(main)
                with torch.cuda.stream(lanes[k]):
                    outs.append(self._render(self._static[k], self._static_bg[k]))
            for k in range(K):
                main.wait_stream(lanes[k])
            return outs

        graphs.warm(self._plan, all_frames, dev)
        self._graph = torch.cuda.CUDAGraph()
        with graphs.capture(self._graph, self._plan):
            outs = all_frames()
            if self.as_uint8:
                self._out = torch.stack([o[0] for o in outs])
                self._out_u8 = torch.stack([o[1] for o in outs])
            else:
                self._out = torch.stack(outs)
        self._lanes = lanes
        self.frames_per_replay = K
        return self

    def check_overflow(self):
        return self._plan.overflowed() if self._graph is not None else []

    def close(self):
        self._graph = None
        self.frames_per_replay = 1
        diff_gauss.set_capacity_plan(None)
