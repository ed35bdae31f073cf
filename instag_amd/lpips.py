"""LPIPS (AlexNet, eval mode) and the patch loss the late face and fuse phases add.

The `lpips` package's criterion with ``net='alex'`` (restated by the reference in lpipsPyTorch/modules/{lpips,networks,
utils}.py), on the square patches ``F.unfold(img[None], p, stride=p)`` cuts (utils/loss_utils.py:22-24):
train_face.py:596-620 (lips rectangle filled with the background colour, p = 64..96, weight 0.01) and
train_fuse_con.py:186-193 (p = 32..42, weight 0.05).

    w = LPIPSWeights.load("alexnet.pth", "alex.pth")         # the two files a user of the lpips package already has
    term = PatchLPIPS(w, H, W, 64, 96)(image, gt, p, lips_rect, bg)

On the GPU the whole term -- forward and the gradient with respect to the image -- runs in csrc/lpips.hip; the
``*_torch`` functions are the plain-torch statement of the same arithmetic (any dtype, CPU or GPU) that the tests
compare against and the CPU path uses.  The project ships no weights and fetches none.
"""
from __future__ import annotations

import ctypes as C
import random
from typing import Optional

import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CHANNELS = (64, 192, 384, 256, 256)
FEATURES = (0, 3, 6, 8, 10)                       # torchvision alexnet.features indices of the five convolutions
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
MIN_PATCH = 31                                    # below it the second 3x3 pool window no longer fits

FACE_LPIPS_WEIGHT, FACE_PATCH_RANGE = 0.01, (64, 96)        # train_face.py:609,617
FUSE_LPIPS_WEIGHT, FUSE_PATCH_RANGE = 0.05, (32, 42)        # train_fuse_con.py:192-193


# ---- schedule ---------------------------------------------------------------------------------------------------------
def face_lpips_start(opt) -> int:
    """train_face.py:42: lpips_start_iter = densify_until_iter - 1500."""
    return opt.densify_until_iter - 1500


def face_lpips_on(iteration: int, opt) -> bool:
    """train_face.py:333,596: the mouth mask is closed and the patch term added when iteration > lpips_start_iter."""
    return iteration > face_lpips_start(opt)


def fuse_lpips_start(opt) -> int:
    """train_fuse_con.py:42: lpips_start_iter = iterations / 2."""
    return opt.iterations // 2


def fuse_lpips_on(iteration: int, opt) -> bool:
    return iteration > fuse_lpips_start(opt)


def draw_face_patch(rng: random.Random) -> int:
    """train_face.py:609."""
    return rng.randint(32, 48) * 2


def draw_fuse_patch(rng: random.Random) -> int:
    """train_fuse_con.py:192."""
    return rng.randint(16, 21) * 2


def close_mask(mask: torch.Tensor) -> torch.Tensor:
    """train_face.py:333-335: a 3x3 max-pool, then a 3x3 min-pool, of a boolean [H,W] mask."""
    m = mask[None, None].float()
    m = F.max_pool2d(m, 3, 1, 1)
    m = -F.max_pool2d(-m, 3, 1, 1)
    return m[0, 0].bool()


# ---- weights ----------------------------------------------------------------------------------------------------------
class LPIPSWeights:
    """The frozen parameters: ``conv[l] = (weight, bias)`` of AlexNet's five convolutions and ``lin[l]`` = the [C_l]
    weights of the 1x1 convolutions.  Kept in fp32 on the CPU; device copies in the kernels' layouts are made once per
    device (``device_pack``)."""

    def __init__(self, conv, lin):
        assert len(conv) == 5 and len(lin) == 5
        self.conv = [(w.detach().float().contiguous().cpu(), b.detach().float().contiguous().cpu()) for w, b in conv]
        self.lin = [l.detach().float().reshape(-1).contiguous().cpu() for l in lin]
        for (w, b), l, shape in zip(self.conv, self.lin, CONV_SHAPES):
            if tuple(w.shape) != shape or tuple(b.shape) != shape[:1] or tuple(l.shape) != shape[:1]:
                raise ValueError(f"LPIPS weights: expected a {shape} convolution, got {tuple(w.shape)}, "
                                 f"bias {tuple(b.shape)}, lin {tuple(l.shape)}")
        self._packs = {}

    @classmethod
    def from_state_dicts(cls, alexnet_sd, lin_sd) -> "LPIPSWeights":
        """``alexnet_sd``: torchvision's ``features.{0,3,6,8,10}.{weight,bias}``; ``lin_sd``: the lpips package's
        ``lin{0..4}.model.1.weight`` or the renamed ``{0..4}.1.weight`` of lpipsPyTorch/modules/utils.py:22-29."""
        conv = [(alexnet_sd[f"features.{i}.weight"], alexnet_sd[f"features.{i}.bias"]) for i in FEATURES]
        lin = []
        for l in range(5):
            for key in (f"lin{l}.model.1.weight", f"{l}.1.weight"):
                if key in lin_sd:
                    lin.append(lin_sd[key])
                    break
            else:
                raise KeyError(f"lin{l}.model.1.weight")
        return cls(conv, lin)

    @classmethod
    def load(cls, alex_path, lin_path) -> "LPIPSWeights":
        return cls.from_state_dicts(torch.load(alex_path, map_location="cpu"), torch.load(lin_path, map_location="cpu"))

    @classmethod
    def random(cls, seed: int = 0) -> "LPIPSWeights":
        """Seeded stand-ins with the scale of trained ones (tests, benches): He-style convolutions, small biases,
        non-negative lin weights as the package's are."""
        g = torch.Generator().manual_seed(seed)
        conv = []
        for co, ci, kh, kw in CONV_SHAPES:
            w = torch.randn(co, ci, kh, kw, generator=g) * (2.0 / (ci * kh * kw)) ** 0.5
            conv.append((w, torch.randn(co, generator=g) * 0.05))
        lin = [torch.rand(c, generator=g) * (2.0 / c) for c in CHANNELS]
        return cls(conv, lin)

    def to(self, device=None, dtype=None):
        """(conv, lin) lists of tensors for the torch statement."""
        conv = [(w.to(device=device, dtype=dtype), b.to(device=device, dtype=dtype)) for w, b in self.conv]
        return conv, [l.to(device=device, dtype=dtype) for l in self.lin]

    def device_pack(self, device):
        """struct instag_lpips_weights for ``device`` (and the tensors it points into)."""
        from . import _lib
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        pack = self._packs.get(key)
        if pack is not None:
            return pack
        keep, s = [], _lib.LpipsWeights()
        for l, (w, b) in enumerate(self.conv):
            co, ci, kh, kw = w.shape
            K = ci * kh * kw
            wf = torch.zeros((K + 31) // 32 * 32, co)
            wf[:K] = w.reshape(co, K).t()
            # data gradient of a stride-1 layer = the same convolution with [(cout, ky, kx)][cin] of the flipped weight
            wb = w if l == 0 else w.flip(2, 3).permute(0, 2, 3, 1).reshape(co * kh * kw, ci)
            ts = [t.contiguous().to(device) for t in (wf, b, wb, self.lin[l])]
            keep += ts
            s.wf[l], s.bias[l], s.wb[l], s.lin[l] = [t.data_ptr() for t in ts]
        pack = self._packs[key] = (s, keep)
        return pack


# ---- plain-torch statement -------------------------------------------------------------------------------------------
def _features(v, conv):
    taps = []
    v = F.relu(F.conv2d(v, conv[0][0], conv[0][1], stride=4, padding=2)); taps.append(v)
    v = F.max_pool2d(v, 3, 2)
    v = F.relu(F.conv2d(v, conv[1][0], conv[1][1], padding=2)); taps.append(v)
    v = F.max_pool2d(v, 3, 2)
    for l in (2, 3, 4):
        v = F.relu(F.conv2d(v, conv[l][0], conv[l][1], padding=1)); taps.append(v)
    return taps


def _normalize_activation(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def lpips_torch(x, y, w: LPIPSWeights):
    """lpips.LPIPS(net='alex')(x, y) for x, y [N,3,h,w] in [-1,1] -> [N,1,1,1]."""
    conv, lin = w.to(x.device, x.dtype)
    shift = torch.tensor(SHIFT, dtype=x.dtype, device=x.device)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=x.dtype, device=x.device)[None, :, None, None]
    fx, fy = _features((x - shift) / scale, conv), _features((y - shift) / scale, conv)
    res = []
    for a, b, l in zip(fx, fy, lin):
        d = (_normalize_activation(a) - _normalize_activation(b)) ** 2
        res.append(F.conv2d(d, l[None, :, None, None]).mean((2, 3), True))
    return torch.sum(torch.cat(res, 0).view(5, -1, 1, 1, 1), 0)


def patchify(img, p: int):
    """utils/loss_utils.py:22-24 for one [3,H,W] image -> [n,3,p,p]."""
    return F.unfold(img[None], kernel_size=p, stride=p).permute(0, 2, 1).reshape(-1, 3, p, p)


def patch_lpips_torch(image, gt, p: int, w: LPIPSWeights, lips_rect=None, bg=None):
    """train_face.py:606-620 (with ``lips_rect``) / train_fuse_con.py:192-193 without the weight: the mean LPIPS of the
    p x p patches of ``image`` and ``gt`` ([3,H,W] in [0,1]) -> 0-d tensor."""
    p = int(p)
    if lips_rect is not None:
        r0, r1, c0, c1 = [int(v) for v in (lips_rect.tolist() if torch.is_tensor(lips_rect) else lips_rect)]
        image, gt = image.clone(), gt.clone()
        image[:, r0:r1, c0:c1] = bg[:, None, None].to(image.dtype)
        gt[:, r0:r1, c0:c1] = bg[:, None, None].to(gt.dtype)
    return lpips_torch(patchify(image * 2 - 1, p), patchify(gt * 2 - 1, p), w).mean()


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class _Plan:
    """Workspace and launch geometry for one (H, W, [p_min, p_max]) -- or one stack of n p x p patches -- on one device."""

    def __init__(self, w: LPIPSWeights, device, H, W, p_min, p_max, n_stack=0):
        from . import _lib
        self.L = _lib.lib()
        self.args = (int(H), int(W), int(p_min), int(p_max), int(n_stack))
        nbytes = _lib.workspace_bytes(self.L.instag_lpips_workspace_bytes(*self.args))
        self.device = torch.device(device)
        self.n_max = self.L.instag_lpips_max_patches(*self.args)
        self.struct, self._keep = w.device_pack(self.device)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.nbytes = nbytes
        self.p_dev = torch.full((1,), p_min, dtype=torch.int32, device=self.device)
        self.generation = 0        # forwards so far: a backward must belong to the LAST one (its activations are in ws)

    def forward(self, image, gt, p_dev, p_host, rect, bg, want_mean):
        from . import _lib
        per = torch.empty(self.n_max, dtype=torch.float32, device=self.device)
        mean = torch.empty((), dtype=torch.float32, device=self.device) if want_mean else None
        H, W, p_min, p_max, n_stack = self.args
        self.generation += 1
        _lib.check(self.L.instag_lpips_forward(C.byref(self.struct), _lib.ptr(image), _lib.ptr(gt), _lib.ptr(p_dev),
                                               p_host, _lib.ptr(rect), _lib.ptr(bg), H, W, p_min, p_max, n_stack,
                                               _lib.ptr(self.ws), self.nbytes, _lib.ptr(per), _lib.ptr(mean),
                                               _lib.current_stream()), "lpips_forward")
        return per, mean

    def backward(self, p_dev, p_host, rect, g, per_patch, like, generation):
        from . import _lib
        if generation != self.generation:
            raise RuntimeError("LPIPS backward: the operator ran another forward since this one and its saved "
                               "activations are gone; run backward before the next call, or use one operator "
                               "(PatchLPIPS / LPIPS object) per term")
        d = torch.empty_like(like)
        H, W, p_min, p_max, n_stack = self.args
        _lib.check(self.L.instag_lpips_backward(C.byref(self.struct), _lib.ptr(p_dev), p_host, _lib.ptr(rect),
                                                _lib.ptr(g), int(per_patch), H, W, p_min, p_max, n_stack,
                                                _lib.ptr(self.ws), self.nbytes, _lib.ptr(d), _lib.current_stream()),
                   "lpips_backward")
        return d


class _PatchLPIPSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, plan, p_dev, p_host, rect, bg):
        image = image.contiguous().float()
        _, mean = plan.forward(image, gt.detach().contiguous().float(), p_dev, p_host, rect, bg, True)
        ctx.plan, ctx.p_dev, ctx.p_host, ctx.rect, ctx.like = plan, p_dev, p_host, rect, image
        ctx.generation = plan.generation
        return mean

    @staticmethod
    def backward(ctx, g):
        d = ctx.plan.backward(ctx.p_dev, ctx.p_host, ctx.rect, g.contiguous().float(), False, ctx.like,
                              ctx.generation)
        return d, None, None, None, None, None, None


class _StackLPIPSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, plan):
        x = x.contiguous().float()
        per, _ = plan.forward(x, y.detach().contiguous().float(), plan.p_dev, plan.args[2], None, None, False)
        ctx.plan, ctx.like, ctx.generation = plan, x, plan.generation
        return per[:x.shape[0]].view(-1, 1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        d = plan.backward(plan.p_dev, plan.args[2], None, g.contiguous().float().view(-1), True, ctx.like,
                          ctx.generation)
        return d, None, None


class PatchLPIPS:
    """``(image, gt, p, lips_rect=None, bg=None) -> mean LPIPS of the p x p patches`` (0-d tensor) for [3,H,W] images
    in [0,1], differentiable in ``image``; p in [p_min, p_max].

    On the GPU the operator's buffers and grids are sized for the whole range and the kernels read p from device
    memory, so a captured call serves every patch size: pass ``p`` as a device integer tensor (its first element is
    read on every replay; ``stage(p)`` validates a value and writes it into the operator's own scalar ``p_dev``), and
    ``lips_rect`` as a device int32 tensor (r0, r1, c0, c1).  One forward's saved activations are overwritten by the
    next: run backward before calling again (a stale backward raises).  On the CPU the call is ``patch_lpips_torch``."""

    def __init__(self, w: LPIPSWeights, H: int, W: int, p_min: int, p_max: int):
        if p_min < MIN_PATCH:
            raise ValueError(f"PatchLPIPS: a patch below {MIN_PATCH} pixels leaves no room for the second pool window")
        if p_max < p_min or min(H, W) < p_max:
            raise ValueError(f"PatchLPIPS: patch range [{p_min}, {p_max}] does not fit a {H}x{W} image")
        self.w, self.H, self.W, self.p_min, self.p_max = w, int(H), int(W), int(p_min), int(p_max)
        self._plans = {}

    def _plan(self, device) -> _Plan:
        key = (device.type, device.index)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = _Plan(self.w, device, self.H, self.W, self.p_min, self.p_max)
        return plan

    def check(self, p: int) -> int:
        p = int(p)
        if not self.p_min <= p <= self.p_max:
            raise ValueError(f"PatchLPIPS: patch size {p} outside the declared range [{self.p_min}, {self.p_max}]")
        return p

    def p_dev(self, device):
        return self._plan(torch.device(device)).p_dev

    def stage(self, p: int, device):
        """Write ``p`` into the operator's device scalar (outside a capture) and return that scalar."""
        t = self.p_dev(device)
        t.fill_(self.check(p))
        return t

    def __call__(self, image, gt, p, lips_rect=None, bg=None):
        assert tuple(image.shape) == (3, self.H, self.W) and tuple(gt.shape) == (3, self.H, self.W), \
            f"PatchLPIPS was built for [3,{self.H},{self.W}] images"
        if lips_rect is not None and bg is None:
            raise ValueError("PatchLPIPS: a lips rectangle needs the background colour")
        if not image.is_cuda:
            if torch.is_tensor(p):
                p = int(p.reshape(-1)[0])
            return patch_lpips_torch(image, gt, self.check(p), self.w, lips_rect, bg)
        dev = image.device
        plan = self._plan(dev)
        if torch.is_tensor(p):
            p_host = -1
            p_dev = p.reshape(-1)
            if p_dev.dtype == torch.int64:
                p_dev = p_dev[:1].view(torch.int32)        # (little endian: the low word; patch sizes are positive)
            assert p_dev.dtype == torch.int32 and p_dev.device == dev, "p: a device int32 / int64 tensor"
        else:
            p_host = self.check(p)
            p_dev = self.stage(p_host, dev)
        rect = None
        if lips_rect is not None:
            rect = lips_rect if torch.is_tensor(lips_rect) else torch.tensor([int(v) for v in lips_rect])
            rect = rect.to(device=dev, dtype=torch.int32).contiguous()
            bg = bg.to(device=dev, dtype=torch.float32).contiguous()
        return _PatchLPIPSFn.apply(image, gt, plan, p_dev, p_host, rect, bg if rect is not None else None)


class LPIPS:
    """Callable as the package's criterion: ``(x, y) -> [N,1,1,1]`` for patches [N,3,h,w] in [-1,1] (differentiable
    in x).  The drop-in for code that holds patches already; the HIP path takes square patches of at least 31 pixels.
    One object keeps the activations of its LAST forward per (device, N, h): run backward before calling it again with
    the same shape (a stale backward raises), or build one LPIPS object per term of a loss that sums several."""

    def __init__(self, w: LPIPSWeights):
        self.w = w
        self._plans = {}

    def __call__(self, x, y):
        assert x.dim() == 4 and x.shape[1] == 3 and x.shape == y.shape, "LPIPS: x, y of one shape [N,3,h,w]"
        if not x.is_cuda:
            return lpips_torch(x, y, self.w)
        N, _, h, wd = x.shape
        if h != wd or h < MIN_PATCH:
            raise ValueError(f"LPIPS: the HIP operator takes square patches of at least {MIN_PATCH} pixels, got {h}x{wd}")
        key = (x.device.type, x.device.index, N, h)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = _Plan(self.w, x.device, h, h, h, h, n_stack=N)
        return _StackLPIPSFn.apply(x, y, plan)
