"""Face parsing on the device: from ``ori_imgs/<i>.jpg`` to ``parsing/<i>.png`` (csrc/parsing.hip).

The reference makes the parsing maps with data_utils/face_parsing/test.py:72-106: a BiSeNet over ResNet-18 (model.py,
resnet.py; weights ``data_utils/face_parsing/79999_iter.pth``) in eval mode on the frame resized to 512x512, ``argmax``
over its 19 classes, and ``vis_parsing_maps``' colour table written through OpenCV.  Here:

    w = BiSeNetWeights.load("79999_iter.pth")                     # the file a user of the reference already has
    parsing = parse_identity(path, w, "cuda")                      # reads ori_imgs/*.jpg, writes parsing/*.png
    bc, gt, torso = prepare_identity(path, "cuda", parsing=parsing)

On the GPU the network, the bilinear upsample, the argmax and the colour table run in csrc/parsing.hip (inference only,
fp32, as the reference runs it); ``bisenet_torch``, ``labels_torch``, ``colour_map_torch`` and ``parse_torch`` are the
plain-torch statement of the same arithmetic (any dtype, CPU or GPU) that the tests compare against and a CPU device
uses.  The project ships no weights and fetches none.

Colours are RGB as PIL and prepare.py read the file (the reference paints BGR for ``cv2.imwrite``): class 0 white
(background), 1-10, 12, 13 and 18 blue (head; 18 because ``range(18, num_of_class + 1)`` repaints it whenever it occurs),
11 grey (100,100,100), 14 and 15 green (neck), 16 red (torso), 17 black.

Unpinned against the reference's libraries: the nearest resize of the colour map to a frame size other than the parsed
one follows the integer rule ``src = min((dst * n_src) // n_dst, n_src - 1)`` per axis (``cv2.INTER_NEAREST`` is not
available to check against; the rule is the identity for the 512x512 frames InsTaG uses), and the resize of a non-512
frame to 512x512 is PIL's ``Image.BILINEAR`` on the host, as in the reference.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn.functional as F

N_CLASSES = 19
BN_EPS = 1e-5
SIZE = 512                                           # test.py:94
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MIN_SIDE, SIDE_MULTIPLE = 64, 32

# RGB colour of every class
COLOURS = np.array([(255, 255, 255)] + [(0, 0, 255)] * 10 + [(100, 100, 100)] + [(0, 0, 255)] * 2 + [(0, 255, 0)] * 2
                   + [(255, 0, 0), (0, 0, 0), (0, 0, 255)], dtype=np.uint8)


def _block(prefix, cin, cout, stride):
    out = [(f"{prefix}.conv1", f"{prefix}.bn1", cin, cout, 3, stride),
           (f"{prefix}.conv2", f"{prefix}.bn2", cout, cout, 3, 1)]
    if cin != cout or stride != 1:
        out.append((f"{prefix}.downsample.0", f"{prefix}.downsample.1", cin, cout, 1, stride))
    return out


def _layers():
    r = "cp.resnet"
    out = [(f"{r}.conv1", f"{r}.bn1", 3, 64, 7, 2)]
    for stage, (cin, cout) in enumerate(((64, 64), (64, 128), (128, 256), (256, 512)), start=1):
        out += _block(f"{r}.layer{stage}.0", cin, cout, 1 if stage == 1 else 2)
        out += _block(f"{r}.layer{stage}.1", cout, cout, 1)
    out += [("cp.arm32.conv.conv", "cp.arm32.conv.bn", 512, 128, 3, 1),
            ("cp.arm16.conv.conv", "cp.arm16.conv.bn", 256, 128, 3, 1),
            ("cp.conv_head32.conv", "cp.conv_head32.bn", 128, 128, 3, 1),
            ("cp.conv_head16.conv", "cp.conv_head16.bn", 128, 128, 3, 1),
            ("ffm.convblk.conv", "ffm.convblk.bn", 256, 256, 1, 1),
            ("conv_out.conv.conv", "conv_out.conv.bn", 256, 256, 3, 1),
            ("conv_out.conv_out", None, 256, N_CLASSES, 1, 1),
            # the [B,C]-sized products behind the global average pools
            ("cp.conv_avg.conv", "cp.conv_avg.bn", 512, 128, 1, 1),
            ("cp.arm32.conv_atten", "cp.arm32.bn_atten", 128, 128, 1, 1),
            ("cp.arm16.conv_atten", "cp.arm16.bn_atten", 128, 128, 1, 1),
            ("ffm.conv1", None, 256, 64, 1, 1),
            ("ffm.conv2", None, 64, 256, 1, 1)]
    return tuple(out)


# (convolution, its BatchNorm or None, cin, cout, kernel, stride) in the order of struct instag_parsing_weights
LAYERS = _layers()
INDEX = {name: i for i, (name, *_) in enumerate(LAYERS)}
# the auxiliary heads: in the checkpoint, never read by the forward pass test.py runs
AUX = tuple((f"{h}.conv.conv", f"{h}.conv.bn", 128, 64, 3, 1) for h in ("conv_out16", "conv_out32")) + \
      tuple((f"{h}.conv_out", None, 64, N_CLASSES, 1, 1) for h in ("conv_out16", "conv_out32"))
_BN = (("gamma", "weight"), ("beta", "bias"), ("mean", "running_mean"), ("var", "running_var"))


def macs_per_frame(H: int = SIZE, W: int = SIZE) -> int:
    """Multiply-accumulates of the convolutions of one H x W frame."""
    h = {s: (H // s) * (W // s) for s in (2, 4, 8, 16, 32)}
    total = 0
    for name, _, cin, cout, k, _ in LAYERS[:INDEX["cp.conv_avg.conv"]]:
        if name == "cp.resnet.conv1":
            pix = h[2]
        elif ".layer" in name:                                   # every convolution of a stage writes the stage's extent
            pix = h[(4, 8, 16, 32)[int(name.split(".layer")[1][0]) - 1]]
        else:
            pix = {"cp.arm32.conv.conv": h[32], "cp.arm16.conv.conv": h[16], "cp.conv_head32.conv": h[16]}.get(name, h[8])
        total += cin * cout * k * k * pix
    return total


# ---- weights ----------------------------------------------------------------------------------------------------------
class BiSeNetWeights:
    """The frozen parameters of ``BiSeNet(19)``: per layer of ``LAYERS`` the bias-free convolution's weight and, where
    it has one, BatchNorm's gamma, beta, running mean and running variance.  Kept in fp32 on the CPU; the device copy
    (convolutions in the kernels' layout, BatchNorm folded) is made once per device (``device_pack``).  ``aux``: the
    tensors of the two auxiliary heads when the source had them; they only pass through ``state_dict``."""

    def __init__(self, layers, aux=None):
        if len(layers) != len(LAYERS):
            raise ValueError(f"BiSeNet weights: expected {len(LAYERS)} layers, got {len(layers)}")
        self.layers = []
        for lay, (name, bn, cin, cout, k, _) in zip(layers, LAYERS):
            fields = ("weight",) + (tuple(f for f, _ in _BN) if bn else ())
            lay = {f: lay[f].detach().float().contiguous().cpu() for f in fields}
            for f in fields:
                want = (cout, cin, k, k) if f == "weight" else (cout,)
                if tuple(lay[f].shape) != want:
                    raise ValueError(f"BiSeNet weights: {name} {f} has shape {tuple(lay[f].shape)}, expected {want}")
            self.layers.append(lay)
        self.aux = {k: v.detach().clone().cpu() for k, v in (aux or {}).items()}
        self._packs = {}

    @classmethod
    def from_state_dict(cls, sd) -> "BiSeNetWeights":
        """``sd``: the keys of 79999_iter.pth (``BiSeNet(19).state_dict()``).  ``conv_out16.*``, ``conv_out32.*`` and
        ``num_batches_tracked`` are accepted and not read; a missing key raises a ValueError naming it."""
        def get(key):
            if key not in sd:
                raise ValueError(f"BiSeNet weights: the state dict misses {key!r}")
            return sd[key]

        layers = []
        for name, bn, *_ in LAYERS:
            lay = {"weight": get(f"{name}.weight")}
            if bn:
                lay.update({f: get(f"{bn}.{key}") for f, key in _BN})
            layers.append(lay)
        aux = {k: v for k, v in sd.items() if k.startswith(("conv_out16.", "conv_out32."))}
        return cls(layers, aux)

    @classmethod
    def load(cls, path) -> "BiSeNetWeights":
        return cls.from_state_dict(torch.load(path, map_location="cpu"))

    @classmethod
    def random(cls, seed: int = 0) -> "BiSeNetWeights":
        """Seeded stand-ins with the scale of trained ones (tests, benches): He-scaled convolutions and non-trivial
        BatchNorm statistics -- gamma and the variance in [0.5, 1.5], beta and the running mean of about 0.2 -- so that
        the fold is exercised and about half of every stage's units are active.  The last convolution of a residual
        block is scaled by a further 1/2 so that the trunk's magnitude stays of order one through the eight blocks, and
        every class row of the classifier sums to zero over its inputs -- they are all positive, and an uncentred row
        turns their common mean into a per-class offset that lets two or three classes win everywhere.  The auxiliary heads are drawn too (after everything else), so ``state_dict()`` is a complete checkpoint."""
        g = torch.Generator().manual_seed(seed)

        def draw(table):
            out = []
            for name, bn, cin, cout, k, _ in table:
                gain = 0.5 if name.endswith(".conv2") and ".layer" in name else 1.0
                lay = dict(weight=torch.randn(cout, cin, k, k, generator=g) * (gain * (2.0 / (cin * k * k)) ** 0.5))
                if name == "conv_out.conv_out":
                    lay["weight"] -= lay["weight"].mean(dim=1, keepdim=True)
                if bn:
                    lay.update(gamma=torch.rand(cout, generator=g) + 0.5, beta=torch.randn(cout, generator=g) * 0.2,
                               mean=torch.randn(cout, generator=g) * 0.2, var=torch.rand(cout, generator=g) + 0.5)
                out.append(lay)
            return out

        layers = draw(LAYERS)
        aux = {}
        for lay, (name, bn, *_) in zip(draw(AUX), AUX):
            aux.update(_entries(name, bn, lay))
        return cls(layers, aux)

    def state_dict(self):
        """The keys of the checkpoint (the reference module's), ``num_batches_tracked`` included."""
        out = {}
        for lay, (name, bn, *_) in zip(self.layers, LAYERS):
            out.update(_entries(name, bn, lay))
        out.update({k: v.clone() for k, v in self.aux.items()})
        return out

    def to(self, device=None, dtype=None):
        """name -> dict of tensors of ``device`` / ``dtype`` for the torch statement."""
        return {name: {f: t.to(device=device, dtype=dtype) for f, t in lay.items()}
                for lay, (name, *_) in zip(self.layers, LAYERS)}

    def folded(self, dtype=torch.float64):
        """Per layer (convolution weight, scale, shift) with BatchNorm (eval) folded in fp64: scale = gamma /
        sqrt(var + eps), shift = beta - mean * scale; (1, 0) for a layer without BatchNorm."""
        out = []
        for lay in self.layers:
            d = {f: t.double() for f, t in lay.items()}
            if "gamma" in d:
                scale = d["gamma"] / torch.sqrt(d["var"] + BN_EPS)
                shift = d["beta"] - d["mean"] * scale
            else:
                scale, shift = torch.ones(d["weight"].shape[0], dtype=torch.float64), \
                    torch.zeros(d["weight"].shape[0], dtype=torch.float64)
            out.append((d["weight"].to(dtype), scale.to(dtype), shift.to(dtype)))
        return out

    def device_pack(self, device):
        """struct instag_parsing_weights for ``device`` (and the tensors it points into): every convolution as
        [K = (cin, ky, kx)][cout], the stem's K = 147 padded with zero rows to 160; the five [B,C]-sized products
        behind the pools as stored, [cout][cin]."""
        from . import _lib
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        pack = self._packs.get(key)
        if pack is not None:
            return pack
        keep, s = [], _lib.ParsingWeights()
        for l, (w, scale, shift) in enumerate(self.folded(torch.float32)):
            wk = w.reshape(w.shape[0], -1)
            if l < INDEX["cp.conv_avg.conv"]:
                wk = wk.t()
            if l == 0:
                wk = torch.cat([wk, torch.zeros(160 - wk.shape[0], wk.shape[1])], dim=0)
            ts = [t.contiguous().to(device) for t in (wk, scale, shift)]
            keep += ts
            s.w[l], s.scale[l], s.shift[l] = [t.data_ptr() for t in ts]
        pack = self._packs[key] = (s, keep)
        return pack


def _entries(name, bn, lay):
    out = {f"{name}.weight": lay["weight"].clone()}
    if bn:
        out.update({f"{bn}.{key}": lay[f].clone() for f, key in _BN})
        out[f"{bn}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return out


# ---- plain-torch statement -------------------------------------------------------------------------------------------
def normalise(frames_u8, dtype=torch.float32):
    """u8 [B,H,W,3] -> [B,3,H,W] of ``dtype``: ``ToTensor`` (u8 / 255) and ``Normalize(MEAN, STD)``, in ``dtype``."""
    x = torch.as_tensor(frames_u8)
    if x.dim() != 4 or x.shape[-1] != 3 or x.dtype != torch.uint8:
        raise ValueError(f"parsing: frames uint8 [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    x = x.permute(0, 3, 1, 2).to(dtype) / 255
    mean = torch.tensor(MEAN, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


def bisenet_torch(weights: BiSeNetWeights, x, taps=None):
    """``BiSeNet(19).forward`` in eval mode up to ``conv_out`` for normalised ``x`` [B,3,H,W] -> logits
    [B,19,H/8,W/8] (model.py:241-247, resnet.py:71-80), BatchNorm not folded.  ``taps``: a list that receives every
    stage's output after its ReLU (the stem, the eight blocks, the seven ConvBNReLU modules)."""
    p = weights.to(x.device, x.dtype)

    def conv(name, t, bn=True):
        _, _, _, _, k, stride = LAYERS[INDEX[name]]
        lay = p[name]
        y = F.conv2d(t, lay["weight"], None, stride=stride, padding=k // 2)
        if bn:
            y = F.batch_norm(y, lay["mean"], lay["var"], lay["gamma"], lay["beta"], training=False, eps=BN_EPS)
        return y

    def tap(t):
        if taps is not None:
            taps.append(t)
        return t

    def cbr(name, t):
        return tap(F.relu(conv(name, t)))

    def pool(t):
        return F.avg_pool2d(t, t.shape[2:])

    def arm(name, t):
        f = cbr(f"{name}.conv.conv", t)
        return f * torch.sigmoid(conv(f"{name}.conv_atten", pool(f)))

    r = "cp.resnet"
    t = F.max_pool2d(cbr(f"{r}.conv1", x), kernel_size=3, stride=2, padding=1)
    feats = []
    for stage in (1, 2, 3, 4):
        for b in (0, 1):
            pre = f"{r}.layer{stage}.{b}"
            res = conv(f"{pre}.conv2", F.relu(conv(f"{pre}.conv1", t)))
            short = conv(f"{pre}.downsample.0", t) if f"{pre}.downsample.0" in INDEX else t
            t = tap(F.relu(short + res))
        feats.append(t)
    _, feat8, feat16, feat32 = feats

    avg = cbr("cp.conv_avg.conv", pool(feat32))
    up32 = F.interpolate(arm("cp.arm32", feat32) + avg, feat16.shape[2:], mode="nearest")
    cp16 = cbr("cp.conv_head32.conv", up32)
    up16 = F.interpolate(arm("cp.arm16", feat16) + cp16, feat8.shape[2:], mode="nearest")
    cp8 = cbr("cp.conv_head16.conv", up16)

    feat = cbr("ffm.convblk.conv", torch.cat([feat8, cp8], dim=1))
    a = torch.sigmoid(conv("ffm.conv2", F.relu(conv("ffm.conv1", pool(feat), bn=False)), bn=False))
    fuse = feat * a + feat
    return conv("conv_out.conv_out", cbr("conv_out.conv.conv", fuse), bn=False)


def upsample_torch(logits8, H: int, W: int):
    """Bilinear, ``align_corners=True``, to [B,19,H,W] (model.py:251)."""
    return F.interpolate(logits8, (H, W), mode="bilinear", align_corners=True)


def first_argmax(full):
    """[B,C,H,W] -> u8 [B,H,W]: the first maximum over C, as numpy's argmax takes it."""
    C_ = full.shape[1]
    idx = torch.arange(C_, device=full.device).view(1, C_, 1, 1)
    hit = full == full.max(dim=1, keepdim=True).values
    return torch.where(hit, idx, C_).min(dim=1).values.to(torch.uint8)


def labels_torch(logits8, H: int, W: int):
    """Logits at 1/8 resolution -> labels u8 [B,H,W]: the bilinear upsample and the first-maximum argmax."""
    return first_argmax(upsample_torch(logits8, H, W))


def resize_index(n_dst: int, n_src: int, device=None):
    """Source index of every destination index of the nearest resize: min((dst * n_src) // n_dst, n_src - 1)."""
    return torch.clamp((torch.arange(n_dst, device=device, dtype=torch.int64) * n_src) // n_dst, max=n_src - 1)


def colour_map_torch(labels, out_h=None, out_w=None):
    """labels u8 [B,H,W] -> u8 [B,out_h,out_w,3]: the colour table, then the nearest resize (module docstring)."""
    labels = torch.as_tensor(labels)
    H, W = labels.shape[1:]
    out_h, out_w = int(out_h or H), int(out_w or W)
    table = torch.from_numpy(COLOURS).to(labels.device)
    src = labels[:, resize_index(out_h, H, labels.device)][:, :, resize_index(out_w, W, labels.device)]
    return table[src.long()]


def _out_size(out_size, H, W):
    if out_size is None:
        return H, W
    out_h, out_w = (int(v) for v in out_size)
    if out_h < 1 or out_w < 1:
        raise ValueError("parsing: out_size (h, w) >= 1")
    return out_h, out_w


def _check_frames(frames_u8):
    x = torch.as_tensor(frames_u8)
    if x.dim() != 4 or x.shape[-1] != 3 or x.dtype != torch.uint8:
        raise ValueError(f"parsing: frames uint8 [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    H, W = int(x.shape[1]), int(x.shape[2])
    if H < MIN_SIDE or W < MIN_SIDE or H % SIDE_MULTIPLE or W % SIDE_MULTIPLE:
        raise ValueError(f"parsing: H and W multiples of {SIDE_MULTIPLE} and at least {MIN_SIDE}, got {H} x {W}")
    return x, H, W


@torch.no_grad()
def parse_torch(weights: BiSeNetWeights, frames_u8, out_size=None, dtype=torch.float32):
    """The chain from u8 frames [B,H,W,3] to the colour map u8 [B,h,w,3] in plain torch, on the frames' device."""
    x, H, W = _check_frames(frames_u8)
    out_h, out_w = _out_size(out_size, H, W)
    logits8 = bisenet_torch(weights, normalise(x, dtype))
    return colour_map_torch(labels_torch(logits8, H, W), out_h, out_w)


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class FaceParser:
    """``parse(frames u8 [B,H,W,3]) -> u8 [B,h,w,3]``, ``labels -> u8 [B,H,W]`` and ``logits -> [B,19,H/8,W/8]`` on
    ``device``, on torch's current stream; inference only.  On the GPU the frames go through csrc/parsing.hip in chunks
    of at most ``max_batch`` with one workspace that is kept (the workspace is the operator's: use one operator per
    stream); on the CPU all three are the torch statement."""

    def __init__(self, weights: BiSeNetWeights, device="cuda", max_batch: int = 8):
        if max_batch < 1:
            raise ValueError("FaceParser: max_batch >= 1")
        self.weights = weights
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self._ws = None
        if self.device.type == "cuda":
            from . import _lib
            self._L = _lib.lib()
            self._struct, self._keep = weights.device_pack(self.device)

    def _workspace(self, batch, H, W):
        key = (batch, H, W)
        if self._ws is None or self._ws[0] != key:
            nbytes = int(self._L.instag_parsing_workspace_bytes(batch, H, W))
            if nbytes == 0:
                raise ValueError(self._L.instag_last_error().decode("utf-8", "replace"))
            self._ws = None
            self._ws = (key, torch.empty(nbytes, dtype=torch.uint8, device=self.device), nbytes)
        return self._ws[1], self._ws[2]

    def _run(self, frames_u8, out_size, want):
        from . import _lib
        x, H, W = _check_frames(frames_u8)
        out_h, out_w = _out_size(out_size, H, W)
        x = x.to(self.device).contiguous()
        B = int(x.shape[0])
        dev = self.device
        logits = torch.empty(B, N_CLASSES, H // 8, W // 8, dtype=torch.float32, device=dev) if "logits" in want else None
        labels = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if "labels" in want else None
        colours = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=dev) if "colours" in want else None
        if B == 0:
            return logits, labels, colours
        ws, nbytes = self._workspace(min(B, self.max_batch), H, W)
        with torch.cuda.device(dev):
            for i in range(0, B, self.max_batch):
                m = min(self.max_batch, B - i)
                rc = self._L.instag_parsing_forward(
                    C.byref(self._struct), _lib.ptr(x[i:i + m]), m, H, W, out_h, out_w,
                    _lib.ptr(None if logits is None else logits[i:i + m]),
                    _lib.ptr(None if labels is None else labels[i:i + m]),
                    _lib.ptr(None if colours is None else colours[i:i + m]), _lib.ptr(ws), nbytes,
                    _lib.current_stream())
                _raise(rc, "parsing_forward")
        return logits, labels, colours

    @torch.no_grad()
    def logits(self, frames_u8):
        if self.device.type != "cuda":
            x, _, _ = _check_frames(frames_u8)
            return bisenet_torch(self.weights, normalise(x.to(self.device)))
        return self._run(frames_u8, None, ("logits",))[0]

    @torch.no_grad()
    def labels(self, frames_u8):
        if self.device.type != "cuda":
            x, H, W = _check_frames(frames_u8)
            return labels_torch(bisenet_torch(self.weights, normalise(x.to(self.device))), H, W)
        return self._run(frames_u8, None, ("labels",))[1]

    @torch.no_grad()
    def parse(self, frames_u8, out_size=None):
        if self.device.type != "cuda":
            return parse_torch(self.weights, torch.as_tensor(frames_u8).to(self.device), out_size)
        return self._run(frames_u8, out_size, ("colours",))[2]


def _raise(code, what):
    if code == 0:
        return
    from . import _lib
    msg = _lib.lib().instag_last_error().decode("utf-8", "replace")
    if code == 1:                                                        # INSTAG_E_ARG
        raise ValueError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg}")


def colour_map(logits8, H: int, W: int, out_size=None, want_labels: bool = False):
    """The final stage alone on the device: logits fp32 [B,19,H/8,W/8] (cuda) -> colours u8 [B,h,w,3] (and labels u8
    [B,H,W]): the bilinear upsample, the first-maximum argmax, the colour table and the nearest resize, one kernel."""
    from . import _lib
    logits8 = logits8.detach().to(dtype=torch.float32).contiguous()
    if logits8.dim() != 4 or tuple(logits8.shape[1:]) != (N_CLASSES, H // 8, W // 8) or H % 8 or W % 8:
        raise ValueError(f"parsing: logits [B,{N_CLASSES},H/8,W/8], got {tuple(logits8.shape)} for {H} x {W}")
    out_h, out_w = _out_size(out_size, H, W)
    B = int(logits8.shape[0])
    colours = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=logits8.device)
    labels = torch.empty(B, H, W, dtype=torch.uint8, device=logits8.device) if want_labels else None
    with torch.cuda.device(logits8.device):
        rc = _lib.lib().instag_parsing_labels(_lib.ptr(logits8), B, H, W, out_h, out_w, _lib.ptr(labels),
                                              _lib.ptr(colours), _lib.current_stream())
    _raise(rc, "parsing_labels")
    return (colours, labels) if want_labels else colours


# ---- a directory --------------------------------------------------------------------------------------------------------
def parse_identity(path, weights: BiSeNetWeights, device="cuda", write: bool = True, batch: int = 8):
    """ori_imgs/<i>.jpg of ``path`` (ascending numeric order) -> parsing u8 [N,H,W,3] on ``device``, what
    ``extract_background`` / ``gt_and_torso`` take, H x W the frames' own size.  As test.py:92-106 does, a frame that is
    not 512 x 512 is resized to it on the host (PIL, bilinear) and its colour map resized back (nearest).  ``write``:
    also parsing/<i>.png."""
    from PIL import Image
    from .prepare import list_frames
    ids = list_frames(path)
    device = torch.device(device)
    parser = FaceParser(weights, device, max_batch=batch)
    out, size = [], None
    if write:
        os.makedirs(os.path.join(path, "parsing"), exist_ok=True)
    for s in range(0, len(ids), batch):
        frames = []
        for i in ids[s:s + batch]:
            img = Image.open(os.path.join(path, "ori_imgs", f"{i}.jpg"))
            if size is None:
                size = img.size                                              # (width, height)
            elif img.size != size:
                raise ValueError(f"{path}: ori_imgs/{i}.jpg is {img.size}, the first frame {size}")
            if img.size != (SIZE, SIZE):
                img = img.resize((SIZE, SIZE), Image.BILINEAR)
            frames.append(np.array(img.convert("RGB")))
        par = parser.parse(torch.from_numpy(np.stack(frames)), out_size=(size[1], size[0]))
        out.append(par)
        if write:
            host = par.cpu().numpy()
            for j, i in enumerate(ids[s:s + batch]):
                Image.fromarray(host[j], "RGB").save(os.path.join(path, "parsing", f"{i}.png"))
    return torch.cat(out, dim=0)
