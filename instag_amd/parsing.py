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

from . import convnet
from .convnet import BN_EPS, first_argmax  # noqa: F401  (first_argmax stays importable from here)

N_CLASSES = 19
SIZE = 512                                           # test.py:94
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# RGB colour of every class
COLOURS = np.array([(255, 255, 255)] + [(0, 0, 255)] * 10 + [(100, 100, 100)] + [(0, 0, 255)] * 2 + [(0, 255, 0)] * 2
                   + [(255, 0, 0), (0, 0, 0), (0, 0, 255)], dtype=np.uint8)


def _block(prefix, cin, cout, stride):
    out = [(f"{prefix}.conv1", f"{prefix}.bn1", False, cin, cout, 3, stride),
           (f"{prefix}.conv2", f"{prefix}.bn2", False, cout, cout, 3, 1)]
    if cin != cout or stride != 1:
        out.append((f"{prefix}.downsample.0", f"{prefix}.downsample.1", False, cin, cout, 1, stride))
    return out


def _layers():
    r = "cp.resnet"
    out = [(f"{r}.conv1", f"{r}.bn1", False, 3, 64, 7, 2)]
    for stage, (cin, cout) in enumerate(((64, 64), (64, 128), (128, 256), (256, 512)), start=1):
        out += _block(f"{r}.layer{stage}.0", cin, cout, 1 if stage == 1 else 2)
        out += _block(f"{r}.layer{stage}.1", cout, cout, 1)
    out += [(f"{m}.conv", f"{m}.bn", False, cin, cout, k, 1) for m, cin, cout, k in (
        ("cp.arm32.conv", 512, 128, 3), ("cp.arm16.conv", 256, 128, 3), ("cp.conv_head32", 128, 128, 3),
        ("cp.conv_head16", 128, 128, 3), ("ffm.convblk", 256, 256, 1), ("conv_out.conv", 256, 256, 3))]
    out += [("conv_out.conv_out", None, False, 256, N_CLASSES, 1, 1),
            # the [B,C]-sized products behind the global average pools
            ("cp.conv_avg.conv", "cp.conv_avg.bn", False, 512, 128, 1, 1),
            ("cp.arm32.conv_atten", "cp.arm32.bn_atten", False, 128, 128, 1, 1),
            ("cp.arm16.conv_atten", "cp.arm16.bn_atten", False, 128, 128, 1, 1),
            ("ffm.conv1", None, False, 256, 64, 1, 1),
            ("ffm.conv2", None, False, 64, 256, 1, 1)]
    return tuple(out)


# (convolution, its BatchNorm or None, has a bias: never, cin, cout, kernel, stride) in the order of struct
# instag_parsing_weights
LAYERS = _layers()
INDEX = {name: i for i, (name, *_) in enumerate(LAYERS)}
# the auxiliary heads: in the checkpoint, never read by the forward pass test.py runs
AUX = tuple((f"{h}.conv.conv", f"{h}.conv.bn", False, 128, 64, 3, 1) for h in ("conv_out16", "conv_out32")) + \
      tuple((f"{h}.conv_out", None, False, 64, N_CLASSES, 1, 1) for h in ("conv_out16", "conv_out32"))


def macs_per_frame(H: int = SIZE, W: int = SIZE) -> int:
    """Multiply-accumulates of the convolutions of one H x W frame."""
    h = {s: (H // s) * (W // s) for s in (2, 4, 8, 16, 32)}
    total = 0
    for name, _, _, cin, cout, k, _ in LAYERS[:INDEX["cp.conv_avg.conv"]]:
        if name == "cp.resnet.conv1":
            pix = h[2]
        elif ".layer" in name:                                   # every convolution of a stage writes the stage's extent
            pix = h[(4, 8, 16, 32)[int(name.split(".layer")[1][0]) - 1]]
        else:
            pix = {"cp.arm32.conv.conv": h[32], "cp.arm16.conv.conv": h[16], "cp.conv_head32.conv": h[16]}.get(name, h[8])
        total += cin * cout * k * k * pix
    return total


# ---- weights ----------------------------------------------------------------------------------------------------------
class BiSeNetWeights(convnet.ConvWeights):
    """The frozen parameters of ``BiSeNet(19)``: per layer of ``LAYERS`` the bias-free convolution's weight and, where
    it has one, BatchNorm's gamma, beta, running mean and running variance (convnet.ConvWeights).  On the device the
    stem's K = 147 is padded with zero rows to 160 and the five [B,C]-sized products behind the pools stay as stored,
    [cout][cin].  ``aux``: the tensors of the two auxiliary heads when the source had them; they only pass through
    ``state_dict``."""

    TABLE, LABEL, STRUCT, STEM_K = LAYERS, "BiSeNet weights", "ParsingWeights", 160
    COUT_MAJOR = range(INDEX["cp.conv_avg.conv"], len(LAYERS))

    def __init__(self, layers, aux=None):
        super().__init__(layers)
        self.aux = {k: v.detach().clone().cpu() for k, v in (aux or {}).items()}

    @classmethod
    def _extras(cls, sd):
        # (from_state_dict: ``conv_out16.*`` and ``conv_out32.*`` of 79999_iter.pth are accepted and not read)
        return dict(aux={k: v for k, v in sd.items() if k.startswith(("conv_out16.", "conv_out32."))})

    @classmethod
    def random(cls, seed: int = 0) -> "BiSeNetWeights":
        """Seeded stand-ins with the scale of trained ones (tests, benches; convnet.draw_layer), so that the fold is
        exercised and about half of every stage's units are active.  The last convolution of a residual block is
        scaled by a further 1/2 so that the trunk's magnitude stays of order one through the eight blocks, and every
        class row of the classifier sums to zero over its inputs -- they are all positive, and an uncentred row turns
        their common mean into a per-class offset that lets two or three classes win everywhere.  The auxiliary heads
        are drawn too (after everything else), so ``state_dict()`` is a complete checkpoint."""
        g = torch.Generator().manual_seed(seed)

        def draw(row):
            return convnet.draw_layer(g, row, gain=0.5 if row[0].endswith(".conv2") and ".layer" in row[0] else 1.0,
                                      centre=row[0] == "conv_out.conv_out")

        layers, aux = [draw(row) for row in LAYERS], {}
        for row in AUX:
            aux.update(convnet.entries(row, draw(row)))
        return cls(layers, aux)

    def state_dict(self):
        """The keys of the checkpoint (the reference module's), ``num_batches_tracked`` included."""
        out = super().state_dict()
        out.update({k: v.clone() for k, v in self.aux.items()})
        return out


# ---- plain-torch statement -------------------------------------------------------------------------------------------
def normalise(frames_u8, dtype=torch.float32):
    """u8 [B,H,W,3] -> [B,3,H,W] of ``dtype``: ``ToTensor`` (u8 / 255) and ``Normalize(MEAN, STD)``, in ``dtype``."""
    return convnet.normalise("parsing", frames_u8, MEAN, STD, True, dtype)


def bisenet_torch(weights: BiSeNetWeights, x, taps=None):
    """``BiSeNet(19).forward`` in eval mode up to ``conv_out`` for normalised ``x`` [B,3,H,W] -> logits
    [B,19,H/8,W/8] (model.py:241-247, resnet.py:71-80), BatchNorm not folded.  ``taps``: a list that receives every
    stage's output after its ReLU (the stem, the eight blocks, the seven ConvBNReLU modules)."""
    p = weights.to(x.device, x.dtype)

    def conv(name, t, bn=True):
        k, stride = LAYERS[INDEX[name]][5:]
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


@torch.no_grad()
def parse_torch(weights: BiSeNetWeights, frames_u8, out_size=None, dtype=torch.float32):
    """The chain from u8 frames [B,H,W,3] to the colour map u8 [B,h,w,3] in plain torch, on the frames' device."""
    x, H, W = convnet.check_frames("parsing", frames_u8)
    out_h, out_w = _out_size(out_size, H, W)
    logits8 = bisenet_torch(weights, normalise(x, dtype))
    return colour_map_torch(labels_torch(logits8, H, W), out_h, out_w)


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class FaceParser(convnet.FrameOperator):
    """``parse(frames u8 [B,H,W,3]) -> u8 [B,h,w,3]``, ``labels -> u8 [B,H,W]`` and ``logits -> [B,19,H/8,W/8]`` on
    ``device`` through csrc/parsing.hip, in chunks of at most ``max_batch`` (convnet.FrameOperator)."""

    NAME = "parsing"
    net_torch, normalise_torch, labels_torch = staticmethod(bisenet_torch), staticmethod(normalise), \
        staticmethod(labels_torch)

    def __init__(self, weights: BiSeNetWeights, device="cuda", max_batch: int = 8):
        super().__init__(weights, device, int(max_batch))

    def _workspace_bytes(self, batch, H, W):
        return self._L.instag_parsing_workspace_bytes(batch, H, W)

    def _run(self, frames_u8, want, out_size=None):
        from . import _lib
        x, H, W = convnet.check_frames(self.NAME, frames_u8)
        out_h, out_w = _out_size(out_size, H, W)
        x = x.to(self.device).contiguous()
        B = int(x.shape[0])
        outs = self._empty(want, logits=(B, N_CLASSES, H // 8, W // 8), labels=(B, H, W), colours=(B, out_h, out_w, 3))
        self._chunks(x, H, W, lambda c, m, ws, nbytes: self._L.instag_parsing_forward(
            C.byref(self._struct), _lib.ptr(x[c]), m, H, W, out_h, out_w,
            *(_lib.ptr(None if t is None else t[c]) for t in outs), ws, nbytes, _lib.current_stream()),
            "parsing_forward")
        return outs

    @torch.no_grad()
    def parse(self, frames_u8, out_size=None):
        if self.device.type != "cuda":
            return parse_torch(self.weights, torch.as_tensor(frames_u8).to(self.device), out_size)
        return self._run(frames_u8, ("colours",), out_size)[2]


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
    _lib.check_arg(rc, "parsing_labels")
    return (colours, labels) if want_labels else colours


# ---- a directory --------------------------------------------------------------------------------------------------------
def parse_identity(path, weights: BiSeNetWeights, device="cuda", write: bool = True, batch: int = 8, decoder=None):
    """ori_imgs/<i>.jpg of ``path`` (ascending numeric order) -> parsing u8 [N,H,W,3] on ``device``, what
    ``extract_background`` / ``gt_and_torso`` take, H x W the frames' own size.  As test.py:92-106 does, a frame that is
    not 512 x 512 is resized to it on the host (PIL, bilinear) and its colour map resized back (nearest).  ``write``:
    also parsing/<i>.png."""
    from PIL import Image
    parser = FaceParser(weights, torch.device(device), max_batch=batch)
    out = []
    if write:
        os.makedirs(os.path.join(path, "parsing"), exist_ok=True)
    for ids, frames, size in convnet.frame_batches(path, batch, resize=SIZE, decoder=decoder):
        par = parser.parse(frames, out_size=(size[1], size[0]))
        out.append(par)
        if write:
            for i, host in zip(ids, par.cpu().numpy()):
                Image.fromarray(host, "RGB").save(os.path.join(path, "parsing", f"{i}.png"))
    return torch.cat(out, dim=0)
