"""What the pretrained convolution networks share on the host: parsing.py (BiSeNet), teeth.py (ResNet-50 FPN) and the
weights of ave_encoder.py.

``ConvWeights`` holds the frozen parameters of one network described by a layer table -- rows ``(name, bn, bias, cin,
cout, kernel, stride)``: the convolution's module name, its BatchNorm's name or None, whether it has a bias, and its
shape (``cout=None``: ``self.classes``, which the subclass reads from the checkpoint in ``_prepare``).  A subclass
supplies the table, its ``random`` rule and whatever else is its own; the shape validation, the checkpoint keys, the
BatchNorm fold and the device copy are here.

``FrameOperator`` is the base of the operators that take uint8 frames [B,H,W,3] (the parser, the teeth segmenter, the
landmark net and the face detector): the frame check, the outputs and the CPU fall-back.  The weights' device copy,
the kept workspace and the chunk loop are device_op.DeviceOperator's, which the audio operators share.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .device_op import DeviceOperator

BN_EPS = 1e-5
BN = (("gamma", "weight"), ("beta", "bias"), ("mean", "running_mean"), ("var", "running_var"))
MIN_SIDE, SIDE_MULTIPLE = 64, 32


def keys(row):
    """(field, checkpoint key) of every tensor of a table row, in the order a layer's dict holds them."""
    name, bn, bias = row[:3]
    return (("weight", f"{name}.weight"),) + ((("bias", f"{name}.bias"),) if bias else ()) + \
        (tuple((f, f"{bn}.{key}") for f, key in BN) if bn else ())


def entries(row, lay):
    """The checkpoint's entries of one layer: clones of its tensors and BatchNorm's ``num_batches_tracked``."""
    out = {key: lay[f].clone() for f, key in keys(row)}
    if row[1]:
        out[f"{row[1]}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return out


def draw_layer(g, row, gain=1.0, centre=False, classes=None):
    """One layer of seeded stand-ins from generator ``g``: a He-scaled convolution (times ``gain``; ``centre``: every
    output row summing to zero over its inputs), a bias of about 0.1 and BatchNorm statistics -- gamma and the variance
    in [0.5, 1.5], beta and the running mean of about 0.2 -- where the row has them, drawn in this order."""
    _, bn, bias, cin, cout, k, _ = row
    cout = classes if cout is None else cout
    lay = dict(weight=torch.randn(cout, cin, k, k, generator=g) * (gain * (2.0 / (cin * k * k)) ** 0.5))
    if centre:
        lay["weight"] -= lay["weight"].mean(dim=1, keepdim=True)
    if bias:
        lay["bias"] = torch.randn(cout, generator=g) * 0.1
    if bn:
        lay.update(gamma=torch.rand(cout, generator=g) + 0.5, beta=torch.randn(cout, generator=g) * 0.2,
                   mean=torch.randn(cout, generator=g) * 0.2, var=torch.rand(cout, generator=g) + 0.5)
    return lay


# ---- weights ----------------------------------------------------------------------------------------------------------
class ConvWeights:
    """Per row of ``TABLE`` a dict of the convolution's weight, its bias and BatchNorm's gamma, beta, running mean and
    running variance, as the row has them.  Kept in fp32 on the CPU; the device copy (convolutions in the kernels'
    layout, BatchNorm folded) is made once per device (``device_pack``)."""

    TABLE = ()              # the layer table, in the order of the C struct
    LABEL = ""              # what the error messages call the weights
    STRUCT = ""             # the ctypes struct of _lib
    STEM_K = None           # the first layer's K is padded with zero rows to this
    COUT_MAJOR = ()          # layers the kernels read as stored, [cout][cin ky kx], not as [K][cout]
    PRE = ()                 # layers whose BatchNorm stands in FRONT of the convolution: its tensors have cin entries

    def __init__(self, layers):
        if len(layers) != len(self.TABLE):
            raise ValueError(f"{self.LABEL}: expected {len(self.TABLE)} layers, got {len(layers)}")
        self._prepare(layers)
        self.layers = []
        for l, (lay, row) in enumerate(zip(layers, self.TABLE)):
            _, _, _, cin, cout, k, _ = row
            cout = self.classes if cout is None else cout
            lay = {f: lay[f].detach().float().contiguous().cpu() for f, _ in keys(row)}
            for f, t in lay.items():
                want = (cout, cin, k, k) if f == "weight" else (cin if l in self.PRE and f != "bias" else cout,)
                if tuple(t.shape) != want:
                    raise ValueError(f"{self.LABEL}: {self._layer_name(l)} {f} has shape {tuple(t.shape)}, expected {want}")
            self.layers.append(lay)
        self._packs = {}

    def _prepare(self, layers):
        """Called with the right number of layers before they are validated."""

    @classmethod
    def _layer_name(cls, l):
        """What an error message calls layer ``l``."""
        return cls.TABLE[l][0]

    @classmethod
    def _read(cls, sd, missing, **extras):
        """``cls`` from the keys of ``sd``; ``missing(layer index, key)`` makes the exception for an absent key."""
        def get(l, key):
            if key not in sd:
                raise missing(l, key)
            return sd[key]

        return cls([{f: get(l, key) for f, key in keys(row)} for l, row in enumerate(cls.TABLE)], **extras)

    @classmethod
    def from_state_dict(cls, sd):
        """``sd``: the reference modules' keys, or an mmcv checkpoint ``{"meta": ..., "state_dict": ...}`` itself.
        ``num_batches_tracked`` is accepted and not read; a missing key raises a ValueError naming it."""
        if "state_dict" in sd and not torch.is_tensor(sd["state_dict"]):
            sd = sd["state_dict"]
        return cls._read(sd, lambda l, key: ValueError(f"{cls.LABEL}: the state dict misses {key!r}"),
                         **cls._extras(sd))

    @classmethod
    def _extras(cls, sd):
        """Further constructor arguments a subclass takes from the state dict."""
        return {}

    @classmethod
    def load(cls, path):
        return cls.from_state_dict(torch.load(path, map_location="cpu"))

    def state_dict(self):
        """The keys of the checkpoint (the reference modules'), ``num_batches_tracked`` included."""
        out = {}
        for lay, row in zip(self.layers, self.TABLE):
            out.update(entries(row, lay))
        return out

    def to(self, device=None, dtype=None):
        """name -> dict of tensors of ``device`` / ``dtype`` for the torch statement."""
        return {row[0]: {f: t.to(device=device, dtype=dtype) for f, t in lay.items()}
                for lay, row in zip(self.layers, self.TABLE)}

    def folded(self, dtype=torch.float64):
        """Per layer (bias-free convolution weight, scale, shift) with BatchNorm (eval) and the bias folded in fp64:
        scale = gamma / sqrt(var + eps) (1 without BatchNorm), shift = (bias - mean) * scale + beta, an absent term
        being 0."""
        out = []
        for lay in self.layers:
            d = {f: t.double() for f, t in lay.items()}
            zero = torch.zeros(d["weight"].shape[0], dtype=torch.float64)
            scale = d["gamma"] / torch.sqrt(d["var"] + BN_EPS) if "gamma" in d else torch.ones_like(zero)
            shift = (d.get("bias", zero) - d.get("mean", zero)) * scale + d.get("beta", zero)
            out.append((d["weight"].to(dtype), scale.to(dtype), shift.to(dtype)))
        return out

    def device_pack(self, device):
        """The C struct for ``device`` (and the tensors it points into): every convolution as [K = (cin, ky, kx)][cout]
        but those of ``COUT_MAJOR``, the first layer's K padded with zero rows to ``STEM_K``."""
        from . import _lib
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        pack = self._packs.get(key)
        if pack is not None:
            return pack
        keep, s = [], getattr(_lib, self.STRUCT)()
        for l, (w, scale, shift) in enumerate(self.folded(torch.float32)):
            wk = w.reshape(w.shape[0], -1)
            if l not in self.COUT_MAJOR:
                wk = wk.t()
            if l == 0 and self.STEM_K:
                wk = torch.cat([wk, torch.zeros(self.STEM_K - wk.shape[0], wk.shape[1])], dim=0)
            ts = [t.contiguous().to(device) for t in (wk, scale, shift)]
            keep += ts
            s.w[l], s.scale[l], s.shift[l] = [t.data_ptr() for t in ts]
        pack = self._packs[key] = (s, keep)
        return pack


# ---- plain-torch pieces ----------------------------------------------------------------------------------------------
def check_frames(who, frames_u8, sides: bool = True):
    """-> (tensor, H, W) of u8 frames [B,H,W,3]; ``sides``: H and W multiples of 32 and at least 64."""
    x = torch.as_tensor(frames_u8)
    if x.dim() != 4 or x.shape[-1] != 3 or x.dtype != torch.uint8:
        raise ValueError(f"{who}: frames uint8 [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    H, W = int(x.shape[1]), int(x.shape[2])
    if sides and (H < MIN_SIDE or W < MIN_SIDE or H % SIDE_MULTIPLE or W % SIDE_MULTIPLE):
        raise ValueError(f"{who}: H and W multiples of {SIDE_MULTIPLE} and at least {MIN_SIDE}, got {H} x {W}")
    return x, H, W


def normalise(who, frames_u8, mean, std, divide_by_255, dtype=torch.float32):
    """u8 [B,H,W,3] -> [B,3,H,W] of ``dtype``: (u8 [/ 255] - mean) / std per channel, in ``dtype``."""
    x = check_frames(who, frames_u8, sides=False)[0].permute(0, 3, 1, 2).to(dtype)
    if divide_by_255:
        x = x / 255
    mean = torch.tensor(mean, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(std, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


def first_argmax(full):
    """[B,C,H,W] -> u8 [B,H,W]: the first maximum over C, as numpy's argmax takes it."""
    C_ = full.shape[1]
    idx = torch.arange(C_, device=full.device).view(1, C_, 1, 1)
    hit = full == full.max(dim=1, keepdim=True).values
    return torch.where(hit, idx, C_).min(dim=1).values.to(torch.uint8)


# ---- HIP operator -----------------------------------------------------------------------------------------------------
class FrameOperator(DeviceOperator):
    """A network over u8 frames [B,H,W,3] on ``device``, on torch's current stream; inference only.  On the GPU the
    frames go through the network's C entry point in chunks of at most ``max_batch`` with the one kept workspace of
    device_op.DeviceOperator; on the CPU every output is the torch statement.
    A subclass sets ``NAME`` and the three functions of its torch statement, and supplies ``_workspace_bytes`` and
    ``_run(frames, want, ...)``, which allocates the outputs named in ``want`` and hands ``_chunks`` its launch."""

    NAME = ""
    net_torch = normalise_torch = labels_torch = None       # staticmethods of the subclass

    def __init__(self, weights, device, max_batch):
        self.max_batch = self._at_least_one(max_batch, got=False)
        super().__init__(weights, device)

    def _empty(self, want, **shapes):
        """One tensor per keyword, in order (``logits`` fp32, the others u8), None for those not in ``want``."""
        return tuple(torch.empty(*shape, dtype=torch.float32 if name == "logits" else torch.uint8, device=self.device)
                     if name in want else None for name, shape in shapes.items())

    def _chunks(self, x, H, W, launch, what):
        """``launch(chunk slice, its length, workspace pointer, workspace bytes) -> return code`` for every chunk."""
        from . import _lib
        B = int(x.shape[0])
        if B:
            self._each_chunk(B, _lib.workspace_bytes(self._workspace_bytes(min(B, self.max_batch), H, W)), launch, what)

    def _logits_torch(self, frames_u8):
        x, H, W = check_frames(self.NAME, frames_u8)
        return self.net_torch(self.weights, self.normalise_torch(x.to(self.device))), H, W

    @torch.no_grad()
    def logits(self, frames_u8):
        if self.device.type != "cuda":
            return self._logits_torch(frames_u8)[0]
        return self._run(frames_u8, ("logits",))[0]

    @torch.no_grad()
    def labels(self, frames_u8):
        if self.device.type != "cuda":
            return self.labels_torch(*self._logits_torch(frames_u8))
        return self._run(frames_u8, ("labels",))[1]


# ---- a directory --------------------------------------------------------------------------------------------------------
def _decoded_on_device(paths, size, resize, decoder):
    """The files of one batch through ``decoder`` (a ``jpeg_decode.JpegDecoder``) -> (frames on its device, (width,
    height)), or None where the batch is PIL's: a file the decoder's parser refuses, files of different sizes or not of
    ``size``, or a size that ``resize`` changes."""
    files = []
    for p in paths:
        with open(p, "rb") as f:
            files.append(f.read())
    want = (resize, resize) if resize else size
    if size is not None and want != size:
        return None
    return decoder.decode_uniform(files, want)


def frame_batches(path, batch: int, resize=None, decoder=None):
    """ori_imgs/<i>.jpg of ``path`` in ascending numeric order, ``batch`` at a time -> (ids, u8 frames [b,H,W,3], the
    files' (width, height)).  Every file has the first one's size; ``resize``: frames of another size are resized to
    (resize, resize) on the host (PIL, bilinear).  ``decoder``: a ``jpeg_decode.JpegDecoder``; a batch is then decoded
    on its device from the files' bytes and comes back there, with the same bytes as PIL's; a batch with a file its
    parser refuses (progressive, grayscale, restart markers, ...), with files of mixed sizes or one that ``resize``
    changes is PIL's as before."""
    from PIL import Image
    from .prepare import list_frames
    ids, size = list_frames(path), None
    for s in range(0, len(ids), batch):
        if decoder is not None:
            got = _decoded_on_device([os.path.join(path, "ori_imgs", f"{i}.jpg") for i in ids[s:s + batch]], size, resize,
                                     decoder)
            if got is not None:
                size = got[1]
                yield ids[s:s + batch], got[0], size
                continue
        frames = []
        for i in ids[s:s + batch]:
            img = Image.open(os.path.join(path, "ori_imgs", f"{i}.jpg"))
            if size is None:
                size = img.size                                              # (width, height)
            elif img.size != size:
                raise ValueError(f"{path}: ori_imgs/{i}.jpg is {img.size}, the first frame {size}")
            if resize and img.size != (resize, resize):
                img = img.resize((resize, resize), Image.BILINEAR)
            frames.append(np.array(img.convert("RGB")))
        yield ids[s:s + batch], torch.from_numpy(np.stack(frames)), size
