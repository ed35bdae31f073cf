"""The training set of one identity, resident in device memory as 8-bit planes (csrc/frames.hip).

The reference keeps every camera's decoded files on the host as numpy arrays and uploads a frame's image, background
and masks inside the iteration that uses them (dataset_readers.py:222-249, train_face.py:324-327, 393: blocking
``.cuda()`` copies).  The data is 8-bit at the source: an RGB image, a torso RGBA composited over one shared background,
a parsing image that encodes three masks in colours, a teeth mask.  Kept that way a frame is 7 bytes per pixel (gt RGB,
background RGB, one mask byte) against the 27 of the fp32 form a step reads, so a whole identity fits in HBM and feeding
a captured step is one small launch that expands frame ``i`` into the step's static frame:

    store = FrameStore("cuda")
    store.append(gt, torso, bc, parsing, teeth, cameras, au_exp, lips_rect, audio_index)   # instag_frame_ingest
    store.set_audio(features)                                                             # [T, C, L]
    trainer.step(store.ref(i))                                  # Frame.copy_from -> instag_frame_unpack

``ingest_torch`` and ``unpack_torch`` state in plain torch what the two kernels produce; they serve a store on a CPU
device and are the reference of the GPU tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from .train import Frame

REC_DWORDS = 48                      # instag_frame_record_dwords(): 16 + 16 + 3 + 6 + 4 used
# (name in the packed Frame, first dword of the record, shape, dtype)
RECORD = (("world_view_transform", 0, (4, 4), torch.float32), ("full_proj_transform", 16, (4, 4), torch.float32),
          ("camera_center", 32, (3,), torch.float32), ("au_exp", 35, (6,), torch.float32),
          ("lips_rect", 41, (4,), torch.int32))
_ARG_OF = dict(original_image="off_image", background="off_background", face_mask="off_face", hair_mask="off_hair",
               mouth_mask="off_mouth", world_view_transform="off_world_view", full_proj_transform="off_full_proj",
               camera_center="off_camera_center", au_exp="off_au_exp", lips_rect="off_lips_rect", auds="off_auds",
               normal="off_normal", depth="off_depth")


def _pad256(n: int) -> int:
    return (n + 255) // 256 * 256


def store_stride(H: int, W: int) -> int:
    """Bytes of one frame in the store: rgb, bg [H*W*3] and mask [H*W], each padded to 256 bytes."""
    return 2 * _pad256(H * W * 3) + _pad256(H * W)


def ingest_torch(gt, torso, bc, parsing, teeth):
    """What instag_frame_ingest writes, in plain torch.  gt [F,H,W,3], torso [F,H,W,4], bc [H,W,3], parsing [F,H,W,3],
    teeth [F,H,W] uint8 -> rgb, bg [F,H,W,3] uint8, mask [F,H,W] uint8 (bit 0 face, 1 hair, 2 mouth), counts [F,3] int32.

    bg is dataset_readers.py:232-235 as numpy evaluates it (fp64, one rounding per operation, truncating cast);
    the masks are :247-249, where ``*`` binds tighter than ``^``: face = (blue & no red & no green) ^ teeth."""
    t = torso[..., :3].double()
    a = torso[..., 3:].double()
    bg = (t * a / 255.0 + bc.double() * (1 - a / 255.0)).to(torch.uint8)
    R, G, B = parsing[..., 0], parsing[..., 1], parsing[..., 2]
    tm = teeth != 0
    face = ((B > 254) & (R == 0) & (G == 0)) ^ tm
    hair = (R < 1) & (G < 1) & (B < 1)
    mouth = ((R == 100) & (G == 100) & (B == 100)) | tm
    mask = face.to(torch.uint8) | (hair.to(torch.uint8) << 1) | (mouth.to(torch.uint8) << 2)
    counts = torch.stack([m.flatten(1).sum(1) for m in (face, hair, mouth)], dim=1).to(torch.int32)
    return gt.clone(), bg, mask, counts


def audio_window(features, index: int):
    """get_audio_features(features, 2, index) (utils/audio_utils.py:38-73) for a table [T,C,L]: rows index - 4 ..
    index + 3, zero rows where the window leaves the table -> [8,C,L]."""
    T = features.shape[0]
    left, right = index - 4, index + 4
    pad_left, pad_right = max(0, -left), max(0, right - T)
    rows = features[max(left, 0):min(right, T)]
    zeros = features.new_zeros
    return torch.cat([zeros((pad_left,) + tuple(features.shape[1:])), rows,
                      zeros((pad_right,) + tuple(features.shape[1:]))], dim=0)


class StoredFrame:
    """Handle of frame ``index`` of a FrameStore.  ``Frame.copy_from(handle)`` expands it straight into the packed
    frame (one launch, nothing materialised); every other use -- an eager step reading the tensors, ``clone_static``
    in front of a capture -- goes through ``store.frame(index)``, made on first touch and kept."""

    def __init__(self, store: "FrameStore", index: int, background: bool = True, priors: Optional[bool] = None):
        self.store, self.index = store, int(index)
        self._want = (background, priors)
        self.image_height, self.image_width = store.H, store.W
        self.FoVx, self.FoVy = store.FoVx, store.FoVy
        self._frame = None

    def materialise(self) -> Frame:
        if self._frame is None:
            self._frame = self.store.frame(self.index, *self._want)
        return self._frame

    def __getattr__(self, name):
        if name.startswith("__") or name in ("store", "index", "_frame", "_want"):
            raise AttributeError(name)
        return getattr(self.materialise(), name)


class _Chunk:
    __slots__ = ("start", "F", "buf", "records", "normal", "depth")


class FrameStore:
    def __init__(self, device):
        self.device = torch.device(device)
        self.H = self.W = None
        self.FoVx = self.FoVy = None
        self.chunks = []
        self.audio = None
        self.audio_index = []
        self._counts = []
        self.has_priors = None
        self._args = {}

    # ---- building -----------------------------------------------------------------------------------------------
    def append(self, gt, torso, bc, parsing, teeth, cameras: Sequence, au_exp, lips_rect, audio_index,
               normal=None, depth=None):
        """A batch of F frames as decoded: uint8 arrays gt [F,H,W,3], torso [F,H,W,4], bc [H,W,3], parsing [F,H,W,3],
        teeth [F,H,W] (bool or uint8); ``cameras`` F scene_synth.Camera; au_exp [F,6]; lips_rect [F,4]; audio_index [F]
        (row of the audio table the frame's window is centred on); optional priors normal [F,3,H,W], depth [F,H,W]."""
        dev = self.device
        u8 = lambda x: torch.as_tensor(x).to(torch.uint8).contiguous()
        gt, torso, bc, parsing, teeth = u8(gt), u8(torso), u8(bc), u8(parsing), u8(teeth)
        F, H, W = int(gt.shape[0]), int(gt.shape[1]), int(gt.shape[2])
        if F < 1 or H < 1 or W < 1:
            raise ValueError("append: empty batch")
        if tuple(gt.shape) != (F, H, W, 3) or tuple(torso.shape) != (F, H, W, 4) or tuple(bc.shape) != (H, W, 3) \
                or tuple(parsing.shape) != (F, H, W, 3) or tuple(teeth.shape) != (F, H, W):
            raise ValueError("append: gt [F,H,W,3], torso [F,H,W,4], bc [H,W,3], parsing [F,H,W,3], teeth [F,H,W]")
        if len(cameras) != F or len(audio_index) != F:
            raise ValueError("append: one camera and one audio index per frame")
        cam = cameras[0]
        if (cam.image_height, cam.image_width) != (H, W):
            raise ValueError("append: the cameras are not of the images' size")
        if self.H is None:
            self.H, self.W, self.FoVx, self.FoVy = H, W, float(cam.FoVx), float(cam.FoVy)
            self.has_priors = normal is not None
        if (H, W) != (self.H, self.W) or any(abs(c.FoVx - self.FoVx) > 1e-12 or abs(c.FoVy - self.FoVy) > 1e-12
                                              for c in cameras):
            raise ValueError("append: one image size and one field of view per store")
        if (normal is not None) != self.has_priors or (normal is None) != (depth is None):
            raise ValueError("append: priors for every frame of a store (normal and depth together) or for none")

        rec = torch.zeros(F, REC_DWORDS, dtype=torch.float32)
        rec[:, 0:16] = torch.stack([c.world_view_transform.reshape(16) for c in cameras]).float().cpu()
        rec[:, 16:32] = torch.stack([c.full_proj_transform.reshape(16) for c in cameras]).float().cpu()
        rec[:, 32:35] = torch.stack([c.camera_center.reshape(3) for c in cameras]).float().cpu()
        rec[:, 35:41] = torch.as_tensor(au_exp).float().reshape(F, 6).cpu()
        rec.view(torch.int32)[:, 41:45] = torch.as_tensor(lips_rect).to(torch.int32).reshape(F, 4).cpu()

        ch = _Chunk()
        ch.start, ch.F = len(self), F
        stride = store_stride(H, W)
        ch.buf = torch.zeros(F * stride, dtype=torch.uint8, device=dev)
        ch.records = rec.to(dev)
        ch.normal = ch.depth = None
        if normal is not None:
            ch.normal = torch.as_tensor(normal).float().reshape(F, 3, H, W).contiguous().to(dev)
            ch.depth = torch.as_tensor(depth).float().reshape(F, H, W).contiguous().to(dev)
        if dev.type == "cuda":
            lib = _lib.lib()
            assert lib.instag_frame_store_stride(H, W) == stride and lib.instag_frame_record_dwords() == REC_DWORDS
            src = [x.to(dev) for x in (gt, torso, bc, parsing, teeth)]
            counts = torch.empty(F, 3, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.instag_frame_ingest(*[_lib.ptr(x) for x in src], F, H, W, _lib.ptr(ch.buf),
                                                   _lib.ptr(counts), _lib.current_stream()), "frame_ingest")
            counts = counts.cpu()                 # (waits for the kernel: the uploads may be freed)
        else:
            rgb, bg, mask, counts = ingest_torch(gt, torso, bc, parsing, teeth)
            v_rgb, v_bg, v_mask = self._planes(ch)
            v_rgb.copy_(rgb), v_bg.copy_(bg), v_mask.copy_(mask)
        self.chunks.append(ch)
        self._counts.append(counts)
        self.audio_index.extend(int(i) for i in audio_index)
        return self

    def set_audio(self, features):
        """The audio feature table [T,C,L] (29,16 deepspeech / esperanto, 1,512 ave) every frame's window is cut from."""
        f = torch.as_tensor(features).float()
        if f.dim() != 3 or f.shape[0] < 1:
            raise ValueError("set_audio: features [T,C,L]")
        self.audio = f.contiguous().to(self.device)
        self._args.clear()
        return self

    # ---- reading ------------------------------------------------------------------------------------------------
    def __len__(self):
        return sum(c.F for c in self.chunks)

    @property
    def counts(self) -> torch.Tensor:
        """[N,3] int32 on the host: pixels of the face, hair and mouth mask of every frame."""
        return torch.cat(self._counts) if self._counts else torch.zeros(0, 3, dtype=torch.int32)

    @property
    def nbytes(self) -> int:
        n = 0 if self.audio is None else self.audio.numel() * 4
        for c in self.chunks:
            n += c.buf.numel() + c.records.numel() * 4
            if c.normal is not None:
                n += (c.normal.numel() + c.depth.numel()) * 4
        return n

    def _planes(self, ch):
        """Strided views of a chunk's buffer: rgb, bg [F,H,W,3], mask [F,H,W]."""
        H, W = self.H, self.W
        stride, P3 = store_stride(H, W), _pad256(H * W * 3)
        rgb = torch.as_strided(ch.buf, (ch.F, H, W, 3), (stride, W * 3, 3, 1), 0)
        bg = torch.as_strided(ch.buf, (ch.F, H, W, 3), (stride, W * 3, 3, 1), P3)
        mask = torch.as_strided(ch.buf, (ch.F, H, W), (stride, W, 1), 2 * P3)
        return rgb, bg, mask

    def planes(self):
        """rgb, bg [N,H,W,3], mask [N,H,W] uint8 of the whole store (copies)."""
        parts = [self._planes(c) for c in self.chunks]
        return tuple(torch.cat([p[k] for p in parts]) for k in range(3))

    def _locate(self, i: int):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(f"frame {i} outside [0, {len(self)})")
        for k, c in enumerate(self.chunks):
            if i < c.start + c.F:
                return k, c, i - c.start
        raise AssertionError

    def _audio_index(self, i: int) -> int:
        if self.audio is None:
            raise RuntimeError("FrameStore: set_audio() first")
        a = self.audio_index[i]
        if not 0 <= a <= self.audio.shape[0]:          # (== T: the last window the reference accepts, half zeros)
            raise IndexError(f"frame {i}: audio index {a} outside the table [0, {self.audio.shape[0]}]")
        return a

    def layout(self, background: bool = False, priors: bool = False):
        """The packed-Frame layout (train.py Frame.packed: name, shape, dtype in buffer order) this store fills."""
        H, W = self.H, self.W
        C, L = (int(s) for s in self.audio.shape[1:]) if self.audio is not None else (29, 16)
        out = [(k, s, d) for k, _, s, d in RECORD[:3]]
        out.append(("original_image", (3, H, W), torch.float32))
        out += [("auds", (8, C, L), torch.float32), ("au_exp", (6,), torch.float32)]
        out += [(k, (H, W), torch.bool) for k in ("face_mask", "hair_mask", "mouth_mask")]
        out.append(("lips_rect", (4,), torch.int32))
        if priors:
            out += [("normal", (3, H, W), torch.float32), ("depth", (H, W), torch.float32)]
        if background:
            out.append(("background", (3, H, W), torch.float32))
        return tuple(out)

    def empty_frame(self, background: bool = False, priors: bool = False) -> Frame:
        """A zeroed packed Frame of ``layout(...)`` on the store's device."""
        lay = self.layout(background, priors)
        offs, total = _offsets(lay)
        buf = torch.zeros(total, dtype=torch.uint8, device=self.device)
        v = {k: buf[o:o + _nbytes(s, d)].view(d).view(s) for (k, s, d), o in zip(lay, offs)}
        td = {k: v[k] for k, _, _ in lay if k not in Frame.TENSORS}
        f = Frame(self.H, self.W, self.FoVx, self.FoVy, v["world_view_transform"], v["full_proj_transform"],
                  v["camera_center"], td, v["original_image"])
        f._buf, f._layout = buf, lay
        return f

    def frame(self, i: int, background: bool = True, priors: Optional[bool] = None) -> Frame:
        """Frame ``i`` as a freshly packed Frame (for eager use): with the background, and the priors when held."""
        f = self.empty_frame(background, self.has_priors if priors is None else priors)
        self.unpack_into(f, i)
        return f

    def ref(self, i: int, background: bool = True, priors: Optional[bool] = None) -> StoredFrame:
        """Handle of frame ``i``; ``background`` / ``priors`` say what its materialised form carries (the face and
        mouth stages read no background: a static frame cloned from ``ref(i, background=False)`` spares its write)."""
        self._locate(i)
        return StoredFrame(self, i, background, priors)

    def unpack_torch(self, i: int, background: bool = True, priors: Optional[bool] = None) -> dict:
        """What instag_frame_unpack writes for frame ``i``, in plain torch: name -> tensor."""
        _, ch, j = self._locate(i)
        rgb, bg, mask = (p[j] for p in self._planes(ch))
        out = dict(original_image=rgb.permute(2, 0, 1) / 255.0)
        if background:
            out["background"] = bg.permute(2, 0, 1) / 255.0
        for bit, k in enumerate(("face_mask", "hair_mask", "mouth_mask")):
            out[k] = ((mask >> bit) & 1).bool()
        for k, first, shape, dtype in RECORD:
            n = 1
            for s in shape:
                n *= s
            out[k] = ch.records[j, first:first + n].view(dtype).reshape(shape).clone()
        out["auds"] = audio_window(self.audio, self._audio_index(i))
        if self.has_priors if priors is None else priors:
            if ch.normal is None:
                raise ValueError("the store holds no priors")
            out["normal"], out["depth"] = ch.normal[j].clone(), ch.depth[j].clone()
        return out

    def unpack_into(self, static: Frame, i: int):
        """Expand frame ``i`` into the packed Frame ``static`` (Frame.packed): one launch on the current stream."""
        lay, buf = getattr(static, "_layout", None), getattr(static, "_buf", None)
        if lay is None or buf is None:
            raise ValueError("unpack_into: the destination must be a packed Frame (Frame.packed)")
        k, ch, j = self._locate(i)
        a_idx = self._audio_index(i)
        if buf.device.type != "cuda":
            want = self._check_layout(lay)
            src = self.unpack_torch(i, background="background" in want, priors="normal" in want)
            for name in want:
                t = getattr(static, name) if name in Frame.TENSORS else static.talking_dict[name]
                t.copy_(src[name])
            return
        key = (buf.data_ptr(), buf.numel(), k)
        hit = self._args.get(key)
        if hit is None or hit[0] is not lay:
            offs = dict(zip(self._check_layout(lay), _offsets(lay)[0]))
            a = _lib.FrameUnpackArgs()
            a.store, a.records, a.audio, a.dst = ch.buf.data_ptr(), ch.records.data_ptr(), self.audio.data_ptr(), \
                buf.data_ptr()
            a.normal = ch.normal.data_ptr() if ch.normal is not None else None
            a.depth = ch.depth.data_ptr() if ch.depth is not None else None
            a.dst_bytes = buf.numel()
            for name, field in _ARG_OF.items():
                setattr(a, field, offs.get(name, -1))
            a.F, a.H, a.W, a.T = ch.F, self.H, self.W, int(self.audio.shape[0])
            a.audio_row = int(self.audio.shape[1] * self.audio.shape[2])
            hit = self._args[key] = (lay, a, ch.buf, self.audio)      # (the tensors: their addresses stay taken)
        a = hit[1]
        a.idx, a.audio_index = j, a_idx
        with torch.cuda.device(buf.device):
            _lib.check(_lib.lib().instag_frame_unpack(C.byref(a), _lib.current_stream()), "frame_unpack")

    def _check_layout(self, lay):
        """Names of ``lay`` in order; raises for a layout this store cannot serve."""
        if self.audio is None:
            raise RuntimeError("FrameStore: set_audio() first")
        have = {k: (tuple(s), d) for k, s, d in lay}
        names = [k for k, _, _ in lay]
        want = {k: (tuple(s), d) for k, s, d in self.layout("background" in have, "normal" in have or "depth" in have)}
        if ("normal" in have) != ("depth" in have):
            raise ValueError("unpack_into: normal and depth come together")
        if "normal" in have and not self.has_priors:
            raise ValueError("unpack_into: the frame has prior maps, the store holds none")
        if have != want:
            diff = sorted(set(have.items()) ^ set(want.items()), key=str)
            raise ValueError(f"unpack_into: the frame's layout is not one the store fills: {diff}")
        return names


def _nbytes(shape, dtype) -> int:
    n = torch.empty(0, dtype=dtype).element_size()
    for s in shape:
        n *= int(s)
    return n


def _offsets(lay):
    """Byte offsets of a packed Frame's tensors (each on a 256-byte boundary, as Frame.packed lays them out)."""
    offs, total = [], 0
    for _, s, d in lay:
        offs.append(total)
        total += _pad256(_nbytes(s, d))
    return offs, total
