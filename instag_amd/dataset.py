"""Train from a processed identity directory: the reader and the per-stage frame sampler.

``read_identity`` restates the reference's readCamerasFromTransforms (scene/dataset_readers.py:99-324) on the directory
its preprocessing produces -- transforms_{train,val}.json, gt_imgs/, torso_imgs/, bc.jpg, parsing/, teeth_mask/,
ori_imgs/*.lms, au.csv, aud_*.npy, sapiens/ -- and returns the decoded 8-bit arrays plus a metadata table; the
composite, the masks and the audio windows are left to the frame store's kernels (frame_store.py).  ``open_identity``
puts the arrays into a FrameStore.  Everything except ``decode_images`` works on arrays and needs no image library.

``FrameSampler`` restates how each stage picks the frame of an iteration (train_face.py:122-301, train_mouth.py:119-148,
train_fuse_con.py:87-89): pop without replacement from a refilled stack, re-drawn under the stage's curriculum.

One deviation: the reference's mouth-stage loops (train_mouth.py:133-148) do not terminate when no frame qualifies;
here they are bounded the way the face stage bounds its own -- 100 attempts, then the nearest frame.
"""
from __future__ import annotations

import csv
import glob
import json
import math
import os
import random
from typing import Optional

import numpy as np
import torch

from .scene_synth import camera_from_c2w

POSTFIX = {"deepspeech": "_ds", "esperanto": "_eo", "hubert": "_hu"}
AU_EXP_COLUMNS = tuple("AU" + str(i).zfill(2) + "_r" for i in (1, 4, 5, 6, 7, 45))


# ---- the array-level part (dataset_readers.py:103-213, 252-283, 316-317) ------------------------------------------------
def read_au_csv(path) -> dict:
    """au.csv -> {column: float64 array} (the columns pandas.read_csv would give; header names stripped of blanks)."""
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    names = [n.strip() for n in rows[0]]
    body = [r for r in rows[1:] if r]
    keep = set(AU_EXP_COLUMNS) | {"AU25_r"}
    return {n: np.array([float(r[j]) for r in body], dtype=np.float64) for j, n in enumerate(names) if n in keep}


def effective_views(split: str, audio_file: str, n_views: int) -> int:
    """dataset_readers.py:103: a view limit holds for the train split without a driving audio only."""
    return n_views if "train" in split and audio_file == "" else -1


def identity_table(contents: dict, au: dict, landmarks, n_audio: int, split: str, audio_file: str = "",
                   n_views: int = -1, size=None) -> dict:
    """Everything readCamerasFromTransforms derives without touching an image file.

    contents: the parsed transforms file; au: read_au_csv's columns; landmarks: img_id -> [68,2] array (a callable or a
    mapping); n_audio: rows of the audio table; size: (width, height) of the images (for the fields of view).
    The ``[:N_views]`` slices are the reference's: with N_views = -1 they drop the LAST frame and the last AU row."""
    N = effective_views(split, audio_file, n_views)
    focal = contents["focal_len"]
    frames = list(contents["frames"][:N])
    if audio_file != "":
        frames = frames * (n_audio // len(frames) + 1)                            # :153-155
    au_blink = au["AU45_r"]
    au25 = au["AU25_r"]
    au25 = np.clip(au25[:N], 0, np.percentile(au25[:N], 95))                      # :161
    q25, q50, q75, q100 = np.percentile(au25, 25), np.percentile(au25, 50), np.percentile(au25, 75), au25.max()
    cols = []
    for name in AU_EXP_COLUMNS:
        c = au[name]
        if name == "AU45_r":
            c = c.clip(0, 2)
        cols.append(c[:, None])
    au_exp_all = np.concatenate(cols, axis=-1, dtype=np.float32)                  # :172

    get = landmarks if callable(landmarks) else landmarks.__getitem__
    lips, mouth, lhalf = [], [], []
    for fr in frames:                                                             # :178-192
        lms = np.asarray(get(fr["img_id"]))
        xmin, xmax = int(lms[48:60, 1].min()), int(lms[48:60, 1].max())
        ymin, ymax = int(lms[48:60, 0].min()), int(lms[48:60, 0].max())
        lips.append([xmin, xmax, ymin, ymax])
        mouth.append([int(lms[60:68, 1].min()), int(lms[60:68, 1].max())])
        lhalf.append([int(lms[31:36, 1].min()), int(lms[:, 1].max()), int(lms[:, 0].min()), int(lms[:, 0].max())])
    lips, mouth, lhalf = np.array(lips), np.array(mouth), np.array(lhalf)
    opening = mouth[:, 1] - mouth[:, 0]
    mouth_lb, mouth_ub = opening.min(), opening.max()

    out = {k: [] for k in ("img_id", "audio_index", "blink", "au25", "au_exp", "lips_rect", "lhalf_rect", "mouth_bound",
                           "R", "T", "c2w")}
    for idx, fr in enumerate(frames):                                             # :202-320
        img_id = fr["img_id"]
        a_idx = img_id if audio_file == "" else idx
        if (img_id > n_audio) if audio_file == "" else (idx >= n_audio):         # :252-260 (the break)
            break
        c2w = np.array(fr["transform_matrix"], dtype=np.float64)
        flipped = c2w.copy()
        flipped[:3, 1:3] *= -1
        w2c = np.linalg.inv(flipped)
        out["R"].append(np.transpose(w2c[:3, :3]))
        out["T"].append(w2c[:3, 3])
        out["c2w"].append(c2w)
        out["img_id"].append(img_id)
        out["audio_index"].append(a_idx)
        out["blink"].append(np.clip(au_blink[img_id], 0, 2) / 2)
        out["au25"].append([au25[img_id], q25, q50, q75, q100])
        out["au_exp"].append(au_exp_all[img_id])
        xmin, xmax, ymin, ymax = lips[idx].tolist()
        cx, cy = (xmin + xmax) // 2, (ymin + ymax) // 2                           # :271-278: padded to a square
        l = max(xmax - xmin, ymax - ymin) // 2
        out["lips_rect"].append([cx - l, cx + l, cy - l, cy + l])
        out["lhalf_rect"].append(lhalf[idx])
        out["mouth_bound"].append([mouth_lb, mouth_ub, opening[idx]])
    n = len(out["img_id"])
    table = dict(img_id=np.array(out["img_id"], dtype=np.int64), audio_index=np.array(out["audio_index"], dtype=np.int64),
                 blink=np.array(out["blink"], dtype=np.float64), au25=np.array(out["au25"], dtype=np.float64).reshape(n, 5),
                 au_exp=np.array(out["au_exp"], dtype=np.float32).reshape(n, 6),
                 lips_rect=np.array(out["lips_rect"], dtype=np.int64).reshape(n, 4),
                 lhalf_rect=np.array(out["lhalf_rect"], dtype=np.int64).reshape(n, 4),
                 mouth_bound=np.array(out["mouth_bound"], dtype=np.int64).reshape(n, 3),
                 R=np.array(out["R"]).reshape(n, 3, 3), T=np.array(out["T"]).reshape(n, 3),
                 c2w=np.array(out["c2w"]).reshape(n, 4, 4), focal_len=float(focal), n_views=N)
    if size is not None:
        w, h = size
        table["FovX"], table["FovY"] = 2 * math.atan(w / (2 * focal)), 2 * math.atan(h / (2 * focal))
    return table


def audio_table(path, audio_extractor="deepspeech", audio_file="", audio_features=None) -> torch.Tensor:
    """The feature table [T,C,L] (dataset_readers.py:111-150): aud{_ds,_eo,_hu}.npy, ``audio_file`` (.npy) when given;
    for 'ave' aud_ave.npy or ``audio_features`` -- the [N,512,1] array ave_encoder.ave_features makes from a wav."""
    if audio_features is not None:
        feats = np.asarray(audio_features.cpu() if torch.is_tensor(audio_features) else audio_features)
    elif audio_extractor == "ave":
        cache = os.path.join(path, "aud_ave.npy")
        if audio_file != "" or not os.path.exists(cache):
            raise FileNotFoundError("'ave' features: pass audio_features=ave_encoder.ave_features(wav, ...) "
                                    "(no aud_ave.npy in the directory, or a driving audio was named)")
        feats = np.load(cache)
    elif audio_file == "":
        feats = np.load(os.path.join(path, "aud{}.npy".format(POSTFIX[audio_extractor])))
    else:
        feats = np.load(audio_file)
    return torch.from_numpy(np.ascontiguousarray(feats)).float().permute(0, 2, 1).contiguous()


# ---- files --------------------------------------------------------------------------------------------------------------
def decode_images(path, img_ids, extension=".jpg") -> dict:
    """gt [F,H,W,3], torso [F,H,W,4], bc [H,W,3], parsing [F,H,W,3], teeth [F,H,W] uint8 of the listed frames
    (dataset_readers.py:222-246: the conversions the reference applies when it opens each file)."""
    from PIL import Image          # only here: everything else of the module works on arrays
    cache = {}

    def one(i):
        if i not in cache:
            gt = np.array(Image.open(os.path.join(path, "gt_imgs", str(i) + extension)).convert("RGB"))
            torso = np.array(Image.open(os.path.join(path, "torso_imgs", str(i) + ".png")).convert("RGBA"))
            parsing = np.array(Image.open(os.path.join(path, "parsing", str(i) + ".png")).convert("RGB"))
            teeth = np.load(os.path.join(path, "teeth_mask", str(i) + ".npy"))
            cache[i] = (gt, torso, parsing, (teeth != 0).astype(np.uint8))
        return cache[i]

    rows = [one(int(i)) for i in img_ids]
    bc = np.array(Image.open(os.path.join(path, "bc.jpg")).convert("RGB"))
    return dict(gt=np.stack([r[0] for r in rows]), torso=np.stack([r[1] for r in rows]), bc=bc,
                parsing=np.stack([r[2] for r in rows]), teeth=np.stack([r[3] for r in rows]))


def _latest(path, kind):
    c = glob.glob(os.path.join(path, "sapiens", kind, "sapiens_*"))
    c.sort(reverse=True)                                                          # :288-301: the latest folder
    if not c:
        raise FileNotFoundError(f"no sapiens/{kind}/sapiens_* folder in {path}")
    return c[0]


def _select_priors(priors, img_ids):
    """The rows of ``priors`` (read_identity) for the frames ``img_ids``, in their order -> (normal, depth) tensors."""
    if priors.get("normal") is None or priors.get("depth") is None:
        raise ValueError("priors: normal and depth come together (run both networks)")
    where = {int(i): k for k, i in enumerate(np.asarray(priors["ids"]).reshape(-1).tolist())}
    for i in img_ids:
        if int(i) not in where:
            raise KeyError(f"priors: no geometry prior for train frame {int(i)} (ids cover {len(where)} frames)")
    normal, depth = torch.as_tensor(priors["normal"]), torch.as_tensor(priors["depth"])
    rows = torch.tensor([where[int(i)] for i in img_ids], dtype=torch.int64, device=normal.device)
    return normal.index_select(0, rows), depth.index_select(0, rows.to(depth.device))


def read_identity(path, split, audio_extractor="deepspeech", audio_file="", n_views=-1, extension=".jpg",
                  preload_priors: Optional[bool] = None, audio_features=None, priors=None) -> dict:
    """-> dict: the raw uint8 arrays (gt, torso, bc, parsing, teeth), cameras (scene_synth.Camera), au_exp, lips_rect,
    lhalf_rect, audio_index, audio [T,C,L], normal / depth (train split with n_views > 0, unless preload_priors is
    False) and ``meta``: img_id, blink, au25 [F,5], mouth_bound [F,3], R, T, FovX, FovY.
    ``priors``: a dict {"ids", "normal" [N,3,H,W], "depth" [N,H,W]} as ``sapiens.geometry_identity`` returns it, used in
    place of the sapiens/ files (the maps stay tensors on their device); a train frame whose id is not among ``ids``
    raises KeyError naming it."""
    with open(os.path.join(path, f"transforms_{split}.json")) as f:
        contents = json.load(f)
    audio = audio_table(path, audio_extractor, audio_file, audio_features)
    au = read_au_csv(os.path.join(path, "au.csv"))
    lms = lambda i: np.loadtxt(os.path.join(path, "ori_imgs", str(i) + ".lms"))
    table = identity_table(contents, au, lms, int(audio.shape[0]), split, audio_file, n_views)
    out = decode_images(path, table["img_id"], extension)
    h, w = out["gt"].shape[1:3]
    focal = table["focal_len"]
    out["cameras"] = [camera_from_c2w(c, focal, w, h) for c in table["c2w"]]
    out.update(au_exp=table["au_exp"], lips_rect=table["lips_rect"], lhalf_rect=table["lhalf_rect"],
               audio_index=table["audio_index"], audio=audio)
    if split == "train" and table["n_views"] > 0 and preload_priors is not False:      # :286-314
        if priors is not None:
            out["normal"], out["depth"] = _select_priors(priors, table["img_id"])
        else:
            nd, dd = _latest(path, "normal"), _latest(path, "depth")
            out["normal"] = np.stack([np.load(os.path.join(nd, f"{i}.npy")).transpose(2, 0, 1) for i in table["img_id"]])
            out["depth"] = np.stack([np.load(os.path.join(dd, f"{i}.npy")) for i in table["img_id"]])
    out["meta"] = dict(img_id=table["img_id"], blink=table["blink"], au25=table["au25"],
                       mouth_bound=table["mouth_bound"], R=table["R"], T=table["T"],
                       FovX=2 * math.atan(w / (2 * focal)), FovY=2 * math.atan(h / (2 * focal)))
    return out


def open_identity(path, split, device, batch: int = 256, **kw):
    """-> (FrameStore on ``device``, metadata table); the frames are ingested ``batch`` at a time."""
    from .frame_store import FrameStore
    d = read_identity(path, split, **kw)
    store = FrameStore(device)
    n = len(d["cameras"])
    for s in range(0, n, batch):
        p = slice(s, min(n, s + batch))
        store.append(d["gt"][p], d["torso"][p], d["bc"], d["parsing"][p], d["teeth"][p], d["cameras"][p],
                     d["au_exp"][p], d["lips_rect"][p], d["audio_index"][p],
                     normal=d["normal"][p] if "normal" in d else None, depth=d["depth"][p] if "depth" in d else None)
    store.set_audio(d["audio"])
    return store, d["meta"]


# ---- which frame an iteration trains on ---------------------------------------------------------------------------------
class FrameSampler:
    """``next(iteration)`` -> index of the frame that iteration trains on.

    stage 'face' (train_face.py:122-301): before ``warm_step`` every ``select_interval``-th iteration re-draws until the
    frame's mouth opening lies in a window that slides up with the iteration; between ``warm_step`` and
    ``mouth_select_iter`` the same with the blink value; 100 attempts, then the nearest frame.
    stage 'mouth' (train_mouth.py:119-148): before ``warm_step`` only frames at or above the 75 % AU25 quantile;
    afterwards every ``select_interval``-th iteration the sliding AU25 window, and no frame whose mouth mask has fewer
    than 20 pixels (``counts``: FrameStore.counts).  The reference's loops are unbounded; here: 100 attempts, then the
    nearest frame (``capped`` counts how often that happened).
    stage 'fuse' (train_fuse_con.py:87-89): the plain pop.
    meta: blink [F], au25 [F,5], mouth_bound [F,3] (read_identity's table)."""

    def __init__(self, meta, stage: str = "face", seed: int = 0, counts=None, iterations: int = 10000,
                 warm_step: int = 3000, select_interval: Optional[int] = None, max_attempts: int = 100, rng=None):
        if stage not in ("face", "mouth", "fuse"):
            raise ValueError(f"FrameSampler: unknown stage {stage!r}")
        self.stage = stage
        self.rng = rng if rng is not None else random.Random(seed)
        self.blink = [float(x) for x in np.asarray(meta["blink"]).reshape(-1)]
        self.au25 = np.asarray(meta["au25"], dtype=np.float64).tolist()
        self.mouth_bound = np.asarray(meta["mouth_bound"]).tolist()
        self.n = len(self.blink)
        if self.n < 1:
            raise ValueError("FrameSampler: no frames")
        self.mouth_pixels = None if counts is None else [int(c) for c in torch.as_tensor(counts)[:, 2]]
        if stage == "mouth" and self.mouth_pixels is None:
            raise ValueError("FrameSampler: the mouth stage needs the store's counts")
        self.warm_step = warm_step
        self.mouth_select_iter = iterations
        self.mouth_step = 1 / max(iterations, 1)
        self.select_interval = select_interval if select_interval is not None else {"face": 10, "mouth": 5}.get(stage, 1)
        self.max_attempts = max_attempts
        self.stack = []
        self.capped = 0

    def _pop(self) -> int:
        if not self.stack:
            self.stack = list(range(self.n))
        return self.stack.pop(self.rng.randint(0, len(self.stack) - 1))

    def _select(self, cam: int, value, lb, ub) -> int:
        """Re-draw until lb <= value(cam) <= ub; after max_attempts the first frame in the window, else the nearest."""
        attempts = 0
        while (value(cam) < lb or value(cam) > ub) and attempts < self.max_attempts:
            cam = self._pop()
            attempts += 1
        if attempts >= self.max_attempts:
            self.capped += 1
            best, dist = None, float("inf")
            for c in range(self.n):
                v = value(c)
                d = lb - v if v < lb else v - ub if v > ub else None
                if d is None:
                    best = c
                    break
                if d < dist:
                    best, dist = c, d
            if best is not None:
                cam = best
        return cam

    def next(self, iteration: int) -> int:
        cam = self._pop()
        if self.stage == "fuse":
            return cam
        if self.stage == "face":
            g_lb, g_ub = self.mouth_bound[cam][0], self.mouth_bound[cam][1]
            g_lb = g_lb + (g_ub - g_lb) * 0.2
            window = (g_ub - g_lb) * 0.5
            lb = g_lb + self.mouth_step * iteration * (g_ub - g_lb)
            ub = lb + window
            lb = lb - window
            au_lb = 0 + self.mouth_step * iteration * (1 - 0)
            au_ub = au_lb + 0.4
            au_lb = au_lb - 0.4 * 1.5
            if iteration < self.warm_step and iteration < self.mouth_select_iter:
                if iteration % self.select_interval == 0:
                    cam = self._select(cam, lambda c: self.mouth_bound[c][2], lb, ub)
            if self.warm_step < iteration < self.mouth_select_iter:
                if iteration % self.select_interval == 0:
                    cam = self._select(cam, lambda c: self.blink[c], au_lb, au_ub)
            return cam
        g_lb, g_ub = self.au25[cam][1], self.au25[cam][3]
        au_ub = g_ub
        au_lb = au_ub - self.mouth_step * iteration * (g_ub - g_lb)
        au, inf = (lambda c: self.au25[c][0]), float("inf")
        if iteration < self.warm_step:
            cam = self._select(cam, au, g_ub, inf)
        if self.warm_step < iteration < self.mouth_select_iter:
            if iteration % self.select_interval == 0:
                cam = self._select(cam, au, au_lb, au_ub)
            cam = self._select(cam, lambda c: self.mouth_pixels[c], 20, inf)
        return cam
