"""Prepare an identity's background, ground-truth and torso frames on the device (csrc/prepare.hip).

The reference makes ``bc.jpg``, ``gt_imgs/`` and ``torso_imgs/`` in its preprocessing script (data_utils/process.py:89-176
extract_background, :199-374 extract_torso_and_gt): a kd-tree query over every pixel of every 20th frame, a [S, H*W]
float64 distance stack, and a per-frame Python loop of lexsort / unique / dilation / blur, on sklearn, scipy and OpenCV.
Both steps need nothing but the decoded frames and their parsing maps, and what they produce is what
``FrameStore.append`` takes in, so here they are integer kernels on 8-bit data that is headed for HBM anyway:

    bc, gt, torso = prepare_identity(path, "cuda")        # reads ori_imgs/*.jpg, parsing/*.png; writes the files
    store, meta = open_identity(path, "train", "cuda")    # the directory is now a processed one

Colours are RGB as PIL decodes them (the reference reads BGR through OpenCV): head (0,0,255), neck (0,255,0),
torso (255,0,0), background (255,255,255).

``background_torch`` and ``frames_torch`` state in plain torch / numpy what the kernels produce; they serve a CPU
device and are the reference of the GPU tests.

Stated deviations from the reference:
  * frame order.  The reference walks ``glob`` order, which depends on the file system and decides which sample wins
    an argmax tie; here frames are sorted by numeric stem.
  * hole filling ties.  The kd-tree's choice among equidistant known pixels is unspecified; here: the smallest squared
    distance, then the smallest row, then the smallest column.
  * the blur of the painted neck pixels is the fixed-point statement below (``BLUR_Q``); its distance to OpenCV's own
    8-bit GaussianBlur is unmeasured (expected: +-1 level on painted neck pixels only).
  * the in-memory route (the returned tensors) skips the JPEG round trip the reference's bc.jpg and gt_imgs/*.jpg go
    through before its loader reads them; the written files go through it as the reference's do.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from . import _lib

HEAD, NECK, TORSO, BACKGROUND = (0, 0, 255), (0, 255, 0), (255, 0, 0), (255, 255, 255)
KNOWN_D2 = 25                       # a pixel is known iff max_d2 > 25  (the reference's max_dist > 5)
L_TORSO, L_NECK, PUSH_DOWN = 9, 53, 4
MIN_H, MIN_W = 64, 3                # the 53-pixel paint wraps at most once; the reflect-101 border of the 5-tap blur
MAX_SIDE = 2048


def _blur_weights():
    w = np.exp(-np.arange(-2, 3, dtype=np.float64) ** 2 / 32.0)          # sigma = 4: 2 sigma^2 = 32
    q = np.round(256.0 * w / w.sum()).astype(np.int64)
    q[2] += 256 - q.sum()
    return q


BLUR_Q = _blur_weights()            # [48, 53, 54, 53, 48]


def darken_table() -> np.ndarray:
    """[53,256] uint8: trunc(v * 0.98**k) as numpy evaluates the reference's paint (fp64 product, truncating cast)."""
    scaler = 0.98 ** np.arange(L_NECK)
    return (np.arange(256)[None, :] * scaler[:, None]).astype(np.uint8)


def _np(x):
    if torch.is_tensor(x):
        x = x.cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint8))


def _is(par, colour):
    return (par[..., 0] == colour[0]) & (par[..., 1] == colour[1]) & (par[..., 2] == colour[2])


def _check_stack(ori, parsing, what):
    if ori.ndim != 4 or ori.shape[-1] != 3 or ori.shape != parsing.shape or ori.shape[0] < 1:
        raise ValueError(f"{what}: ori and parsing [N,H,W,3] uint8, N >= 1")
    H, W = ori.shape[1:3]
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: image sides in 1 .. {MAX_SIDE}")
    return int(ori.shape[0]), int(H), int(W)


# ---- plain statements ---------------------------------------------------------------------------------------------------
def _nearest_in_row(mask):
    """mask [H,W] bool -> column [H,W] int64 of the nearest set pixel of the same row (of two at the same distance
    the left one) and its squared distance (2^40 where the row has none)."""
    W = mask.shape[-1]
    x = np.arange(W, dtype=np.int64)
    big = np.int64(1 << 20)
    left = np.maximum.accumulate(np.where(mask, x, -big), axis=-1)
    right = np.minimum.accumulate(np.where(mask, x, big)[..., ::-1], axis=-1)[..., ::-1]
    col = np.where(x - left <= right - x, left, right)
    g2 = np.where(mask.any(-1, keepdims=True), (x - col) ** 2, np.int64(1) << 40)
    return col, g2


def nearest_set_pixel(mask):
    """mask [H,W] bool (some pixel set) -> d2, sy, sx [H,W] int64: the exact squared Euclidean distance to the nearest
    set pixel and that pixel; among equidistant ones the smallest row, then the smallest column."""
    H, W = mask.shape
    col, g2 = _nearest_in_row(mask)                                       # [H',W]
    d2 = np.empty((H, W), dtype=np.int64)
    sy = np.empty((H, W), dtype=np.int64)
    rows = np.arange(H, dtype=np.int64)
    step = max(1, (1 << 22) // (H * W))
    for y0 in range(0, H, step):
        y = rows[y0:y0 + step]
        dy2 = (y[:, None] - rows[None, :]) ** 2                          # [y,H']
        cand = g2[None, :, :] + dy2[:, :, None]                          # [y,H',W]
        j = cand.argmin(axis=1)                                          # the first minimum: the smallest row
        sy[y0:y0 + step] = j
        d2[y0:y0 + step] = np.take_along_axis(cand, j[:, None, :], axis=1)[:, 0]
    return d2, sy, np.take_along_axis(col, sy, axis=0)


def squared_distance(mask):
    return nearest_set_pixel(mask)[0]


def background_torch(ori, parsing):
    """ori, parsing [S,H,W,3] uint8 -> bc [H,W,3] uint8, max_d2 [H,W] int32, arg [H,W] int32 (torch, on the host).

    max_d2: the maximum over the samples of the squared distance to the sample's nearest non-background pixel; arg: the
    first sample attaining it.  Known pixels (max_d2 > 25) take ori[arg]; every other pixel takes the colour of its
    nearest known pixel (ties: smallest squared distance, then row, then column)."""
    ori, parsing = _np(ori), _np(parsing)
    S, H, W = _check_stack(ori, parsing, "background")
    max_d2 = np.full((H, W), -1, dtype=np.int64)
    arg = np.zeros((H, W), dtype=np.int64)
    for s in range(S):
        fg = ~_is(parsing[s], BACKGROUND)
        if not fg.any():
            raise ValueError(f"background: sample {s} has no non-background pixel")
        d2 = squared_distance(fg)
        better = d2 > max_d2                                             # strictly greater: the first sample wins
        max_d2[better], arg[better] = d2[better], s
    known = max_d2 > KNOWN_D2
    if not known.any():
        raise ValueError("background: no pixel is ever farther than 5 from the foreground")
    yy, xx = np.mgrid[0:H, 0:W]
    bc = np.zeros((H, W, 3), dtype=np.uint8)
    bc[known] = ori[arg[known], yy[known], xx[known]]
    _, sy, sx = nearest_set_pixel(known)
    bc = bc[sy, sx]                                                      # (a known pixel is its own nearest one)
    return torch.from_numpy(bc), torch.from_numpy(max_d2.astype(np.int32)), torch.from_numpy(arg.astype(np.int32))


def hole_sources(known):
    """known [H,W] bool -> (hy, hx, sy, sx): for every unknown pixel the known pixel the tie rule picks, by brute force
    over all pairs (small images: the tests' check of nearest_set_pixel)."""
    ky, kx = np.nonzero(known)
    hy, hx = np.nonzero(~known)
    d2 = (hy[:, None] - ky[None, :]) ** 2 + (hx[:, None] - kx[None, :]) ** 2
    j = np.argmin(d2, axis=1)
    return hy, hx, ky[j], kx[j]


def dilate_neck(neck):
    """neck [...,H,W] bool -> dilated by 3 rows each way, nothing beyond the border (scipy's binary_dilation with the
    vertical 3x3 structuring element, 3 iterations)."""
    out = neck.copy()
    for d in (1, 2, 3):
        out[..., d:, :] |= neck[..., :-d, :]
        out[..., :-d, :] |= neck[..., d:, :]
    return out


def blur5(img):
    """img [H,W,3] uint8 -> the 5x5 fixed-point Gaussian (sigma 4, reflect-101): weights BLUR_Q / 256 per axis,
    horizontal then vertical, (sum + 32768) >> 16."""
    H, W = img.shape[:2]
    v = img.astype(np.int64)

    def reflect(i, n):
        i = np.abs(i)
        return np.where(i >= n, 2 * n - 2 - i, i)

    h = sum(int(BLUR_Q[d + 2]) * v[:, reflect(np.arange(W) + d, W)] for d in range(-2, 3))
    s = sum(int(BLUR_Q[d + 2]) * h[reflect(np.arange(H) + d, H)] for d in range(-2, 3))
    return ((s + 32768) >> 16).astype(np.uint8)


def frames_torch(ori, parsing, bc):
    """ori, parsing [F,H,W,3], bc [H,W,3] uint8 -> gt [F,H,W,3], torso [F,H,W,4] uint8 (torch, on the host): the six
    steps of process.py:199-374 in its order (module docstring: colours, blur)."""
    ori, parsing, bc = _np(ori), _np(parsing), _np(bc)
    F, H, W = _check_stack(ori, parsing, "frames")
    if H < MIN_H or W < MIN_W:
        raise ValueError(f"frames: H >= {MIN_H} and W >= {MIN_W} (the 53-pixel paint wraps at most once)")
    if bc.shape != (H, W, 3):
        raise ValueError("frames: bc [H,W,3]")
    table = darken_table()
    cols = np.arange(W)
    gt_out = np.empty((F, H, W, 3), dtype=np.uint8)
    torso_out = np.empty((F, H, W, 4), dtype=np.uint8)
    for f in range(F):
        par = parsing[f]
        head, neck, torso, bg = _is(par, HEAD), _is(par, NECK), _is(par, TORSO), _is(par, BACKGROUND)
        gt = np.where(bg[..., None], bc, ori[f])
        t = np.where(head[..., None], bc, gt)
        # 3. columns whose topmost torso pixel lies right under head: 9 rows upward, darkening
        yt = torso.argmax(0)
        q3 = torso.any(0) & head[(yt - 1) % H, cols]
        p3 = np.zeros((H, W), dtype=bool)
        if q3.any():
            x, y = cols[q3], yt[q3]
            for k in range(L_TORSO):
                t[(y - k) % H, x] = table[k][gt[y, x]]
                p3[(y - k) % H, x] = True
        # 4. the same from the dilated neck, started up to 4 rows further down, 53 rows
        dn = dilate_neck(neck)
        yn = dn.argmax(0)
        q4 = dn.any(0) & head[(yn - 1) % H, cols]
        p4 = np.zeros((H, W), dtype=bool)
        x = cols[q4]
        y = yn[q4] + np.minimum(dn.sum(0)[q4] - 1, PUSH_DOWN)
        for k in range(L_NECK):
            t[(y - k) % H, x] = table[k][gt[y, x]]
            p4[(y - k) % H, x] = True
        # 5. blur, on the neck paint only, read from the image as it stands
        t[p4] = blur5(t.copy())[p4]
        # 6.
        mask = dn | torso | p3 | p4
        gt_out[f] = gt
        torso_out[f, ..., :3] = t * mask[..., None]
        torso_out[f, ..., 3] = mask * np.uint8(255)
    return torch.from_numpy(gt_out), torch.from_numpy(torso_out)


# ---- the kernels --------------------------------------------------------------------------------------------------------
def _dev_u8(x, device):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device, dtype=torch.uint8).contiguous()


_TABLES = {}


def _table(device):
    key = (device.type, device.index)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(darken_table()).to(device)
    return _TABLES[key]


def background(ori, parsing, device=None):
    """ori, parsing [S,H,W,3] uint8 (the samples) -> bc [H,W,3] uint8, max_d2, arg [H,W] int32 on the device."""
    device = torch.device(device if device is not None else (ori.device if torch.is_tensor(ori) else "cpu"))
    if device.type != "cuda":
        return background_torch(ori, parsing)
    ori, parsing = _dev_u8(ori, device), _dev_u8(parsing, device)
    S, H, W = _check_stack(ori, parsing, "background")
    lib = _lib.lib()
    bc = torch.empty(H, W, 3, dtype=torch.uint8, device=device)
    max_d2 = torch.empty(H, W, dtype=torch.int32, device=device)
    arg = torch.empty(H, W, dtype=torch.int32, device=device)
    nbytes = int(lib.instag_prep_background_workspace_bytes(S, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        rc = lib.instag_prep_background(_lib.ptr(ori), _lib.ptr(parsing), S, H, W, _lib.ptr(bc), _lib.ptr(max_d2),
                                        _lib.ptr(arg), _lib.ptr(ws), nbytes, _lib.current_stream())
    _lib.check_arg(rc, "background")
    return bc, max_d2, arg


def extract_background(ori, parsing, every: int = 20, device=None):
    """bc [H,W,3] from every ``every``-th frame of ori, parsing [N,H,W,3] (process.py:101: image_paths[::20])."""
    return background(ori[::every], parsing[::every], device)[0]


def gt_and_torso(ori, parsing, bc, batch: int = 256, device=None):
    """ori, parsing [N,H,W,3], bc [H,W,3] uint8 -> gt [N,H,W,3], torso [N,H,W,4] uint8 on the device, ``batch`` frames
    per launch (the inputs may live on the host: a batch is uploaded, processed, released)."""
    device = torch.device(device if device is not None else (ori.device if torch.is_tensor(ori) else "cpu"))
    N, H, W = _check_stack(ori, parsing, "frames")
    if H < MIN_H or W < MIN_W:
        raise ValueError(f"frames: H >= {MIN_H} and W >= {MIN_W} (the 53-pixel paint wraps at most once)")
    if tuple(bc.shape) != (H, W, 3):
        raise ValueError("frames: bc [H,W,3]")
    if device.type != "cuda":
        return frames_torch(ori, parsing, bc)
    if batch < 1:
        raise ValueError("frames: batch >= 1")
    bc = _dev_u8(bc, device)
    gt = torch.empty(N, H, W, 3, dtype=torch.uint8, device=device)
    torso = torch.empty(N, H, W, 4, dtype=torch.uint8, device=device)
    frames_into(ori, parsing, bc, gt, torso, batch)
    return gt, torso


def frames_into(ori, parsing, bc, gt, torso, batch: int = 256):
    """The kernels on preallocated contiguous device outputs gt [N,H,W,3], torso [N,H,W,4] (every byte of both is
    written), ``batch`` frames per call.  A batch's uploads are released to the allocator of the stream they are
    read on, so no synchronisation is needed."""
    device = gt.device
    lib = _lib.lib()
    N, H, W = int(gt.shape[0]), int(gt.shape[1]), int(gt.shape[2])
    if not (gt.is_contiguous() and torso.is_contiguous()) or tuple(torso.shape) != (N, H, W, 4):
        raise ValueError("frames: contiguous outputs gt [N,H,W,3], torso [N,H,W,4]")
    table = _table(device)
    cols = torch.empty(min(batch, N) * W * 2, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        for s in range(0, N, batch):
            e = min(N, s + batch)
            o, p = _dev_u8(ori[s:e], device), _dev_u8(parsing[s:e], device)
            rc = lib.instag_prep_frames(_lib.ptr(o), _lib.ptr(p), _lib.ptr(bc), _lib.ptr(table), e - s, H, W,
                                        _lib.ptr(gt[s:e]), _lib.ptr(torso[s:e]), _lib.ptr(cols),
                                        _lib.current_stream())
            _lib.check_arg(rc, "frames")


# ---- a directory --------------------------------------------------------------------------------------------------------
def list_frames(path):
    """Numeric stems of ori_imgs/*.jpg, ascending."""
    stems = [os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(path, "ori_imgs", "*.jpg"))]
    ids = sorted(int(s) for s in stems if s.isdigit())
    if not ids:
        raise FileNotFoundError(f"no ori_imgs/<number>.jpg in {path}")
    return ids


def prepare_identity(path, device, every: int = 20, write: bool = True, batch: int = 256, parsing=None, decoder=None):
    """ori_imgs/*.jpg + parsing/*.png of ``path`` -> (bc [H,W,3], gt [N,H,W,3], torso [N,H,W,4]) uint8 on ``device``,
    frames in ascending numeric order, ready for FrameStore.append.  ``write``: also bc.jpg, gt_imgs/<i>.jpg (quality 95)
    and torso_imgs/<i>.png, after which dataset.open_identity works on the directory.  ``parsing``: the parsing maps
    u8 [N,H,W,3] in the same order (a tensor on any device or an array; parsing.parse_identity's result), used in place
    of reading parsing/*.png.  ``decoder``: a ``jpeg_decode.JpegDecoder``; ori_imgs/*.jpg are then decoded on its device
    (``convnet.frame_batches``) and stay there."""
    from PIL import Image
    ids = list_frames(path)
    if decoder is None:
        ori = np.stack([np.array(Image.open(os.path.join(path, "ori_imgs", f"{i}.jpg")).convert("RGB")) for i in ids])
    else:
        from .convnet import frame_batches
        ori = torch.cat([f.to(decoder.device) for _, f, _ in frame_batches(path, min(batch, 64), decoder=decoder)])
    if parsing is None:
        parsing = np.stack([np.array(Image.open(os.path.join(path, "parsing", f"{i}.png")).convert("RGB")) for i in ids])
    elif tuple(parsing.shape) != tuple(ori.shape):
        raise ValueError(f"prepare_identity: parsing {tuple(parsing.shape)}, the frames are {ori.shape}")
    device = torch.device(device)
    bc = extract_background(ori, parsing, every, device)
    gt, torso = gt_and_torso(ori, parsing, bc, batch, device)
    if write:
        for d in ("gt_imgs", "torso_imgs"):
            os.makedirs(os.path.join(path, d), exist_ok=True)
        Image.fromarray(bc.cpu().numpy(), "RGB").save(os.path.join(path, "bc.jpg"), quality=95)
        for s in range(0, len(ids), batch):
            g, t = gt[s:s + batch].cpu().numpy(), torso[s:s + batch].cpu().numpy()
            for j, i in enumerate(ids[s:s + batch]):
                Image.fromarray(g[j], "RGB").save(os.path.join(path, "gt_imgs", f"{i}.jpg"), quality=95)
                Image.fromarray(t[j], "RGBA").save(os.path.join(path, "torso_imgs", f"{i}.png"))
    return bc, gt, torso
