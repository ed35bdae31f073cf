"""What the JPEG decoder's tests share: the files (this project's encoder's and PIL's own), PIL's pixels of them and the
statement's, each computed once and never changed."""
import functools
import io

import numpy as np
import torch

from tests import mjpeg_helpers as Hh

SIZES = ((1, 1), (8, 8), (17, 9), (33, 47), (40, 56))               # (H, W) of the PIL-written files
QUALITIES = (30, 75, 95, 100)
PIL_SUBS = {0: "4:4:4", 2: "4:2:0"}


def content(H, W, seed=3):
    """Smooth and noisy at once: every quality leaves AC coefficients in every block."""
    return Hh._u8(Hh._typical(H, W, seed) * 0.5 + Hh._noise(H, W, seed + 1, 60) * 0.5)


def pil_encode(frame, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.asarray(frame)).save(buf, "JPEG", **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def pil_files(size, subsampling):
    """The eight files PIL writes of one frame: quality 30 / 75 / 95 / 100, standard and ``optimize=True`` tables."""
    frame = content(*size).numpy()
    return tuple(pil_encode(frame, quality=q, optimize=o, subsampling=subsampling) for q in QUALITIES for o in (False, True))


@functools.lru_cache(maxsize=None)
def pil_pixels(data):
    return torch.from_numpy(Hh.pil_decode(data).copy())


@functools.lru_cache(maxsize=None)
def statement_pixels(data):
    from instag_amd import jpeg_decode as D
    return D.jpeg_decode_torch([data])[0]


@functools.lru_cache(maxsize=None)
def statement_coefficients(data):
    from instag_amd import jpeg_decode as D
    return D.coefficients_from_scan_torch(D.parse_jpeg(data), data)


@functools.lru_cache(maxsize=None)
def big_noise():
    """256 x 320 of noise at quality 100, 4:4:4 (test_mjpeg_gpu.py's frame): (file, the statement's pixels)."""
    from instag_amd import mjpeg as M
    data = M.jpeg_encode_torch(Hh._u8(Hh._noise(256, 320, 11))[None], 100, "4:4:4")[0]
    return data, statement_pixels(data)


def refused():
    """name -> (file, a word its refusal names)."""
    frame = content(40, 56).numpy()
    return {
        "progressive": (pil_encode(frame, progressive=True), "progressive"),
        "restart": (pil_encode(frame, restart_marker_blocks=4), "restart"),
        "4:2:2": (pil_encode(frame, subsampling=1), "2x1"),
        "grayscale": (pil_encode(frame[..., 0]), "1 component"),
        "cut": (pil_encode(frame)[:-2], "EOI"),
    }


def cut_scan(data, keep=0.5):
    """The file with its scan cut to ``keep`` of its bytes, EOI behind it (a kept 0xFF at the cut goes too, so that the
    file still parses)."""
    from instag_amd import jpeg_decode as D
    off, n = D.parse_jpeg(data).scan
    scan = data[off:off + int(n * keep)]
    while scan.endswith(b"\xff"):
        scan = scan[:-1]
    return data[:off] + scan + b"\xff\xd9"
