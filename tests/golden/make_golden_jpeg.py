"""Generate golden G22 (tests/golden/g22_jpeg_decode.npz): four small JPEG files and the pixels PIL (libjpeg-turbo,
``Image.open(...).convert("RGB")``) decodes from them.  It pins the statement of instag_amd/jpeg_decode.py on a machine
whose PIL links another libjpeg, or none.

    python tests/golden/make_golden_jpeg.py

The files: PIL's own of a 33 x 47 frame at quality 75 with 4:2:0 and standard tables, of a 40 x 56 frame at quality 95
with 4:4:4 and ``optimize=True`` tables, of a 17 x 9 frame at quality 30 with 4:2:0 and ``optimize=True`` tables; and
this project's encoder's (``mjpeg.jpeg_encode_torch``) of the 32 x 32 noise case at quality 100, 4:2:0.  Stored per file:
its bytes (uint8) and the pixels uint8 [H,W,3]; and PIL's and its libjpeg's versions as text.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    sys.path.insert(0, ROOT)
    import PIL
    from PIL import features
    from tests import jpeg_decode_helpers as J, mjpeg_helpers as Hh
    files = [
        J.pil_encode(J.content(33, 47).numpy(), quality=75, subsampling=2),
        J.pil_encode(J.content(40, 56).numpy(), quality=95, subsampling=0, optimize=True),
        J.pil_encode(J.content(17, 9).numpy(), quality=30, subsampling=2, optimize=True),
        Hh.statement("noise32", "4:2:0")[0],
    ]
    res = {}
    for i, data in enumerate(files):
        res[f"file{i}"] = np.frombuffer(data, np.uint8)
        res[f"pixels{i}"] = Hh.pil_decode(data)
    version = f"PIL {PIL.__version__}, {features.version('jpg')} (libjpeg-turbo: {features.check_feature('libjpeg_turbo')})"
    res["decoder"] = np.frombuffer(version.encode(), np.uint8)
    path = os.path.join(HERE, "g22_jpeg_decode.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes;", version, [len(f) for f in files])


if __name__ == "__main__":
    main()
