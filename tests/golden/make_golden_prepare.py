"""Golden G11 (tests/golden/g11_prepare.npz): what sklearn's kd-tree and scipy's binary_dilation answer on a small
synthetic identity, recorded so that the tests of instag_amd.prepare need neither library.

    python tests/golden/make_golden_prepare.py

9 frames of 72 x 40, every 2nd one a background sample (5 samples).  Each frame: a head ellipse, a neck bar under it
and a torso block under that, all jittered per frame, on a white (background) parsing map; the colour frames are noise.
Recorded: the kd-tree distance from every pixel to each sample's nearest non-background pixel reduced the way the
reference reduces it (max over the samples > 5, argmax), the kd-tree's nearest known pixel of every unknown pixel,
and scipy's vertically dilated neck masks (3 iterations of the 3x3 vertical structuring element).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.prepare_helpers import scene  # noqa: E402

H, W, FRAMES, EVERY = 72, 40, 9, 2


def main():
    from scipy.ndimage import binary_dilation
    from sklearn.neighbors import NearestNeighbors
    ori, parsing = scene(FRAMES, H, W, seed=11)
    samples = parsing[::EVERY]
    all_xys = np.mgrid[0:H, 0:W].reshape(2, -1).transpose()
    stack = []
    for par in samples:
        fg = np.stack(np.nonzero(~(par == 255).all(-1))).transpose()
        d, _ = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(fg).kneighbors(all_xys)
        stack.append(d)
    stack = np.stack(stack)
    known = (np.max(stack, 0) > 5).reshape(H, W)
    argmax = np.argmax(stack, 0).reshape(H, W)
    holes = np.stack(np.nonzero(~known)).transpose()
    kn = np.stack(np.nonzero(known)).transpose()
    _, idx = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(kn).kneighbors(holes)
    source = kn[idx[:, 0]]
    structure = np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0]], dtype=bool)
    neck = (parsing[..., 0] == 0) & (parsing[..., 1] == 255) & (parsing[..., 2] == 0)
    dilated = np.stack([binary_dilation(n, structure=structure, iterations=3) for n in neck])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g11_prepare.npz")
    np.savez_compressed(out, ori=ori, parsing=parsing, every=np.int64(EVERY), known=known, argmax=argmax.astype(np.uint8),
                        hole_source=source.astype(np.uint8), dilated_neck=np.packbits(dilated, axis=-1),
                        max_dist_sq_rounded=np.rint(np.max(stack, 0).reshape(H, W) ** 2).astype(np.int32))
    print(out, os.path.getsize(out), "bytes;", int(known.sum()), "known,", len(holes), "holes")


if __name__ == "__main__":
    main()
