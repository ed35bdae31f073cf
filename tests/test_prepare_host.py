"""CPU: the plain statements of instag_amd.prepare against golden G11 (sklearn's kd-tree, scipy's dilation, recorded by
tests/golden/make_golden_prepare.py), against a scalar restatement of the torso steps, and on hand-built columns."""
import ctypes
import os

import numpy as np
import pytest
import torch

from instag_amd import prepare as P
from tests import prepare_helpers as PH


@pytest.fixture(scope="module")
def g11(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "g11_prepare.npz")))
    g["every"] = int(g["every"])
    g["dilated_neck"] = np.unpackbits(g["dilated_neck"], axis=-1, count=g["ori"].shape[2]).astype(bool)
    return g


@pytest.fixture(scope="module")
def background(g11):
    e = g11["every"]
    return [t.numpy() for t in P.background_torch(g11["ori"][::e], g11["parsing"][::e])]


def test_known_pixels_and_argmax_match_the_kd_tree(g11, background):
    bc, max_d2, arg = background
    assert max_d2.dtype == np.int32 and arg.dtype == np.int32 and bc.dtype == np.uint8
    assert np.array_equal(max_d2 > 25, g11["known"])
    assert np.array_equal(arg, g11["argmax"].astype(np.int32))
    assert np.array_equal(max_d2, g11["max_dist_sq_rounded"])
    assert len(np.unique(arg)) > 1 and 0 < g11["known"].sum() < g11["known"].size
    ori = g11["ori"][::g11["every"]]
    yy, xx = np.nonzero(g11["known"])
    assert np.array_equal(bc[yy, xx], ori[arg[yy, xx], yy, xx])


def test_hole_fill_matches_the_kd_tree_where_the_nearest_known_pixel_is_unique(g11, background):
    bc, max_d2, arg = background
    known = g11["known"]
    hy, hx, sy, sx = P.hole_sources(known)
    assert np.array_equal(np.stack([hy, hx], 1), np.stack(np.nonzero(~known), 1))
    ky, kx = np.nonzero(known)
    d2 = (hy[:, None] - ky[None]) ** 2 + (hx[:, None] - kx[None]) ** 2
    dmin = d2.min(1)
    unique = (d2 == dmin[:, None]).sum(1) == 1
    print("unique fraction", unique.mean())
    assert unique.mean() >= 0.85
    want = g11["hole_source"].astype(np.int64)
    assert np.array_equal(sy[unique], want[unique, 0]) and np.array_equal(sx[unique], want[unique, 1])
    # everywhere: at the minimum distance, and among those the smallest row, then the smallest column
    assert np.array_equal((hy - sy) ** 2 + (hx - sx) ** 2, dmin)
    raster = np.where(d2 == dmin[:, None], (ky * known.shape[1] + kx)[None], 1 << 30).min(1)
    assert np.array_equal(sy * known.shape[1] + sx, raster)
    assert not unique.all()                                  # the tie rule is exercised
    # the kd-tree's own choice lies at the minimum distance too
    assert np.array_equal((hy - want[:, 0]) ** 2 + (hx - want[:, 1]) ** 2, dmin)
    ori = g11["ori"][::g11["every"]]
    assert np.array_equal(bc[hy, hx], ori[arg[sy, sx], sy, sx])


def test_dilated_neck_matches_scipy(g11):
    par = g11["parsing"]
    neck = (par[..., 0] == 0) & (par[..., 1] == 255) & (par[..., 2] == 0)
    assert neck.any() and np.array_equal(P.dilate_neck(neck), g11["dilated_neck"])
    edge = np.zeros((2, 64, 3), dtype=bool)
    edge[0, 0, 0] = edge[0, 63, 1] = edge[1, 2, 2] = True
    want = np.zeros_like(edge)
    want[0, 0:4, 0] = want[0, 60:64, 1] = want[1, 0:6, 2] = True
    assert np.array_equal(P.dilate_neck(edge), want)


def test_frames_match_the_scalar_restatement_on_the_golden_scene(g11, background):
    ori, par, bc = g11["ori"][:3], g11["parsing"][:3], background[0]
    gt, torso = (t.numpy() for t in P.frames_torch(ori, par, bc))
    painted = 0
    for f in range(3):
        g, t, p3, p4 = PH.naive_frame(ori[f], par[f], bc)
        assert np.array_equal(gt[f], g) and np.array_equal(torso[f], t), f
        painted += int(p4.sum())
    assert painted > 0


def test_hand_built_columns():
    H, W = 64, 9
    ori, par, bc = PH.special_frames(H, W)
    gt, torso = (t.numpy() for t in P.frames_torch(ori, par, bc))
    table = P.darken_table()
    naive = [PH.naive_frame(ori[f], par[f], bc) for f in range(3)]
    for f in range(3):
        assert np.array_equal(gt[f], naive[f][0]) and np.array_equal(torso[f], naive[f][1]), f
    # frame 0, column 1: a torso top at row 0 paints rows 0, H-1 .. H-8 (no blur on the torso paint)
    assert naive[0][2][:, 1].nonzero()[0].tolist() == [0] + list(range(H - 8, H))
    for k in range(9):
        assert torso[0, (0 - k) % H, 1].tolist() == table[k][ori[0, 0, 1]].tolist() + [255], k
    assert not naive[0][2][:, 2].any() and not naive[0][2][:, 7].any()
    assert torso[0, 6:, 2].max() == 0 and (torso[0, 0:6, 2, 3] == 255).all()
    # frame 0, column 4: c = 4 dilated rows, so the paint starts at row 3, not 4, and wraps
    assert naive[0][3][:, 4].nonzero()[0].tolist() == [0, 1, 2, 3] + list(range(H - 49, H))
    # frame 1, column 1: the same at the bottom border
    assert naive[1][3][:, 1].nonzero()[0].tolist() == list(range(H - 53, H))
    # frame 1, column 4: the neck paint (rows 23 .. 0, 63 .. 35) over the torso paint (rows 26 .. 18)
    p3, p4 = naive[1][2][:, 4], naive[1][3][:, 4]
    assert p3.nonzero()[0].tolist() == list(range(18, 27)) and p4[18:24].all() and not p4[24:27].any()
    for y in (24, 25, 26):
        assert torso[1, y, 4, :3].tolist() == table[26 - y][ori[1, 26, 4]].tolist()
    assert (torso[1, 35:, 4, 3] == 255).all() and (torso[1, 27:35, 4, 3] == 255).all() and torso[1, 41:, 5].max() == 0
    # frame 2: no column qualifies: the torso image is the torso block and nothing else
    assert not naive[2][2].any() and not naive[2][3].any()
    want = np.zeros((H, W, 4), dtype=np.uint8)
    want[30:41, 2:7, :3], want[30:41, 2:7, 3] = ori[2, 30:41, 2:7], 255
    assert np.array_equal(torso[2], want)
    # gt: bc exactly where the parsing is background
    white = (par == 255).all(-1)
    assert np.array_equal(gt[white], np.broadcast_to(bc, ori.shape)[white]) and np.array_equal(gt[~white], ori[~white])


def test_blur_weights_and_darkening_table():
    assert P.BLUR_Q.tolist() == [48, 53, 54, 53, 48]
    flat = np.full((7, 6, 3), 200, dtype=np.uint8)
    assert np.array_equal(P.blur5(flat), flat)               # the weights sum to 256 per axis
    t = P.darken_table()
    assert t.shape == (53, 256) and t.dtype == np.uint8 and np.array_equal(t[0], np.arange(256))
    scaler = 0.98 ** np.arange(53)
    for k, v in ((1, 255), (8, 100), (52, 255), (52, 1), (17, 200)):
        assert int(t[k, v]) == int(float(v) * scaler[k])


def test_value_errors():
    ori, par = PH.scene(2, 63, 20, 1)
    with pytest.raises(ValueError, match="H >= 64"):
        P.frames_torch(ori, par, np.zeros((63, 20, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="H >= 64"):
        P.gt_and_torso(ori, par, np.zeros((63, 20, 3), dtype=np.uint8))
    ori, par = PH.scene(3, 64, 20, 1)
    par[1] = 255
    with pytest.raises(ValueError, match="sample 1 has no non-background pixel"):
        P.background_torch(ori, par)
    par = np.full_like(par, 255)
    par[:, ::4, ::4] = 0                                    # foreground everywhere within 5 pixels
    with pytest.raises(ValueError, match="no pixel"):
        P.background_torch(ori, par)


def test_cpu_device_routes_and_sampling():
    ori, par = PH.scene(5, 64, 24, 3)
    bc = P.extract_background(ori, par, every=2)
    assert torch.equal(bc, P.background_torch(ori[::2], par[::2])[0])
    gt, torso = P.gt_and_torso(torch.from_numpy(ori), torch.from_numpy(par), bc, batch=2)
    want = P.frames_torch(ori, par, bc)
    assert torch.equal(gt, want[0]) and torch.equal(torso, want[1])


def test_library_exports_the_entry_points_and_checks_arguments():
    from instag_amd import _lib
    lib = _lib.lib()
    for n in ("instag_prep_background_workspace_bytes", "instag_prep_background", "instag_prep_frames"):
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert lib.instag_prep_background_workspace_bytes(5, 72, 40) >= 5 * 72 * 40 * 2 + 6 * 4
    assert lib.instag_prep_background_workspace_bytes(5, 4096, 40) == 0
    one = ctypes.c_void_p(256)
    assert lib.instag_prep_frames(one, one, one, one, 1, 63, 40, one, one, one, None) == 1
    assert b"H in 64" in lib.instag_last_error()
    assert lib.instag_prep_frames(one, one, one, None, 1, 64, 40, one, one, one, None) == 1
    assert lib.instag_prep_background(one, one, 1, 72, 40, one, one, one, one, 16, None) == 3      # INSTAG_E_SPACE
    assert lib.instag_prep_background(one, one, 0, 72, 40, one, one, one, one, 1 << 20, None) == 1
