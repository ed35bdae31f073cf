"""Shared builders for parity tests: same seeded scene on the CPU oracle and on the HIP path."""
import torch

from instag_amd.scene_synth import activated, synthetic_gaussians, toy_cameras
from oracle.rasterize_ref import RasterSettings


def make_scene(n, size, sh_degree=1, seed=0, cam_index=0, bg=(0.0, 1.0, 0.0), scale_mult=1.0):
    cam = toy_cameras(size)[cam_index]
    a = activated(synthetic_gaussians(n, sh_degree=sh_degree, seed=seed))
    a["scales"] = a["scales"] * scale_mult
    a["extra"] = torch.ones(n, 1)
    settings = dict(image_height=size, image_width=size, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                    bg=torch.tensor(bg, dtype=torch.float32), scale_modifier=1.0,
                    viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                    sh_degree=sh_degree, campos=cam.camera_center, prefiltered=False, debug=False)
    return a, settings


def oracle_settings(settings):
    return RasterSettings(**settings)


def hip_settings(settings, device="cuda"):
    from instag_amd.diff_gauss import GaussianRasterizationSettings
    s = dict(settings)
    for k in ("bg", "viewmatrix", "projmatrix", "campos"):
        s[k] = s[k].to(device)
    return GaussianRasterizationSettings(**s)


def leaf(t, device=None):
    t = t.detach().clone()
    if device is not None:
        t = t.to(device)
    return t.requires_grad_(True)


# ---- grid encoder: level paths and unambiguous inputs (tests/test_grid_matrix_gpu.py) -------------------------------
GRID_LDS_BUDGET_FLOATS = 16384      # csrc/grid.hip LDS_BUDGET_FLOATS: forward, level entries x C
GRID_LDS_BWD_ENTRIES = 16384        # csrc/grid.hip LDS_BWD_ENTRIES: backward, level entries x C
GRID_PLANTED = 5                    # rows grid_inputs() plants in front


def grid_level_scales(L, per_level_scale, base_resolution):
    """fp32 scale of every level as the encoder states it: exp2f(l * S) * H - 1."""
    import numpy as np
    S = np.float32(np.log2(per_level_scale))
    return [np.float32(np.exp2(np.float32(l * S))) * np.float32(base_resolution) - np.float32(1) for l in range(L)]


def grid_level_paths(offsets, D, C, per_level_scale, base_resolution, align_corners):
    """Per level: entries, whether the forward / backward kernel keeps it in LDS, whether it is indexed densely
    (side^D <= entries; otherwise hashed, or wrapped for the tiled grid)."""
    import numpy as np
    levels = []
    for l, scale in enumerate(grid_level_scales(len(offsets) - 1, per_level_scale, base_resolution)):
        size = int(offsets[l + 1] - offsets[l])
        side = int(np.ceil(scale)) + (1 if align_corners else 2)
        levels.append(dict(size=size, side=side, lds_fwd=size * C <= GRID_LDS_BUDGET_FLOATS,
                           lds_bwd=size * C <= GRID_LDS_BWD_ENTRIES, dense=side ** D <= size))
    return levels


def grid_border_distance(x01, per_level_scale, base_resolution, L, align_corners):
    """[B] distance of the closest pos = x * scale + (0 or 0.5), over levels and coordinates, from an integer, in ulps
    of pos taken at max(|pos|, 1).  pos is the oracle's: fp32, product and sum rounded separately."""
    import numpy as np
    x01 = np.asarray(x01, dtype=np.float32)
    worst = np.full(x01.shape[0], np.inf)
    for scale in grid_level_scales(L, per_level_scale, base_resolution):
        pos = x01 * scale + np.float32(0.0 if align_corners else 0.5)
        ulp = np.spacing(np.maximum(np.abs(pos), np.float32(1)))
        worst = np.minimum(worst, (np.abs(pos - np.rint(pos)).astype(np.float64) / ulp).min(axis=1))
    return worst


def grid_inputs(D, n, seed, per_level_scale, base_resolution, L, align_corners, k=8, spare=1.08):
    """n rows of [-1.05, 1.05]^D (bound 1) whose cell is the same for every fp32 evaluation order of pos.

    A point whose pos lies within rounding of a cell border may pick the neighbouring cell on the device: dy_dx is
    piecewise constant per cell, a vertex count of the total variation changes by one.  Such rows are removed before
    either side sees them, so that the comparison needs no allowance for outliers: an in-range row is dropped when any
    pos lies within k ulps of an integer.  k = 8: exp2f (1-2 ulp), the multiply by H and the -1 (a little more) and the
    FMA contraction of x * scale + 0.5 (one rounding) are about 4 ulp; 8 doubles that.
    The device's actual deviation from the oracle's pos has NOT been measured yet (a table e[v] = v_0 & 1 makes a linear
    level return the fraction of pos_0, or one minus it, without rounding: that reads pos back exactly).  With the
    doubling levels of tests/test_grid_matrix_gpu.py the scale is exact and only the FMA contraction remains, <= 1 ulp.
    If a run shows a flip beyond k, raise k and record the observed distance here; add no outlier share.

    Planted in front, never dropped (x is 0 or 1 in every coordinate, so x * scale is exact): all zeros, all ones, a
    single coordinate 1, a single coordinate 0, and one row just outside.  Returns (rows [n, D] fp32, dropped share of
    the in-range candidates)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    cand = rng.uniform(-1.05, 1.05, size=(int(n * spare) + 8, D)).astype(np.float32)
    planted = np.zeros((GRID_PLANTED, D), dtype=np.float32)
    planted[0], planted[1] = -1.0, 1.0
    planted[2], planted[3] = -1.0, 1.0
    planted[2, 0], planted[3, D - 1] = 1.0, -1.0
    planted[4, 1 % D] = np.float32(1) + np.float32(2.0 ** -22)       # (x + 1) / 2 = 1 + 2^-23 in fp32
    x01 = (cand + np.float32(1)) / np.float32(2)
    inside = ~((x01 < 0) | (x01 > 1)).any(axis=1)
    drop = inside & (grid_border_distance(x01, per_level_scale, base_resolution, L, align_corners) <= k)
    rows = np.concatenate([planted, cand[~drop]])[:n]
    assert rows.shape[0] == n
    return rows, float(drop.sum()) / float(inside.sum())
