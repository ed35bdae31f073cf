"""GPU parity of the general grid encoder at all sixteen D x C instantiations of csrc/grid.hip (forward, backward, total
variation) against oracle/grid_ref.py, with no allowance for outliers: inputs whose cell depends on the rounding of pos
are removed before either side sees them (tests/helpers.py: grid_inputs)."""
import itertools

import numpy as np
import pytest
import torch

from tests.helpers import GRID_PLANTED, grid_inputs, grid_level_paths
from tests.test_encoders_gpu import _pair
from tests.test_grid_oracle_host import _index

pytestmark = pytest.mark.gpu

# Levels double (the default per_level_scale, 2): exp2f(l) is exact, so the planted rows' pos = scale (+ 0.5) is the same number on
# both sides; fractional level scales are the business of test_encoders_gpu.py.  log2_hashmap_size = 15 - log2(C): the
# largest levels hold 2^15 / C entries, twice either LDS budget.
SHAPES = {2: dict(base_resolution=16, num_levels=5), 3: dict(base_resolution=4, num_levels=5),
          4: dict(base_resolution=2, num_levels=4), 5: dict(base_resolution=2, num_levels=4)}
LOG2_SIZE = {1: 15, 2: 14, 4: 13, 8: 12}
# (gridtype, align_corners, interpolation): every combination twice over the sixteen pairs, four different ones per D
COMBOS = list(itertools.product(("linear", "smoothstep"), (False, True), ("hash", "tiled")))
PAIRS = list(itertools.product((2, 3, 4, 5), (1, 2, 4, 8)))
COMBO_OF = {pair: COMBOS[(3 * k + 2 * (k // 8)) % 8] for k, pair in enumerate(PAIRS)}


def _config(D, C, gridtype=None, align_corners=None):
    interpolation, align, gtype = COMBO_OF[(D, C)]
    return dict(input_dim=D, level_dim=C, log2_hashmap_size=LOG2_SIZE[C],
                gridtype=gridtype or gtype, align_corners=align if align_corners is None else align_corners,
                interpolation=interpolation, **SHAPES[D])


def _paths(enc, cfg):
    """Level paths from enc.offsets; every config must keep all four kinds, whatever the constants become."""
    levels = grid_level_paths(enc.offsets.cpu().numpy(), cfg["input_dim"], cfg["level_dim"], 2, cfg["base_resolution"], cfg["align_corners"])
    assert int(enc.offsets[-1]) <= 250000
    assert any(lv["lds_fwd"] for lv in levels) and any(lv["lds_bwd"] for lv in levels)
    assert any(not lv["lds_fwd"] for lv in levels) and any(not lv["lds_bwd"] for lv in levels)
    assert any(lv["dense"] for lv in levels) and any(not lv["dense"] for lv in levels)
    return levels


def _describe(levels, gridtype):
    folded = "hashed" if gridtype == "hash" else "wrapped"
    return " ".join(f"{lv['size']}:{'lds' if lv['lds_fwd'] else 'global'}/{'lds' if lv['lds_bwd'] else 'atomic'}/"
                    f"{'dense' if lv['dense'] else folded}" for lv in levels)


def _inputs(cfg, n, seed):
    return grid_inputs(cfg["input_dim"], n, seed, 2, cfg["base_resolution"], cfg["num_levels"], cfg["align_corners"])


def _x01(x):
    return (x.astype(np.float32) + np.float32(1)) / np.float32(2)


def _oracle(ref, x, w):
    """outputs [B, L*C], table gradient (fp64-accumulated), input gradient in [0,1] terms, for upstream gradient w."""
    from oracle import grid_ref
    B = x.shape[0]
    L, C = ref.num_levels, ref.level_dim
    out, dy_dx = ref.forward(x, bound=1, calc_grad_inputs=True)
    if w is None:
        return out, None, None
    grad_lbc = np.ascontiguousarray(w.reshape(B, L, C).transpose(1, 0, 2))
    ge, gi = grid_ref.grid_encode_backward(grad_lbc, _x01(x), ref.embeddings, ref.offsets, np.log2(ref.per_level_scale),
                                           ref.base_resolution, dy_dx, ref.gridtype_id, ref.align_corners, ref.interp_id)
    return out, ge, gi


def _device(enc, x, w, input_grad):
    xh = torch.from_numpy(x).cuda().requires_grad_(input_grad)
    enc.embeddings.grad = None
    out = enc(xh, bound=1)
    out.backward(torch.from_numpy(w).cuda())
    gi = xh.grad.cpu().numpy() * 2.0 if input_grad else None            # d/dx of (x + 1) / 2
    return out.detach().cpu().numpy(), enc.embeddings.grad.cpu().numpy(), gi


def _errors(enc, ref, cfg, x, w):
    """Worst error of outputs, table gradient (with and without the input gradient) and input gradient, each divided by
    its bar: all must be <= 1."""
    out_ref, ge_ref, gi_ref = _oracle(ref, x, w)
    out, ge, gi = _device(enc, x, w, True)
    out_b, ge_b, _ = _device(enc, x, w, False)
    finest = cfg["base_resolution"] * 2 ** (cfg["num_levels"] - 1)
    assert out.shape == out_ref.shape == (x.shape[0], enc.output_dim)
    oob = ((_x01(x) < 0) | (_x01(x) > 1)).any(axis=1)
    assert np.all(out[oob] == 0) and np.all(out_b[oob] == 0) and np.all(gi[oob] == 0)
    ge_bar = 2e-4 * max(1.0, np.abs(ge_ref).max())
    return dict(out=max(np.abs(out - out_ref).max(), np.abs(out_b - out_ref).max()) / (1.5e-6 * finest),
                ge=np.abs(ge - ge_ref).max() / ge_bar, ge_noinput=np.abs(ge_b - ge_ref).max() / ge_bar,
                gi=np.abs(gi - gi_ref).max() / (2e-4 * max(1.0, np.abs(gi_ref).max())))


@pytest.mark.parametrize("D,C", PAIRS, ids=[f"D{d}-C{c}" for d, c in PAIRS])
def test_grid_matrix_forward_backward(D, C):
    """One config per (D, C); B = 1500 rows (six workgroups, the last one ragged) of which some are out of range.
    Bars of test_grid_forward_backward, on every element: outputs 1.5e-6 x finest resolution, table gradient
    2e-4 x max(1, max|ref|), input gradient 2e-4 x max(1, max|ref|)."""
    cfg = _config(D, C)
    enc, ref = _pair(cfg, seed=10 * D + C)
    levels = _paths(enc, cfg)
    x, dropped = _inputs(cfg, 1500, seed=100 * D + C)
    assert dropped <= 0.01
    oob = ((_x01(x) < 0) | (_x01(x) > 1)).any(axis=1)
    assert oob[GRID_PLANTED - 1] and not oob[:GRID_PLANTED - 1].any() and 100 < oob.sum() < 1000
    w = np.random.default_rng(D + C).standard_normal((1500, enc.output_dim)).astype(np.float32)
    err = _errors(enc, ref, cfg, x, w)
    print(f"\nGRIDMATRIX D{D} C{C} {cfg['gridtype']} align={cfg['align_corners']} {cfg['interpolation']} | "
          f"{_describe(levels, cfg['gridtype'])} | dropped {100 * dropped:.3f}% | error/bar: "
          + " ".join(f"{k} {v:.3f}" for k, v in err.items()))
    assert err["out"] <= 1 and err["ge"] <= 1 and err["ge_noinput"] <= 1 and err["gi"] <= 1, err


def test_grid_matrix_covers_every_combination_twice():
    for combo in COMBOS:
        assert sum(COMBO_OF[p] == combo for p in PAIRS) == 2
    for D in (2, 3, 4, 5):
        assert len({COMBO_OF[(D, C)] for C in (1, 2, 4, 8)}) == 4


@pytest.mark.parametrize("D,C,gridtype,align", [(4, 1, "hash", False), (5, 2, "tiled", True), (2, 8, "hash", True),
                                                (4, 8, "tiled", False)],
                         ids=["D4-C1-hash", "D5-C2-tiled-align", "D2-C8-hash-align", "D4-C8-tiled"])
def test_grid_matrix_total_variation(D, C, gridtype, align):
    """grad_total_variation: every entry within 2e-6 x max(1, max|added|) of the oracle, entries no sample hit keep
    their bits, two calls give identical bits."""
    from oracle import grid_ref
    cfg = _config(D, C, gridtype, align)
    enc, ref = _pair(cfg, seed=20 * D + C)
    levels = _paths(enc, cfg)
    x, dropped = _inputs(cfg, 4000, seed=7 * D + C)
    assert dropped <= 0.01
    xh = torch.from_numpy(x).cuda()
    base = torch.randn(enc.embeddings.shape, generator=torch.Generator().manual_seed(D * C))
    results = []
    for _ in range(2):
        enc.embeddings.grad = base.clone().cuda()
        enc.grad_total_variation(weight=3e-3, inputs=xh, bound=1)
        results.append(enc.embeddings.grad.clone())
    assert torch.equal(results[0], results[1])
    want = grid_ref.grad_total_variation(_x01(x), ref.embeddings, base.numpy(), ref.offsets, 3e-3,
                                         np.log2(ref.per_level_scale), ref.base_resolution, ref.gridtype_id,
                                         ref.align_corners)
    got = results[0].cpu().numpy()
    added = np.abs(want - base.numpy())
    assert added.max() > 1e-3
    err = np.abs(got - want).max() / (2e-6 * max(1.0, added.max()))
    untouched = added == 0
    print(f"\nGRIDTV D{D} C{C} {gridtype} align={align} | {_describe(levels, gridtype)} | dropped {100 * dropped:.3f}% | "
          f"error/bar {err:.3f} | untouched {untouched.mean():.3f}")
    assert err <= 1
    assert untouched.any() and np.array_equal(got[untouched], base.numpy()[untouched])


EDGE_PAIRS = [(3, 2), (5, 8)]
EDGE_IDS = ["D3-C2", "D5-C8"]


def _edge_case(D, C, n):
    cfg = _config(D, C)
    enc, ref = _pair(cfg, seed=30 * D + C)
    _paths(enc, cfg)
    x, _ = _inputs(cfg, n + 40, seed=9 * D + C)
    x = x[GRID_PLANTED - 2:]                              # one planted row, the row just outside, then drawn rows
    oob = ((_x01(x) < 0) | (_x01(x) > 1)).any(axis=1)
    return cfg, enc, ref, x, 2 + int(np.argmin(oob[2:]))  # ... and the index of the first drawn row that is in range


@pytest.mark.parametrize("D,C", EDGE_PAIRS, ids=EDGE_IDS)
def test_grid_matrix_batch_sizes(D, C):
    """One thread, one short of a workgroup, exactly one, one more; and the empty batch."""
    cfg, enc, ref, x, first = _edge_case(D, C, 300)
    for B in (1, 255, 256, 257):
        xb = x[first:first + 1] if B == 1 else x[:B]      # B = 1: a drawn in-range row
        w = np.random.default_rng(B).standard_normal((B, enc.output_dim)).astype(np.float32)
        err = _errors(enc, ref, cfg, xb, w)
        print(f"\nGRIDBATCH D{D} C{C} B={B} error/bar: " + " ".join(f"{k} {v:.3f}" for k, v in err.items()))
        assert max(err.values()) <= 1, (B, err)
    for input_grad in (True, False):
        xe = torch.zeros(0, D, device="cuda", requires_grad=input_grad)
        enc.embeddings.grad = None
        out = enc(xe, bound=1)
        assert out.shape == (0, enc.output_dim)
        out.backward(torch.zeros_like(out))
        assert enc.embeddings.grad.shape == enc.embeddings.shape and int(torch.count_nonzero(enc.embeddings.grad)) == 0
        assert not input_grad or xe.grad.shape == (0, D)


@pytest.mark.parametrize("case", ["tiny", "huge", "one-row-2^40", "zero"])
@pytest.mark.parametrize("D,C", EDGE_PAIRS, ids=EDGE_IDS)
def test_grid_matrix_fixed_point_range(D, C, case):
    """The LDS accumulators are fixed point, scaled per workgroup from the largest |gradient|: the table gradient keeps
    the 2e-4 bar, relative to the fp64 oracle's own maximum, for upstream gradients x 2^-100, x 2^+100 and with one row
    2^40 times the others; an all-zero upstream gradient gives exact zeros."""
    cfg, enc, ref, x, first = _edge_case(D, C, 700)
    x = x[:700]
    w = np.random.default_rng(5).standard_normal((700, enc.output_dim)).astype(np.float32)
    if case == "tiny":
        w *= np.float32(2.0 ** -100)
    elif case == "huge":
        w *= np.float32(2.0 ** 100)
    elif case == "one-row-2^40":
        w[first] *= np.float32(2.0 ** 40)
    else:
        w[:] = 0
    _, ge, _ = _device(enc, x, w, False)
    if case == "zero":
        assert np.count_nonzero(ge) == 0
        return
    _, ge_ref, _ = _oracle(ref, x, w)
    top = float(np.abs(ge_ref).max())
    assert np.isfinite(top) and top > 0
    err = float(np.abs(ge.astype(np.float64) - ge_ref).max()) / (2e-4 * top)
    print(f"\nGRIDRANGE D{D} C{C} {case} max|ref| {top:.3e} error/bar {err:.4f}")
    assert err <= 1


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["+inf", "-inf", "nan"])
@pytest.mark.parametrize("D,C", EDGE_PAIRS, ids=EDGE_IDS)
def test_grid_matrix_non_finite_gradient_reaches_the_table(D, C, value):
    """A non-finite upstream gradient of one in-range point, at one channel of a level accumulated in LDS: the entries
    that point touches at that level become non-finite, as with the reference's float atomics (gridencoder.cu:248-340);
    every other entry stays finite and correct."""
    cfg, enc, ref, x, first = _edge_case(D, C, 700)
    x = x[:700]
    levels = _paths(enc, cfg)
    row, level, ch = first, 0, C - 1
    assert levels[level]["lds_bwd"]
    w = np.random.default_rng(6).standard_normal((700, enc.output_dim)).astype(np.float32)
    w_clean = w.copy()
    w_clean[row, level * C + ch] = 0
    w[row, level * C + ch] = value
    _, ge, _ = _device(enc, x, w, False)
    # the 2^D corners of that point at that level, by the plain statement of tests/test_grid_oracle_host.py
    scale, side, size = np.float32(cfg["base_resolution"] - 1), levels[level]["side"], levels[level]["size"]
    pos = _x01(x[row]) * scale + np.float32(0.0 if cfg["align_corners"] else 0.5)
    cell = [int(c) for c in np.floor(pos)]
    touched = np.zeros(ge.shape, dtype=bool)
    for corner in itertools.product((0, 1), repeat=D):
        touched[_index([c + k for c, k in zip(cell, corner)], side, size, cfg["gridtype"] == "hash"), ch] = True
    assert not np.isfinite(ge[touched]).any()
    assert np.isfinite(ge[~touched]).all()
    _, ge_ref, _ = _oracle(ref, x, w_clean)
    assert np.abs(ge - ge_ref)[~touched].max() <= 2e-4 * max(1.0, np.abs(ge_ref).max())
