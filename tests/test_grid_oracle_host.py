"""CPU: oracle/grid_ref.py pinned at D = 4 and 5 (16 and 32 corners, the 4th and 5th hash primes, five strides) by a
second, independent statement of the encoder: scalar Python loops, one point at a time, interpolation in fp64.
The GPU matrix (tests/test_grid_matrix_gpu.py) measures every D x C kernel against this oracle."""
import itertools

import numpy as np
import pytest

from oracle import grid_ref

PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037)


def _index(vertex, side, size, hashed):
    """Dense index while the stride fits the level, else prime-xor hash (gridtype hash) or the wrapped partial index
    (tiled); modulo the level size."""
    stride, index = 1, 0
    for v in vertex:
        if stride <= size:
            index += v * stride
            stride *= side
    if hashed and stride > size:
        index = 0
        for v, p in zip(vertex, PRIMES):
            index ^= (v * p) & 0xFFFFFFFF
    return index % size


def _level(offsets, level, S, H, align):
    scale = np.float32(np.exp2(np.float32(level * S))) * np.float32(H) - np.float32(1)      # exp2f(l * S) * H - 1
    side = int(np.ceil(scale)) + (1 if align else 2)
    return scale, side, int(offsets[level]), int(offsets[level + 1] - offsets[level])


def _locate(x, scale, align):
    """fp32 pos and floor (the cell choice), fp64 fraction."""
    pos = np.asarray(x, dtype=np.float32) * scale + np.float32(0.0 if align else 0.5)
    cell = np.floor(pos)
    return [int(c) for c in cell], [float(f) for f in (pos - cell)]


def plain_forward(inputs, emb, offsets, S, H, gridtype, align, interp):
    B, D = inputs.shape
    L, C = len(offsets) - 1, emb.shape[1]
    out = np.zeros((L, B, C))
    dy_dx = np.zeros((B, L, D, C))
    emb = emb.astype(np.float64)
    for b in range(B):
        if ((inputs[b] < 0) | (inputs[b] > 1)).any():
            continue
        for level in range(L):
            scale, side, off, size = _level(offsets, level, S, H, align)
            cell, t = _locate(inputs[b], scale, align)
            dt = [1.0] * D
            if interp == 1:
                dt = [6.0 * f * (1.0 - f) for f in t]
                t = [f * f * (3.0 - 2.0 * f) for f in t]
            for corner in itertools.product((0, 1), repeat=D):
                e = emb[off + _index([c + k for c, k in zip(cell, corner)], side, size, gridtype == 0)]
                w = [f if k else 1.0 - f for f, k in zip(t, corner)]
                out[level, b] += np.prod(w) * e
                for d in range(D):                  # d/dx_d: the factor of axis d becomes +-scale * dt[d]
                    wd = list(w)
                    wd[d] = (1.0 if corner[d] else -1.0) * float(scale) * dt[d]
                    dy_dx[b, level, d] += np.prod(wd) * e
    return out, dy_dx.reshape(B, L * D * C)


def _points(rng, n, D):
    x = rng.uniform(0.0, 1.0, size=(n, D)).astype(np.float32)
    x[0], x[1] = 0.0, 1.0
    x[2, 0], x[3, D - 1] = 1.0, 0.0
    return x


@pytest.mark.parametrize("interp", [0, 1], ids=["linear", "smoothstep"])
@pytest.mark.parametrize("align", [False, True], ids=["noalign", "align"])
@pytest.mark.parametrize("gridtype", ["hash", "tiled"])
@pytest.mark.parametrize("D,C,log2_size", [(4, 2, 8), (5, 1, 9)], ids=["D4", "D5"])
def test_grid_oracle_matches_the_plain_statement(D, C, log2_size, gridtype, align, interp):
    enc = grid_ref.GridEncoderRef(input_dim=D, num_levels=3, level_dim=C, base_resolution=2, per_level_scale_=2,
                                  log2_hashmap_size=log2_size, gridtype=gridtype, align_corners=align, seed=D)
    S, H = np.log2(enc.per_level_scale), enc.base_resolution
    kinds = set()
    for level in range(3):
        _, side, _, size = _level(enc.offsets, level, S, H, align)
        kinds.add("dense" if side ** D <= size else "folded")
    assert kinds == {"dense", "folded"}                 # a dense and a hashed (tiled: wrapped) level both occur
    rng = np.random.default_rng(10 * D + interp)
    enc.embeddings = rng.standard_normal(enc.embeddings.shape).astype(np.float32)
    x = _points(rng, 40, D)
    out, dy_dx = grid_ref.grid_encode_forward(x, enc.embeddings, enc.offsets, S, H, True, enc.gridtype_id, align, interp)
    want, want_dy = plain_forward(x, enc.embeddings, enc.offsets, S, H, enc.gridtype_id, align, interp)
    # the oracle interpolates in fp32: D weight products and a 2^D-term sum, about 40 roundings of 6e-8 on terms
    # bounded by max|e| ~ 4 -> 1e-5; a wrong corner, prime or stride is an O(1) error
    assert np.abs(out - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
    assert np.abs(dy_dx - want_dy).max() <= 2e-5 * max(1.0, np.abs(want_dy).max())


@pytest.mark.parametrize("log2_size", [12, 8], ids=["dense", "hashed"])
@pytest.mark.parametrize("D", [4, 5])
def test_grid_oracle_known_answers_at_4_and_5_dims(D, log2_size):
    """Vertex value = its embedding, cell centre = mean of the 2^D corners, out of [0,1] -> zeros (outputs and dy_dx).
    align_corners with base resolution 5: scale 4, vertices at x = v / 4 exactly."""
    enc = grid_ref.GridEncoderRef(input_dim=D, num_levels=1, level_dim=1, base_resolution=5, per_level_scale_=2,
                                  log2_hashmap_size=log2_size, align_corners=True)
    size = int(enc.offsets[1])
    assert (5 ** D <= size) == (log2_size == 12)
    enc.embeddings = np.arange(size, dtype=np.float32).reshape(-1, 1)
    rng = np.random.default_rng(D)
    vertices = rng.integers(0, 4, size=(6, D))
    vertices[0], vertices[1] = 0, 3
    x = np.concatenate([vertices / 4.0, (vertices + 0.5) / 4.0, np.full((2, D), 0.5), np.full((1, D), 0.5)])
    x[12, D - 1], x[13, 0], x[14, 2] = 1.5, -0.1, np.nextafter(np.float32(1), np.float32(2))
    out, dy_dx = grid_ref.grid_encode_forward(x.astype(np.float32), enc.embeddings, enc.offsets, 1.0, 5, True, 0, True, 0)
    for i, v in enumerate(vertices):
        assert out[0, i, 0] == _index(list(v), 5, size, True)
        corners = [_index([a + k for a, k in zip(v, c)], 5, size, True) for c in itertools.product((0, 1), repeat=D)]
        assert abs(out[0, 6 + i, 0] - np.mean(corners)) <= 1e-6 * size
    assert np.all(out[0, 12:] == 0) and np.all(dy_dx[12:] == 0)
    if log2_size == 12:                              # d/dx_d at a cell centre of the dense ramp: scale * 5^d
        assert np.allclose(dy_dx[6:12].reshape(6, D), 4.0 * 5.0 ** np.arange(D), rtol=1e-5)


def test_grid_oracle_table_gradient_is_exact_by_linearity_at_5_dims_8_channels():
    enc = grid_ref.GridEncoderRef(input_dim=5, num_levels=3, level_dim=8, base_resolution=2, per_level_scale_=2,
                                  log2_hashmap_size=9, seed=1)
    rng = np.random.default_rng(0)
    enc.embeddings = rng.standard_normal(enc.embeddings.shape).astype(np.float32)
    x = _points(rng, 30, 5)
    x[4, 1] = 1.25                                   # an out-of-range row contributes nothing
    S, H = 1.0, 2
    for gridtype, align, interp in ((0, False, 0), (1, True, 1)):
        out, dy_dx = grid_ref.grid_encode_forward(x, enc.embeddings, enc.offsets, S, H, True, gridtype, align, interp)
        w = rng.standard_normal(out.shape).astype(np.float32)
        ge, _ = grid_ref.grid_encode_backward(w, x, enc.embeddings, enc.offsets, S, H, dy_dx, gridtype, align, interp)
        d = rng.standard_normal(enc.embeddings.shape).astype(np.float32)
        out2, _ = grid_ref.grid_encode_forward(x, enc.embeddings + d, enc.offsets, S, H, False, gridtype, align, interp)
        lhs, rhs = ((out2 - out).astype(np.float64) * w).sum(), (ge.astype(np.float64) * d).sum()
        assert abs(lhs - rhs) < 1e-3 * max(1.0, abs(rhs))


@pytest.mark.parametrize("align", [False, True], ids=["noalign", "align"])
def test_grid_oracle_total_variation_on_dense_levels_at_4_dims(align):
    """grad_total_variation against a direct loop: per sample and level the vertex floor(pos), its 2 D axis neighbours
    inside [0, resolution], r = sum (e_v - e_n), q = sum (e_v - e_n)^2, grad[v] += weight / (2 D) * r / sqrt(q + 1e-9)."""
    D, C, weight = 4, 2, 0.5
    enc = grid_ref.GridEncoderRef(input_dim=D, num_levels=2, level_dim=C, base_resolution=2, per_level_scale_=2,
                                  log2_hashmap_size=12, align_corners=align)
    rng = np.random.default_rng(3)
    enc.embeddings = rng.standard_normal(enc.embeddings.shape).astype(np.float32)
    x = rng.uniform(-0.02, 1.02, size=(300, D)).astype(np.float32)
    x[0], x[1] = 0.0, 1.0
    base = rng.standard_normal(enc.embeddings.shape).astype(np.float32)
    want = base.astype(np.float64).copy()
    emb = enc.embeddings.astype(np.float64)
    for level in range(2):
        scale, side, off, size = _level(enc.offsets, level, 1.0, 2, align)
        assert side ** D <= size
        resolution = side if align else side - 1
        for row in x:
            if ((row < 0) | (row > 1)).any():
                continue
            v, _ = _locate(row, scale, align)
            here = off + sum(c * side ** d for d, c in enumerate(v))
            r, q = np.zeros(C), np.zeros(C)
            for d in range(D):
                for n in (v[d] + 1, v[d] - 1):
                    if 0 <= n <= resolution:
                        there = off + (here - off + (n - v[d]) * side ** d) % size
                        r += emb[here] - emb[there]
                        q += (emb[here] - emb[there]) ** 2
            want[here] += weight / (2 * D) * r / np.sqrt(q + 1e-9)
    got = grid_ref.grad_total_variation(x, enc.embeddings, base, enc.offsets, weight, 1.0, 2, 0, align)
    added = np.abs(want - base)
    assert added.max() > 1e-2
    # the oracle sums r and q over 8 neighbours in fp32: ~8 roundings against |r| / sqrt(q) <= sqrt(8) per sample
    assert np.abs(got - want).max() <= 1e-5 * added.max()
    assert np.array_equal(got[added == 0], base[added == 0])
