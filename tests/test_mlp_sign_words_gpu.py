"""GPU: the ReLU sign words the fused MLP forward kernels write and the backward kernels read in place of the
activations (include/instag_hip.h, csrc/mlp.hip), through the C ABI.

A forward also writes the activations themselves (the weight gradients read them), so every check here has its
reference in the same call: the decoded words must equal ``a > 0`` bit for bit, and the backward's outputs must match a
float64 chain built from those activations."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [  # (K0, H, O, NL)
    pytest.param(36, 32, 6, 2, id="align"),
    pytest.param(36, 16, 6, 2, id="eye_att"),
    pytest.param(74, 64, 11, 3, id="umf-sigma"),
    pytest.param(74, 32, 11, 3, id="pmf-sigma"),
]
# 65569 rows are 2050 tiles on at most 2048 waves: some waves walk a second tile, so the prefetch path runs
ROWS = [1, 31, 33, 65569]
HEADS = (36, 32, 32, 16, 6)          # K0, HA, OA, HB, OB of the two shared-input heads
KX, KA, KE = 36, 32, 6


def _lib():
    from instag_amd import _lib as m
    return m


def _words(N):
    # poisoned: a word or bit the kernel does not write shows up as set padding
    return torch.full(((N + 31) // 32, 64), -1, dtype=torch.int32, device="cuda")


def _empty(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def decode(words, half=None):
    """[T,64] int32 -> bool [32 T, 64]: entry (row, feature) per the header's layout.  Bit 16 b + r of word (tile, lane)
    is feature 32 b + (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of row 32 tile + (lane & 31).  half = 0 / 1: only the low / high
    16 bits, read as block 0 (the two heads of instag_mlp2_forward)."""
    T = words.shape[0]
    dev = words.device
    k = torch.arange(32, device=dev)
    bits = ((words.long().unsqueeze(-1) >> k) & 1).bool()                  # [T,64,32]
    if half is not None:
        bits = bits[:, :, 16 * half:16 * half + 16]
        bits = torch.cat([bits, torch.zeros_like(bits)], dim=2)
    lane = torch.arange(64, device=dev).unsqueeze(1)
    r = k & 15
    feature = 32 * (k >> 4) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)     # [64,32]
    row = (lane & 31).expand(64, 32)
    full = torch.zeros(T, 32, 64, dtype=torch.bool, device=dev)
    full[:, row, feature] = bits                                           # a bijection: 64 x 32 bits <-> 32 x 64 entries
    return full.reshape(T * 32, 64)


def check_words(words, act, name):
    N, H = act.shape
    got = decode(words)
    assert torch.equal(got[:N, :H], act > 0), name
    assert not bool(got[N:].any()), f"{name}: bits of rows >= N"
    assert not bool(got[:, H:].any()), f"{name}: bits of features >= H"


def _weights(g, dims):
    return [(torch.randn(dims[i + 1], dims[i], generator=g) / np.sqrt(dims[i])).cuda() for i in range(len(dims) - 1)]


def mlp_forward(x, ws, O, NL):
    m = _lib()
    N, K0 = x.shape
    H = ws[0].shape[0]
    y, a1, s1 = _empty(N, O), _empty(N, H), _words(N)
    a2, s2 = (_empty(N, H), _words(N)) if NL == 3 else (None, None)
    w3 = ws[2] if NL == 3 else None
    m.check(m.lib().instag_mlp_forward(m.ptr(x), m.ptr(ws[0]), m.ptr(ws[1]), m.ptr(w3), m.ptr(y), m.ptr(a1), m.ptr(a2),
                                       m.ptr(s1), m.ptr(s2), N, K0, H, O, NL, m.current_stream()), "mlp_forward")
    return y, a1, a2, s1, s2


def mlp_backward(dy, s1, s2, ws, K0, NL):
    m = _lib()
    N, O = dy.shape
    H = ws[0].shape[0]
    dz1, dx = _empty(N, H), _empty(N, K0)
    dz2 = _empty(N, H) if NL == 3 else None
    w3 = ws[2] if NL == 3 else None
    m.check(m.lib().instag_mlp_backward(m.ptr(dy), m.ptr(s1), m.ptr(s2), m.ptr(ws[0]), m.ptr(ws[1]), m.ptr(w3),
                                        m.ptr(dz1), m.ptr(dz2), m.ptr(dx), N, K0, H, O, NL, m.current_stream()),
            "mlp_backward")
    return dz1, dz2, dx


@functools.lru_cache(maxsize=None)
def mlp_case(K0, H, O, NL, N):
    """One forward + backward through the C ABI; shared by the tests below and left unchanged by them."""
    g = torch.Generator().manual_seed(1000 * N + K0 + H)
    ws = _weights(g, [K0] + [H] * (NL - 1) + [O])
    x = torch.randn(N, K0, generator=g).cuda()
    dy = torch.randn(N, O, generator=g).cuda()
    fwd = mlp_forward(x, ws, O, NL)
    bwd = mlp_backward(dy, fwd[3], fwd[4], ws, K0, NL)
    return x, dy, ws, fwd, bwd


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    for case in (mlp_case, mlp2_case, glue_case):
        case.cache_clear()


def close(got, want, name, tol=2e-5):
    """The bound of test_fused_mlp_forward_backward (the masks are the forward's own here, so no outliers)."""
    err = (got.double() - want).abs()
    scale = max(1.0, float(want.abs().max()))
    assert float(err.max()) <= tol * scale, f"{name}: max err {float(err.max())} scale {scale}"


def reference_backward(dy, ws, a1, a2):
    wd = [w.double() for w in ws]
    g = dy.double() @ wd[-1]
    dz2 = None
    if a2 is not None:
        dz2 = g * (a2 > 0)
        g = dz2 @ wd[1]
    dz1 = g * (a1 > 0)
    return dz1, dz2, dz1 @ wd[0]


@pytest.mark.parametrize("K0,H,O,NL", SHAPES)
@pytest.mark.parametrize("N", ROWS)
def test_mlp_sign_words_decode_to_the_activation_signs(K0, H, O, NL, N):
    _, _, _, (y, a1, a2, s1, s2), _ = mlp_case(K0, H, O, NL, N)
    assert bool(torch.isfinite(a1).all()) and bool((a1 > 0).any()) == (N > 0)
    check_words(s1, a1, "s1")
    if NL == 3:
        check_words(s2, a2, "s2")


@pytest.mark.parametrize("K0,H,O,NL", SHAPES)
@pytest.mark.parametrize("N", ROWS)
def test_mlp_backward_from_sign_words_matches_float64(K0, H, O, NL, N):
    _, dy, ws, (y, a1, a2, s1, s2), (dz1, dz2, dx) = mlp_case(K0, H, O, NL, N)
    r1, r2, rx = reference_backward(dy, ws, a1, a2)
    close(dz1, r1, "dz1")
    if NL == 3:
        close(dz2, r2, "dz2")
    close(dx, rx, "dx")


# ---- the two shared-input heads: one word per lane, head A low half, head B high half ------------------------------------
def mlp2_forward(x, ws):
    m = _lib()
    N = x.shape[0]
    K0, HA, OA, HB, OB = HEADS
    ya, yb, a1a, a1b, s1 = _empty(N, OA), _empty(N, OB), _empty(N, HA), _empty(N, HB), _words(N)
    m.check(m.lib().instag_mlp2_forward(m.ptr(x), *(m.ptr(w) for w in ws), m.ptr(ya), m.ptr(yb), m.ptr(a1a), m.ptr(a1b),
                                        m.ptr(s1), N, K0, HA, OA, HB, OB, m.current_stream()), "mlp2_forward")
    return ya, yb, a1a, a1b, s1


def mlp2_backward(dya, dyb, s1, ws, dx):
    """dx holds the gradient of the input's other consumers on entry (dx_add aliases dx)."""
    m = _lib()
    N = dya.shape[0]
    K0, HA, OA, HB, OB = HEADS
    dz1a, dz1b = _empty(N, HA), _empty(N, HB)
    m.check(m.lib().instag_mlp2_backward(m.ptr(dya), m.ptr(dyb), m.ptr(s1), m.ptr(s1), *(m.ptr(w) for w in ws),
                                         m.ptr(dz1a), m.ptr(dz1b), m.ptr(dx), m.ptr(dx), N, K0, HA, OA, HB, OB,
                                         m.current_stream()), "mlp2_backward")
    return dz1a, dz1b, dx


@functools.lru_cache(maxsize=None)
def mlp2_case(N):
    K0, HA, OA, HB, OB = HEADS
    assert _lib().lib().instag_mlp2_supported(*HEADS)
    g = torch.Generator().manual_seed(7 + N)
    ws = _weights(g, [K0, HA, OA]) + _weights(g, [K0, HB, OB])
    x = torch.randn(N, K0, generator=g).cuda()
    dya, dyb = torch.randn(N, OA, generator=g).cuda(), torch.randn(N, OB, generator=g).cuda()
    other = torch.randn(N, K0, generator=g).cuda()
    fwd = mlp2_forward(x, ws)
    bwd = mlp2_backward(dya, dyb, fwd[4], ws, other.clone())
    return x, dya, dyb, other, ws, fwd, bwd


@pytest.mark.parametrize("N", ROWS)
def test_mlp2_sign_words_pack_both_heads(N):
    K0, HA, OA, HB, OB = HEADS
    *_, (ya, yb, a1a, a1b, s1), _ = mlp2_case(N)
    for half, act, H in ((0, a1a, HA), (1, a1b, HB)):
        got = decode(s1, half)
        assert torch.equal(got[:N, :H], act > 0), half
        assert not bool(got[N:].any()) and not bool(got[:, H:].any()), f"head {half}: padding bits"


@pytest.mark.parametrize("N", ROWS)
def test_mlp2_backward_from_sign_words_adds_onto_dx(N):
    x, dya, dyb, other, ws, (ya, yb, a1a, a1b, s1), (dz1a, dz1b, dx) = mlp2_case(N)
    ra, _, rxa = reference_backward(dya, ws[0:2], a1a, None)
    rb, _, rxb = reference_backward(dyb, ws[2:4], a1b, None)
    close(dz1a, ra, "dz1a")
    close(dz1b, rb, "dz1b")
    close(dx, other.double() + rxa + rxb, "dx")


# ---- sigma_net with the glue operator in front (forward) and behind (backward) ------------------------------------------
def glue_forward(ins, ws, O):
    m = _lib()
    enc_x, aud, eye_pre, enc_a, enc_e = ins
    N, H = enc_x.shape[0], ws[0].shape[0]
    y, a1, a2, s1, s2 = _empty(N, O), _empty(N, H), _empty(N, H), _words(N), _words(N)
    h_in, amb = _empty(N, KX + KA + KE), _empty(N, 3)
    m.check(m.lib().instag_mlp_forward_glue(*(m.ptr(t) for t in ins), *(m.ptr(w) for w in ws), m.ptr(y), m.ptr(a1),
                                            m.ptr(a2), m.ptr(s1), m.ptr(s2), m.ptr(h_in), m.ptr(amb), N, H, O,
                                            m.current_stream()), "mlp_forward_glue")
    return y, a1, a2, s1, s2, h_in, amb


def glue_backward(dy, d_amb, s1, s2, ins, ws, amb):
    m = _lib()
    L = m.lib()
    enc_x, aud, eye_pre, enc_a, enc_e = ins
    N, O = dy.shape
    H = ws[0].shape[0]
    dz1, dz2 = _empty(N, H), _empty(N, H)
    d_enc_x, d_aud, d_eye = _empty(N, KX), _empty(N, KA), _empty(N, KE)
    parts = _empty(L.instag_mlp_backward_glue_num_partials(N), KA + KE)
    m.check(L.instag_mlp_backward_glue(m.ptr(dy), m.ptr(s1), m.ptr(s2), *(m.ptr(w) for w in ws), m.ptr(dz1), m.ptr(dz2),
                                       m.ptr(aud), m.ptr(eye_pre), m.ptr(enc_a), m.ptr(enc_e), m.ptr(amb), m.ptr(d_amb),
                                       m.ptr(d_enc_x), m.ptr(d_aud), m.ptr(d_eye), m.ptr(parts), N, H, O,
                                       m.current_stream()), "mlp_backward_glue")
    return dz1, dz2, d_enc_x, d_aud, d_eye, parts


@functools.lru_cache(maxsize=None)
def glue_case(H, N):
    O = 11
    assert _lib().lib().instag_mlp_backward_glue_supported(KX + KA + KE, H, O, KX, KA, KE)
    g = torch.Generator().manual_seed(11 * N + H)
    ws = _weights(g, [KX + KA + KE, H, H, O])
    ins = [torch.randn(*shape, generator=g).cuda() for shape in ((N, KX), (N, KA), (N, KE), (KA,), (KE,))]
    dy, d_amb = torch.randn(N, O, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda()
    d_amb[:, 2] = 0
    fwd = glue_forward(ins, ws, O)
    bwd = glue_backward(dy, d_amb, fwd[3], fwd[4], ins, ws, fwd[6])
    return ins, dy, d_amb, ws, fwd, bwd


@pytest.mark.parametrize("H", [64, 32])
@pytest.mark.parametrize("N", [33, 65569])
def test_glue_forward_sign_words_decode_to_the_activation_signs(H, N):
    *_, (y, a1, a2, s1, s2, h_in, amb), _ = glue_case(H, N)
    check_words(s1, a1, "s1")
    check_words(s2, a2, "s2")


@pytest.mark.parametrize("H", [64, 32])
@pytest.mark.parametrize("N", [33, 65569])
def test_glue_backward_from_sign_words_matches_the_two_operators(H, N):
    """instag_mlp_backward_glue == instag_mlp_backward (input gradient stored) + instag_motion_glue_backward, within the
    bound test_glue_sigma_backward_kernel_matches_the_two_operators sets for the same pair of paths."""
    m = _lib()
    L = m.lib()
    ins, dy, d_amb, ws, (y, a1, a2, s1, s2, h_in, amb), (dz1, dz2, d_enc_x, d_aud, d_eye, parts) = glue_case(H, N)
    enc_x, aud, eye_pre, enc_a, enc_e = ins
    u1, u2, d_h_in = mlp_backward(dy, s1, s2, ws, KX + KA + KE, 3)
    assert torch.equal(u1, dz1) and torch.equal(u2, dz2)
    r_enc_x, r_aud, r_eye = _empty(N, KX), _empty(N, KA), _empty(N, KE)
    r_parts = _empty(L.instag_motion_glue_backward_num_partials(N, KX, KA, KE), KA + KE)
    m.check(L.instag_motion_glue_backward(m.ptr(d_h_in), m.ptr(d_amb), m.ptr(aud), m.ptr(eye_pre), m.ptr(enc_a),
                                          m.ptr(enc_e), m.ptr(amb), m.ptr(r_enc_x), m.ptr(r_aud), m.ptr(r_eye),
                                          m.ptr(r_parts), N, KX, KA, KE, m.current_stream()), "motion_glue_backward")
    pairs = (("d_enc_x", d_enc_x, r_enc_x), ("d_aud", d_aud, r_aud), ("d_eye_pre", d_eye, r_eye),
             ("d_enc_a | d_enc_e", parts.double().sum(0), r_parts.double().sum(0)))
    for name, got, want in pairs:
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert err <= 2e-5 * scale + 1e-6, (name, err, scale)
    # and dz1 / dz2 against the float64 chain from the forward's activations
    r1, r2, _ = reference_backward(dy, ws, a1, a2)
    close(dz1, r1, "dz1")
    close(dz2, r2, "dz2")


# ---- edge values --------------------------------------------------------------------------------------------------------
def test_zero_negative_and_nan_preactivations_clear_the_bit_and_the_gradient():
    """Unit 0 of both hidden layers has a zero weight row (pre-activation exactly 0), unit 1 a negative row over
    non-negative inputs (pre-activation < 0), row 5 of x is NaN (every pre-activation NaN, the ReLU gives 0)."""
    K0, H, O, NL, N, nan_row = 74, 64, 11, 3, 70, 5
    g = torch.Generator().manual_seed(3)
    ws = _weights(g, [K0, H, H, O])
    for w in ws[:2]:
        w[0] = 0.0
        w[1] = -w[1].abs() - 0.01
    x = torch.rand(N, K0, generator=g).cuda() + 0.1          # > 0, and the first layer's activations are >= 0
    x[nan_row] = float("nan")
    dy = torch.randn(N, O, generator=g).cuda()
    y, a1, a2, s1, s2 = mlp_forward(x, ws, O, NL)
    dz1, dz2, dx = mlp_backward(dy, s1, s2, ws, K0, NL)
    finite = torch.ones(N, dtype=torch.bool, device="cuda")
    finite[nan_row] = False
    assert bool((a1[finite] > 0).any()) and bool((a2[finite] > 0).any())
    for words, act, dz, name in ((s1, a1, dz1, "layer 1"), (s2, a2, dz2, "layer 2")):
        check_words(words, act, name)
        bits = decode(words)[:N, :H]
        assert not bool(bits[:, 0].any()), f"{name}: pre-activation 0"
        assert not bool(bits[:, 1].any()), f"{name}: pre-activation < 0"
        assert not bool(bits[nan_row].any()), f"{name}: NaN row"
        cleared = dz[finite][~bits[finite]]
        assert cleared.numel() > 0 and bool((cleared == 0.0).all()), f"{name}: dz where the bit is 0"
        assert bool((dz[finite][:, :2] == 0.0).all())
        assert bool(torch.isfinite(dz[finite]).all())
    assert bool(torch.isfinite(dx[finite]).all())


# ---- repeatability -------------------------------------------------------------------------------------------------------
def _same(a, b):
    for p, q in zip(a, b):
        if p is not None:
            assert torch.equal(p.view(torch.int32), q.view(torch.int32))      # (bitwise: NaN-safe, -0 != +0)


def test_two_calls_give_the_same_bits():
    K0, H, O, NL, N = 74, 64, 11, 3, 65569
    x, dy, ws, fwd, bwd = mlp_case(K0, H, O, NL, N)
    again = mlp_forward(x, ws, O, NL)
    _same(fwd, again)
    _same(bwd, mlp_backward(dy, again[3], again[4], ws, K0, NL))

    x, dya, dyb, other, ws, fwd, bwd = mlp2_case(N)
    again = mlp2_forward(x, ws)
    _same(fwd, again)
    _same(bwd, mlp2_backward(dya, dyb, again[4], ws, other.clone()))

    ins, dy, d_amb, ws, fwd, bwd = glue_case(H, N)
    again = glue_forward(ins, ws, O)
    _same(fwd, again)
    _same(bwd, glue_backward(dy, d_amb, again[3], again[4], ins, ws, again[6]))
