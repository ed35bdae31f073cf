"""GPU edge cases of the four "deform + activate" operators (glue.deform_activate with and without its fused
regulariser, glue.mouth_activate, glue.pretrain_deform, glue.pretrain_mouth_deform): the branches that Gaussian random
inputs never reach.  Each operator is compared with the fp64 plain-torch statement of its existing test, at that test's
tolerances in ``_close``'s form, at N = 1 and at N = 259 (one full workgroup plus three rows).  Planted rows:
  scale       scale pre-activations 20.5 and 19.5: either side of the softplus threshold
  zero-quat   a quaternion whose sum is exactly 0 in fp32 and in fp64: forward 0, gradient g / 1e-12.  The row is
              compared on its own, so that its 1e12-sized gradient does not set the scale for the other rows
  zero-head   head entries that are exactly 0 under a regulariser: the gradient of |.| there is 0
Every case also runs a backward in which the loss reads only means3D (and the regulariser's partial sums), so that the
other three upstream gradients arrive as None."""
import pytest
import torch

from tests.test_glue_gpu import _close
from tests.test_pretrain_gpu import _deform_inputs as _face_inputs, _plain_deform
from tests.test_pretrain_mouth_gpu import XYZ_SCALE, _deform_inputs as _mouth_inputs, _plain_mouth_deform

pytestmark = pytest.mark.gpu

REG_WEIGHT = 0.37


def _randn_inputs(shapes, scales=None):
    def make(N, seed):
        g = torch.Generator().manual_seed(seed)
        return [torch.randn(N, k, generator=g) * a + b for k, (a, b) in zip(shapes, scales or [(1, 0)] * len(shapes))], []
    return make


def _deform_ref(xyz, scaling, rotation, opacity, h, p):
    """tests/test_glue_gpu.py: test_deform_activate_matches_torch / test_deform_activate_with_fused_regulariser"""
    ps = torch.tanh(p[:, 3:] / 5) * 0.25 + 1
    means = xyz + (h[:, :3] * 1e-2) * ps
    scales = torch.nn.functional.softplus(scaling + h[:, 8:11])
    rots = torch.nn.functional.normalize(rotation + h[:, 3:7])
    reg = (((h[:, :3] * 1e-2) * ps).abs().mean() + h[:, 3:7].abs().mean() + h[:, 7:8].abs().mean()
           + h[:, 8:11].abs().mean() + (p[:, :3] * 1e-2).abs().mean())
    return means, scales, rots, torch.sigmoid(opacity), REG_WEIGHT * reg


def _mouth_ref(xyz, scaling, rotation, opacity, h, hs):
    """tests/test_glue_gpu.py: test_mouth_activate_matches_plain_torch"""
    d = (h[..., :3] * torch.tensor(XYZ_SCALE, dtype=h.dtype, device=h.device)) * torch.sigmoid(hs) * 2
    return (xyz + d, torch.nn.functional.softplus(scaling), torch.nn.functional.normalize(rotation),
            torch.sigmoid(opacity), None)


def _hip(name):
    from instag_amd import glue
    return {
        "deform_activate": lambda L, E: glue.deform_activate(*L),
        "deform_activate_reg": lambda L, E: glue.deform_activate(*L, reg_weight=REG_WEIGHT),
        "mouth_activate": lambda L, E: glue.mouth_activate(*L, XYZ_SCALE),
        "pretrain_deform": lambda L, E: glue.pretrain_deform(*L, others=E),
        "pretrain_mouth_deform": lambda L, E: glue.pretrain_mouth_deform(*L, h_q=E[0]),
    }[name]


def _mouth_pre_ref(L, E):
    *outs, sums = _plain_mouth_deform(*L, E[0])
    return (*outs, sum(sums))


# inputs: the existing tests' draws.  ref: -> four outputs and the regulariser's sum (or None).  rot / scale: the (leaf,
# columns) of the heads that are added to the rotation / to the scale pre-activation.  zero: the (leaf, columns) the
# regulariser reads.  reg_mult: what the loss multiplies the regulariser by (the pretraining tests' 1e4, times N so that
# the per-Gaussian means 1e-5 / N keep the size they have at N = 1).  tolerances: (outputs, regulariser, gradients).
OPS = {
    "deform_activate": dict(
        inputs=_randn_inputs((3, 3, 4, 1, 11, 6), [(0.1, 0), (2, -4), (1, 0), (2, 0), (1, 0), (3, 0)]),
        ref=lambda L, E: _deform_ref(*L)[:4] + (None,), rot=[(4, slice(3, 7))], scale=[(4, slice(8, 11))], zero=[],
        tol=(2e-5, None, 1e-4)),
    "deform_activate_reg": dict(
        inputs=_randn_inputs((3, 3, 4, 1, 11, 6)),
        ref=lambda L, E: _deform_ref(*L), rot=[(4, slice(3, 7))], scale=[(4, slice(8, 11))],
        zero=[(4, slice(0, 11)), (5, slice(0, 3))], reg_mult=lambda N: 2.5,
        reg_close=lambda got, want: abs(got - want) <= 1e-6 * max(1.0, abs(want)), tol=(2e-5, None, 2e-5)),
    "mouth_activate": dict(
        inputs=_randn_inputs((3, 3, 4, 1, 7, 1)), ref=lambda L, E: _mouth_ref(*L), rot=[], scale=[], zero=[],
        tol=(2e-6, None, 2e-6)),
    "pretrain_deform": dict(
        inputs=lambda N, seed: _face_inputs(N, 1, seed), ref=lambda L, E: _plain_deform(*L, E),
        rot=[(4, slice(3, 7)), (5, slice(3, 7))], scale=[(4, slice(8, 11)), (5, slice(8, 11))],
        zero=[(4, slice(0, 11)), (5, slice(0, 11))], reg_mult=lambda N: 1e4 * N,
        reg_close=lambda got, want: abs(got - want) <= 2e-6 * abs(want), tol=(1e-6, None, 2e-4)),
    "pretrain_mouth_deform": dict(
        inputs=lambda N, seed: (lambda base, hq: (base, [hq]))(*_mouth_inputs(N, seed)), ref=_mouth_pre_ref,
        rot=[], scale=[], zero=[(4, slice(0, 7)), (6, slice(0, 7))], reg_mult=lambda N: 1e4 * N,
        reg_close=lambda got, want: abs(got - want) <= 2e-6 * abs(want), tol=(1e-6, None, 2e-4)),
}
MODES = {False: ("geometry", "means"), True: ("geometry+reg", "reg", "means+reg")}
ROWS_259 = {"scale": 3, "zero-head": 100, "zero-quat": 257}          # (257: in the second workgroup)


def _plant(op, base, kind, r):
    if kind == "scale":
        for c, pre in enumerate((20.5, 19.5)):
            base[1][r, c] = pre - sum(float(base[i][r, cols][c]) for i, cols in op["scale"])
    elif kind == "zero-quat":
        base[2][r] = 0.0
        for j, (i, cols) in enumerate(op["rot"]):
            if j == 0:
                base[2][r] = -base[i][r, cols]
            else:
                base[i][r, cols] = 0.0
    elif kind == "zero-head":
        for i, cols in op["zero"]:
            base[i][r, cols] = 0.0


def _cases():
    out = []
    for name, op in OPS.items():
        kinds = ["scale", "zero-quat"] + (["zero-head"] if op["zero"] else [])
        out += [(name, 1, k) for k in kinds] + [(name, 259, "all")]
    return out


def _compare(a, b, name, tol, own):
    """``_close`` on the zero-quaternion row ``own`` (or None) and on the other rows separately"""
    rest = torch.ones(b.shape[0], dtype=torch.bool, device=b.device)
    if own is not None:
        rest[own] = False
        _close(a[own], b[own], name + "[zero-quat row]", tol)
    if bool(rest.any()):
        _close(a[rest], b[rest], name, tol)


@pytest.mark.parametrize("name,N,kind", _cases(), ids=lambda v: str(v))
def test_deform_operator_edges_match_fp64_statement(name, N, kind):
    op, dev = OPS[name], torch.device("cuda")
    base, extra = op["inputs"](N, seed=31 + N)
    rows = {kind: 0} if N == 1 else {k: r for k, r in ROWS_259.items() if k != "zero-head" or op["zero"]}
    for k, r in rows.items():
        _plant(op, base, k, r)
    own = rows.get("zero-quat")
    base, extra = [t.to(dev) for t in base], [t.to(dev) for t in extra]
    if "scale" in rows:
        pre = base[1][rows["scale"], :2] + sum(base[i][rows["scale"], cols][:2] for i, cols in op["scale"])
        assert float(pre[0]) > 20.0 > float(pre[1]) > 19.0
    g = torch.Generator().manual_seed(5)
    w = [torch.randn(N, k, generator=g).to(dev) for k in (3, 3, 4, 1)]
    tol_out, _, tol_grad = op["tol"]
    has_reg = "reg_mult" in op

    def run(fn, leaves, extra, mode, w):
        *outs, reg = fn(leaves, extra)
        take = 4 if "geometry" in mode else (1 if "means" in mode else 0)
        loss = sum((o * wi).sum() for o, wi in zip(outs[:take], w[:take]))
        if "reg" in mode:
            loss = loss + reg.sum() * op["reg_mult"](N)
        loss.backward()
        return [o.detach() for o in outs], None if reg is None else float(reg.detach().double().sum()), \
            [t.grad for t in leaves]

    hip = _hip(name) if has_reg else (lambda L, E, f=_hip(name): (*f(L, E), None))
    for mode in MODES[has_reg]:
        got, got_reg, got_g = run(hip, [t.clone().requires_grad_(True) for t in base], extra, mode, w)
        want, want_reg, want_g = run(op["ref"], [t.double().requires_grad_(True) for t in base],
                                     [t.double() for t in extra], mode, [t.double() for t in w])
        for a, b, n in zip(got, want, ("means3D", "scales", "rotations", "opacity")):
            _compare(a, b, f"{mode} {n}", tol_out, own)
        if has_reg:
            print(f"{mode} reg: got {got_reg!r} want {want_reg!r}")
            assert op["reg_close"](got_reg, want_reg), (mode, got_reg, want_reg)
        for i, (a, b) in enumerate(zip(got_g, want_g)):
            if b is None:
                assert a is None or float(a.abs().max()) == 0.0, (mode, i)
                continue
            _compare(a, b, f"{mode} d_leaf{i}", tol_grad, own)
        if own is not None:
            assert float(got[2][own].abs().max()) == 0.0 and float(want[2][own].abs().max()) == 0.0
            if "geometry" in mode:
                # (only d_rotation: a head that is added to the rotation also takes its regulariser's gradient)
                _close(got_g[2][own], w[2][own].double() / 1e-12, f"{mode} d_rotation == g / 1e-12", tol_grad)
