"""The tri-plane encode fused into the motion fields' forward MLP kernels (csrc/mlp.hip: triplane_mlp_forward_kernel,
triplane_mlp2_forward_kernel) == the two launches it replaces, bit for bit; one independent check against the numpy
oracle; one train step fused against INSTAG_ENCODE_MLP=split."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FACE = dict(input_dim=2, num_levels=12, level_dim=1, base_resolution=16, log2_hashmap_size=17,
            desired_resolution=256 * 0.15)
BOUND = 0.15
NMAX = 2053
# (hidden, out) of the heads: align_net; aud_ch_att_net + eye_att_net
HEADS = {"align": [(32, 6)], "heads": [(32, 32), (16, 6)]}


class _Scene:
    """Tables, weights, points and shifts shared by every case (built once, never written)."""

    def __init__(self):
        from instag_amd.gridencoder import GridEncoder
        dev = torch.device("cuda")
        g = torch.Generator().manual_seed(3)
        enc = GridEncoder(**FACE)
        self.offsets = enc.offsets.to(dev)
        self.L = enc.num_levels
        self.S = float(np.log2(enc.per_level_scale))
        self.H = int(enc.base_resolution)
        self.T = int(enc.embeddings.shape[0])
        self.tables_host = [torch.randn(self.T, generator=g) for _ in range(3)]
        self.tables = [t.to(dev) for t in self.tables_host]
        # the same values one element into a buffer: 4-byte but not 16-byte aligned -> the scalar staging branch
        self._odd = [torch.cat([torch.zeros(1), t]).to(dev) for t in self.tables_host]
        self.tables_odd = [b[1:] for b in self._odd]
        assert all(t.data_ptr() % 16 == 4 for t in self.tables_odd)
        x = torch.rand(NMAX, 3, generator=g) * 0.34 - 0.17        # some points outside the bound -> zero rows
        x[1] = torch.tensor([BOUND, -BOUND, BOUND])               # exactly on the faces of the box
        x[2] = torch.tensor([-BOUND, 0.03, -BOUND])
        x[3] = torch.tensor([0.16, 0.0, 0.0])                     # outside in two planes, inside in yz
        x[40] = torch.tensor([BOUND, BOUND, BOUND])
        x[NMAX - 1] = torch.tensor([-BOUND, -BOUND, 0.2])
        self.x_host = x
        self.x = x.to(dev)
        # shifts of a size that moves points across cells and across the bound (scale 1e-2 as the alignment head's)
        self.shift_host = {k: torch.randn(NMAX, k, generator=g) * 2.0 for k in (3, 6)}
        self.shift = {k: v.to(dev) for k, v in self.shift_host.items()}
        self.weights_host = {kind: [w for h, o in hs for w in (torch.randn(h, 36, generator=g) / 6.0,
                                                             torch.randn(o, h, generator=g) / np.sqrt(h))]
                             for kind, hs in HEADS.items()}
        self.weights = {k: [w.to(dev) for w in ws] for k, ws in self.weights_host.items()}
        self._split = {}

    def _outputs(self, kind, N, keep):
        dev = self.x.device
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        out = {"enc_x": z(N, 36)}
        for tag, (h, o) in zip("ab", HEADS[kind]):
            out["y" + tag] = z(N, o)
            out["a1" + tag] = z(N, h) if keep else None
        out["s1"] = z((N + 31) // 32, 64, dt=torch.int32) if keep else None
        return out

    def _encoder_args(self, N, shift, tables):
        from instag_amd._lib import ptr
        sh = None if shift is None else self.shift[shift][:N].contiguous()
        return sh, (ptr(self.x[:N].contiguous()), ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), ptr(self.offsets))

    def split(self, kind, N, shift, keep, odd=False):
        """instag_triplane_forward, then instag_mlp_forward / instag_mlp2_forward (computed once per case)."""
        key = (kind, N, shift, keep, odd)
        if key not in self._split:
            from instag_amd import _lib
            from instag_amd._lib import check, ptr
            L = _lib.lib()
            o = self._outputs(kind, N, keep)
            sh, enc = self._encoder_args(N, shift, self.tables_odd if odd else self.tables)
            st = _lib.current_stream()
            check(L.instag_triplane_forward(*enc, ptr(o["enc_x"]), ptr(sh), 0 if sh is None else sh.shape[1], 1e-2, N,
                                            self.L, self.S, self.H, BOUND, self.T, st), "triplane_forward")
            w = self.weights[kind]
            if kind == "align":
                check(L.instag_mlp_forward(ptr(o["enc_x"]), ptr(w[0]), ptr(w[1]), None, ptr(o["ya"]), ptr(o["a1a"]), None,
                                           ptr(o["s1"]), None, N, 36, 32, 6, 2, st), "mlp_forward")
            else:
                check(L.instag_mlp2_forward(ptr(o["enc_x"]), ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(o["ya"]),
                                            ptr(o["yb"]), ptr(o["a1a"]), ptr(o["a1b"]), ptr(o["s1"]), N, 36, 32, 32, 16, 6,
                                            st), "mlp2_forward")
            torch.cuda.synchronize()
            self._split[key] = o
        return self._split[key]

    def fused(self, kind, N, shift, keep, max_blocks=0, odd=False):
        from instag_amd import _lib
        from instag_amd._lib import check, ptr
        L = _lib.lib()
        o = self._outputs(kind, N, keep)
        sh, enc = self._encoder_args(N, shift, self.tables_odd if odd else self.tables)
        common = (*enc, ptr(sh), 0 if sh is None else sh.shape[1], 1e-2, N, self.L, self.S, self.H, BOUND, self.T)
        w = self.weights[kind]
        if kind == "align":
            assert L.instag_triplane_mlp_supported(self.L, self.T, 1, 32, 6, 0, 0)
            check(L.instag_triplane_mlp_forward(*common, ptr(w[0]), ptr(w[1]), ptr(o["enc_x"]), ptr(o["ya"]), ptr(o["a1a"]),
                                                ptr(o["s1"]), 32, 6, max_blocks, _lib.current_stream()),
                  "triplane_mlp_forward")
        else:
            assert L.instag_triplane_mlp_supported(self.L, self.T, 2, 32, 32, 16, 6)
            check(L.instag_triplane_mlp2_forward(*common, ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(o["enc_x"]),
                                                 ptr(o["ya"]), ptr(o["yb"]), ptr(o["a1a"]), ptr(o["a1b"]), ptr(o["s1"]),
                                                 32, 32, 16, 6, max_blocks, _lib.current_stream()),
                  "triplane_mlp2_forward")
        torch.cuda.synchronize()
        return o


@pytest.fixture(scope="module")
def scene():
    return _Scene()


def _same(got, want, tag):
    assert got.keys() == want.keys()
    for k, w in want.items():
        if w is None:
            assert got[k] is None, (tag, k)
        else:
            assert torch.equal(got[k], w), (tag, k, int((got[k] != w).sum()))


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("kind", ["align", "heads"])
@pytest.mark.parametrize("shift", [None, 3, 6])
def test_fused_kernels_equal_the_split_launches_bit_for_bit(scene, kind, shift, keep):
    """enc_x, every Y, every A1 and the sign words, at the tile edges and with one or two workgroups walking 65 tiles
    (the last one ragged); the points include rows outside the bound and exactly on it."""
    for N in (1, 31, 32, 33, NMAX):
        want = scene.split(kind, N, shift, keep)
        if N == NMAX:
            # out-of-bound points are there: a coordinate is outside for 12 % of them (without the shift), which
            # zeroes a plane's 12 columns for 22 % of the rows and the whole row for 4 %
            zero = want["enc_x"].view(N, 3, 12).abs().sum(2) == 0
            assert float(zero[:, 0].float().mean()) > 0.1 and float(zero.all(1).float().mean()) > 0.01
            assert float((want["enc_x"] != 0).float().mean()) > 0.5
        for mb in ((0, 1, 2) if N == NMAX else (0,)):
            _same(scene.fused(kind, N, shift, keep, mb), want, (N, mb))


@pytest.mark.parametrize("kind", ["align", "heads"])
def test_fused_kernels_with_unaligned_tables(scene, kind):
    """A table pointer at an odd element offset: both paths stage with the scalar loop."""
    want = scene.split(kind, NMAX, 6, True, odd=True)
    _same(want, scene.split(kind, NMAX, 6, True), "aligned")
    _same(scene.fused(kind, NMAX, 6, True, 2, odd=True), want, "odd")


def test_predicate_refuses_what_has_no_kernel(scene):
    from instag_amd import _lib
    L = _lib.lib()
    assert not L.instag_triplane_mlp_supported(12, 46600, 1, 32, 6, 0, 0)         # the mouth field's tables
    assert not L.instag_triplane_mlp_supported(12, 46600, 2, 32, 32, 16, 6)
    assert not L.instag_triplane_mlp_supported(11, scene.T, 1, 32, 6, 0, 0)
    assert not L.instag_triplane_mlp_supported(12, scene.T, 1, 64, 6, 0, 0)
    assert not L.instag_triplane_mlp_supported(12, scene.T, 2, 32, 32, 32, 6)
    assert not L.instag_triplane_mlp_supported(12, scene.T, 3, 32, 32, 16, 6)


def test_fused_kernels_against_the_numpy_oracle_and_a_torch_mlp(scene):
    """Independent of the split kernels: enc_x against oracle/grid_ref.py plane by plane (tolerance of
    test_tri_plane_kernels_against_the_numpy_oracle), the heads against a float64 torch MLP over those rows (tolerance of
    tests/test_mlp_gpu.py)."""
    from oracle.grid_ref import GridEncoderRef
    refs = [GridEncoderRef(seed=s, **FACE) for s in (1, 2, 3)]
    for r, t in zip(refs, scene.tables_host):
        assert r.embeddings.shape == (scene.T, 1)
        r.embeddings = t.numpy().reshape(scene.T, 1).copy()
    p = (scene.x_host + 1e-2 * scene.shift_host[6][:, :3]).numpy()      # fp32, as the kernel forms the point
    cols = [(0, 1), (1, 2), (0, 2)]                                      # xy, yz, xz
    enc_ref = np.concatenate([r.forward(p[:, list(c)], bound=BOUND)[0] for r, c in zip(refs, cols)], axis=1)
    assert enc_ref.shape == (NMAX, 36)
    finest = FACE["desired_resolution"]
    for kind in ("align", "heads"):
        got = scene.fused(kind, NMAX, 6, True, 2)
        enc = got["enc_x"].cpu()
        assert np.abs(enc.numpy() - enc_ref).max() <= 1.5e-6 * finest, kind
        w = [v.double() for v in scene.weights_host[kind]]
        for i, tag in enumerate("ab"[:len(w) // 2]):
            a1 = torch.relu(enc.double() @ w[2 * i].t())
            y = a1 @ w[2 * i + 1].t()
            for name, ref in (("a1" + tag, a1), ("y" + tag, y)):
                err = float((got[name].cpu().double() - ref).abs().max())
                assert err <= 2e-5 * max(1.0, float(ref.abs().max())), (kind, name, err)
            # sign words: bit 16 b + r of lane (row & 31) + 32 h of tile row >> 5 <-> feature (r & 3) + 8 (r >> 2) + 4 h
            s1 = got["s1"].cpu().numpy().astype(np.uint32)
            act = got["a1" + tag].cpu().numpy() > 0
            rows = np.arange(NMAX)
            for f in range(act.shape[1]):
                h, r = (f >> 2) & 1, (f & 3) + 4 * (f >> 3)
                bit = (s1[rows >> 5, (rows & 31) + 32 * h] >> (r + 16 * i)) & 1
                assert np.array_equal(bit.astype(bool), act[:, f]), (kind, tag, f)


def _grads(tr):
    out = {k: p.grad.detach().clone() for k, p in tr.g._p.items() if p.grad is not None}
    for name, net in (("umf", tr.motion_net), ("pmf", tr.g.neural_motion_grid)):
        for n_, p_ in net.named_parameters():
            if p_.grad is not None:
                out[f"{name}.{n_}"] = p_.grad.detach().clone()
    return out


def test_train_step_fused_equals_split(monkeypatch):
    """One eager FaceTrainer step: loss and every parameter gradient are the same bits with the fused forward launches as
    with INSTAG_ENCODE_MLP=split, and the fused path is the one that ran."""
    from instag_amd import diff_gauss, encode_mlp
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, PersonalizedMotionNetwork
    from instag_amd.scene_synth import synthetic_frame, synthetic_gaussians, toy_cameras
    from instag_amd.train import FaceTrainer, make_frame
    dev = torch.device("cuda")
    torch.manual_seed(11)
    args = SimpleNamespace(audio_extractor="deepspeech", type="face")
    g = GaussianModel(1, neural_motion_grid=PersonalizedMotionNetwork(args=args).to(dev))
    g.load_raw(synthetic_gaussians(3000, sh_degree=1, seed=5), dev)
    tr = FaceTrainer(g, MotionNetwork(args=args).to(dev), torch.tensor([0.0, 1.0, 0.0], device=dev), densify=False)
    frame = make_frame(toy_cameras(96)[0].to(dev), synthetic_frame(96, 0, dev))
    calls = {"align": 0, "heads": 0}
    for name, key in (("encode_align", "align"), ("encode_heads", "heads")):
        orig = getattr(encode_mlp, name)
        monkeypatch.setattr(encode_mlp, name, lambda *a, _o=orig, _k=key, **kw: (calls.__setitem__(_k, calls[_k] + 1),
                                                                                _o(*a, **kw))[1])
    results = {}
    try:
        for mode in ("fused", "split"):
            monkeypatch.setenv("INSTAG_ENCODE_MLP", mode)
            diff_gauss.set_capacity_plan(None)
            tr._zero_grad()
            _, loss, _ = tr._forward_backward(frame)
            torch.cuda.synchronize()
            results[mode] = (loss.detach().clone(), _grads(tr), dict(calls))
    finally:
        diff_gauss.set_capacity_plan(None)
    assert results["fused"][2] == {"align": 1, "heads": 1} and results["split"][2] == results["fused"][2]
    assert torch.equal(results["fused"][0], results["split"][0])
    gf, gs = results["fused"][1], results["split"][1]
    assert gf.keys() == gs.keys() and any(k.startswith("pmf.align_net") for k in gf) and "umf.encoder_xy.embeddings" in gf
    for k in gs:
        assert torch.equal(gf[k], gs[k]), (k, float((gf[k] - gs[k]).abs().max()))
