"""GPU: the landmark-fit kernels (csrc/track.hip) against the fp64 plain statement, and their bit-exact properties.

Bounds: every comparison against the fp64 statement allows 4 x the error the fp32 CPU statement makes against the same
fp64 run (tests/track_helpers.parity; the rule of the LPIPS parity), with a floor of 4 fp32 ulp of the quantity's
magnitude.  Frames in which some contour slot's best and second-best candidate lie within 1e-3 px of each other in fp64
may choose differently in fp32 and are left out; at most 2 % of the frames may be (the seeds below were checked on the
CPU: fp32 statement against fp64 statement).  Measured on an MI355X: profiles/r04_track_parity.json, DESIGN section 20."""
import os

import numpy as np
import pytest
import torch

from instag_amd import track
from tests import track_helpers as th

pytestmark = pytest.mark.gpu

# (F, P, id_dim, exp_dim, seed)
CASES = [(1, 1, 100, 79, 21), (3, 5, 100, 79, 22), (70, 33, 100, 79, 23), (70, 5, 100, 79, 24), (3, 33, 100, 79, 20),
         (3, 5, 5, 3, 27)]
IDS = [f"F{c[0]}-P{c[1]}-{c[2]}x{c[3]}" for c in CASES]
# the trajectories leave out every frame that meets a near tie at ANY of their 80 iterations; at F = 70 that holds the 2 %
# only for some seeds, and with P = 33 only from a start closer to the fit (perturbation x 0.1): (case, perturbation scale)
TRAJECTORIES = [(CASES[0], 1.0), (CASES[1], 1.0), ((70, 33, 100, 79, 23), 0.1), ((70, 5, 100, 79, 26), 1.0), (CASES[4], 1.0),
                (CASES[5], 1.0)]


def _setup(case, focals=(1000.0,), scale=1.0):
    F, P, I, E, seed = case
    m = th.model(seed, P, I, E)
    ident = th.identity(m, F, seed, 1000.0)
    return m, th.perturbed_state(m, ident, list(focals), seed, scale=scale)


def _assert_parity(report, what):
    for k, (err, e32, bound, floor) in report.items():
        print(f"{what} {k}: |hip - fp64| = {err:.3e}  |fp32 statement - fp64| = {e32:.3e}  bound {bound:.3e}"
              f"{' (ulp floor)' if floor else ''}")
    for k, (err, e32, bound, _) in report.items():
        assert err <= bound, (what, k, err, e32, bound)


def _keep(near, F):
    assert int(near.sum()) <= 0.02 * F, f"{int(near.sum())} of {F} frames near a contour tie"
    return ~near


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_loss_and_grads_match_fp64_autograd(case):
    m, st64 = _setup(case)
    keep = _keep(th.near_tie_frames(m, st64), st64.F)
    want, got32 = {}, {}
    for st, out in ((st64, want), (st64.clone(dtype=torch.float32), got32)):
        lan, g, frame, choice = track.loss_and_grads_torch(m, st)
        out.update(loss=lan.double(), g_id=g["id"].double(), g_exp=g["exp"].double(), g_pose=g["pose"].double(),
                   frame_loss=frame.double())
        out["choice"] = choice
    tracker = track.LandmarkTracker(m, "cuda")
    st = st64.clone(device="cuda", dtype=torch.float32)
    before = th.state_tensors(st, loss=False)
    lan, g = tracker.loss_and_grads(st)
    got = dict(loss=lan, g_id=g["id"], g_exp=g["exp"], g_pose=g["pose"], frame_loss=st.frame_loss)
    choice64 = want.pop("choice")
    got32.pop("choice")
    _assert_parity(th.parity(got, want, got32, keep), "loss_and_grads")
    assert torch.equal(st.sel.cpu().long()[keep], choice64[keep])
    after = th.state_tensors(st, loss=False)
    assert all(torch.equal(before[k], after[k]) for k in before)          # the updates are switched off


@pytest.mark.parametrize("case,scale", TRAJECTORIES, ids=IDS)
def test_short_trajectories_follow_the_fp64_statement(case, scale):
    m, st64 = _setup(case, scale=scale)
    tracker = track.LandmarkTracker(m, "cuda")
    st = st64.clone(device="cuda", dtype=torch.float32)
    st64, st32, near = th.run_fp64_and_fp32(m, st64, [("pose", 40, 0.1)])
    keep = _keep(near, st64.F)
    tracker.fit_pose(st, 40, 0.1)
    _assert_parity(th.parity(th.state_tensors(st), th.state_tensors(st64), th.state_tensors(st32), keep), "pose")
    assert torch.equal(st.sel.cpu()[keep], st64.sel[keep])
    st64, st32, near2 = th.run_fp64_and_fp32(m, st64, [("fresh",), ("joint", 40, 0.1)])
    keep = _keep(near | near2, st64.F)
    st.fresh_idexp_optimizer()
    tracker.fit_joint(st, 40, 0.1, 0.1)
    _assert_parity(th.parity(th.state_tensors(st), th.state_tensors(st64), th.state_tensors(st32), keep), "joint")
    assert torch.equal(st.sel.cpu()[keep], st64.sel[keep])
    assert st.state.cpu()[0, [0, 3]].tolist() == [80.0, 40.0] and torch.equal(st.state.cpu(), st64.state)


def _bits(st):
    return [getattr(st, k).clone() for k in track.TrackState.TENSORS + ("loss", "frame_loss", "sel")]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_segments_continue_bit_exactly(case):
    m, st64 = _setup(case)
    tracker = track.LandmarkTracker(m, "cuda")
    a, b, c = (st64.clone(device="cuda", dtype=torch.float32) for _ in range(3))
    tracker.fit_pose(tracker.fit_pose(a, 25, 0.1), 15, 0.1)
    tracker.fit_pose(b, 40, 0.1)
    tracker.fit_pose(c, 40, 0.1)
    assert _same(_bits(a), _bits(b)) and _same(_bits(b), _bits(c))       # segments; two runs
    for s in (a, b, c):
        s.fresh_idexp_optimizer()
    tracker.fit_joint(tracker.fit_joint(a, 25, 0.1, 0.1), 15, 0.1, 0.1)
    tracker.fit_joint(b, 40, 0.1, 0.1)
    tracker.fit_joint(c, 40, 0.1, 0.1)
    assert _same(_bits(a), _bits(b)) and _same(_bits(b), _bits(c))
    assert not torch.equal(a.id, st64.id.float().cuda())


def test_learning_rate_change_between_segments_matches_the_statement():
    """The joint loop's change 0.1 -> 0.02 (a change takes effect after the step that triggers it: two segments)."""
    m, st64 = _setup(CASES[1])
    tracker = track.LandmarkTracker(m, "cuda")
    st = st64.clone(device="cuda", dtype=torch.float32)
    st64, st32, near = th.run_fp64_and_fp32(m, st64, [("joint", 25, 0.1), ("joint", 15, 0.02)])
    tracker.fit_joint(tracker.fit_joint(st, 25, 0.1, 0.1), 15, 0.02, 0.02)
    _assert_parity(th.parity(th.state_tensors(st), th.state_tensors(st64), th.state_tensors(st32), _keep(near, st64.F)),
                   "lr change")
    other = st64.clone(device="cuda", dtype=torch.float32)               # (and the rate is not ignored)
    assert not torch.equal(tracker.fit_joint(other, 40, 0.1, 0.1).exp, st.exp)


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
def test_groups_in_one_call_equal_separate_calls(case):
    focals = (900.0, 1000.0, 1100.0)
    m, st64 = _setup(case, focals)
    F = st64.F // 3
    tracker = track.LandmarkTracker(m, "cuda")

    def run(st):
        lan, g = tracker.loss_and_grads(st)
        tracker.fit_pose(st, 12, 0.1)
        st.fresh_idexp_optimizer()
        tracker.fit_joint(st, 12, 0.1, 0.05)
        return [lan, g["id"], g["exp"], g["pose"], st.id, st.exp, st.pose, st.loss, st.frame_loss, st.sel, st.m_exp, st.v_id]

    together = run(st64.clone(device="cuda", dtype=torch.float32))
    for i, f in enumerate(focals):
        one = tracker.init_state(st64.lms[i * F:(i + 1) * F], [f], th.H, th.W)
        one.id.copy_(st64.id[i:i + 1])
        one.exp.copy_(st64.exp[i * F:(i + 1) * F])
        one.pose.copy_(st64.pose[i * F:(i + 1) * F])
        for t, o in zip(together, run(one)):
            part = t[i:i + 1] if t.shape[0] == 3 else t[i * F:(i + 1) * F]
            assert torch.equal(part, o)
    assert not torch.equal(together[4][0], together[4][1])              # the focals do differ


def test_shortened_focal_search_returns_the_statements_focal():
    F, P, seed, every, focals, iters = 24, 5, 27, 4, (600, 1000, 1400), (60, 80)
    m = th.model(seed, P)
    lms = th.identity(m, F, seed, 1000.0)["lms"]
    focal64, loss64 = track.search_focal_torch(m, lms, th.H, th.W, focals, every, iters, dtype=torch.float64)
    focal32, loss32 = track.search_focal_torch(m, lms, th.H, th.W, focals, every, iters, dtype=torch.float32)
    bounds = [4.0 * max(abs(a - b), th.EPS32 * abs(b)) for a, b in zip(loss32, loss64)]
    gaps = [abs(loss64[i] - loss64[j]) for i in range(3) for j in range(i)]
    print("fp64 losses", loss64, "fp32 statement", loss32, "bounds", bounds)
    assert min(gaps) > 10 * max(bounds)
    focal, losses = track.LandmarkTracker(m, "cuda").search_focal(lms, th.H, th.W, focals, every, iters)
    print("hip losses", losses)
    assert focal == focal64 == focal32
    for l, w, b in zip(losses, loss64, bounds):
        assert abs(l - w) <= b


def test_track_identity_writes_and_round_trips(tmp_path):
    F, seed = 12, 28
    m = th.model(seed, 5)
    ident = th.identity(m, F, seed, 1000.0)
    os.makedirs(tmp_path / "ori_imgs")
    for i in range(F):
        np.savetxt(tmp_path / "ori_imgs" / f"{i}.lms", ident["lms"][i].numpy(), fmt="%.6f")
    out = track.track_identity(str(tmp_path), m, "cuda", h=th.H, w=th.W, focals=(800, 1000, 1200), every=3,
                               focal_iters=(30, 30), coarse_iters=(30, 30))
    for name in ("track_params.pt", "transforms_train.json", "transforms_val.json"):
        assert os.path.getsize(tmp_path / name) > 0
    saved = torch.load(tmp_path / "track_params.pt")
    assert list(saved) == ["id", "exp", "euler", "trans", "focal"]
    for k, s in dict(id=(1, 100), exp=(F, 79), euler=(F, 3), trans=(F, 3), focal=(1,)).items():
        assert tuple(saved[k].shape) == s and saved[k].device.type == "cpu" and torch.equal(saved[k], out[k])
        assert torch.isfinite(saved[k]).all()
    assert float(saved["focal"]) in (800.0, 1000.0, 1200.0) and float(saved["trans"][:, 2].mean()) < -3.0
