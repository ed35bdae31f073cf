"""CPU: instag_amd.track's plain statements against the reference's recorded answers (golden G12), the contour tie
rule, the transforms writer against the dataset reader, the files track_identity writes, and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from instag_amd import dataset as DS
from instag_amd import track
from tests import dataset_helpers as D
from tests import track_helpers as th

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_track.npz")

# max |fp32 statement - fp64 statement| per recorded quantity on the golden's identity (F = 6, P = 5, dims 100 / 79),
# measured on the CPU; the bound of each comparison against the reference's fp32 record is 4 x this.  Measured distance
# of the fp32 statement to the record, in the same order: 0, 0, 3.8e-6, 9.5e-7, 9.5e-7, 1.9e-6, 1.5e-5, 1.9e-7, 9.5e-7,
# 1.9e-6, 1.0e-6, 2.4e-6, 1.3e-7, 4.8e-7, 4.8e-7.
SPREAD = dict(lands=1.469e-07, proj=4.691e-05, loss_lan=2.994e-06, g_id=1.165e-05, g_exp=4.241e-06, g_euler=4.390e-05,
              g_trans=7.651e-05, pose_fit_euler=1.922e-07, pose_fit_trans=8.969e-07, pose_fit_last_loss=2.806e-06,
              joint_fit_id=9.954e-07, joint_fit_exp=2.135e-06, joint_fit_euler=2.143e-07, joint_fit_trans=4.300e-07,
              joint_fit_last_loss=1.204e-06)


@pytest.fixture(scope="module")
def statement():
    g = np.load(GOLDEN)
    m = th.model(12, 5)
    st = track.TrackState(torch.as_tensor(g["lms"]), [1000.0], [0, 6], th.H, th.W, 100, 79, "cpu", torch.float32)
    st.id.copy_(torch.as_tensor(g["id0"]))
    st.exp.copy_(torch.as_tensor(g["exp0"]))
    st.pose.copy_(torch.as_tensor(g["pose0"]))
    lands = track.landmarks_torch(m, st.id.expand(6, -1), st.exp, st.euler, st.trans, 1000.0, st.cx, st.cy)
    r = dict(lands=lands, proj=track.project_torch(lands, st.euler, st.trans, 1000.0, st.cx, st.cy))
    lan, gr, _, _ = track.loss_and_grads_torch(m, st)
    r.update(loss_lan=lan[0], g_id=gr["id"], g_exp=gr["exp"], g_euler=gr["pose"][:, :3], g_trans=gr["pose"][:, 3:])
    track.fit_pose_torch(m, st, 25, 0.1)
    r.update(pose_fit_euler=st.euler.clone(), pose_fit_trans=st.trans.clone(), pose_fit_last_loss=st.loss[0].clone())
    st.fresh_idexp_optimizer()
    track.fit_joint_torch(m, st, 25, 0.1, 0.1)
    r.update(joint_fit_id=st.id.clone(), joint_fit_exp=st.exp.clone(), joint_fit_euler=st.euler.clone(),
             joint_fit_trans=st.trans.clone(), joint_fit_last_loss=st.loss[0].clone())
    return g, r


@pytest.mark.parametrize("key", sorted(SPREAD))
def test_fp32_statement_reproduces_the_reference(statement, key):
    g, r = statement
    want = torch.as_tensor(g[key]).double()
    err = float((r[key].double().reshape(want.shape) - want).abs().max())
    print(f"{key}: |statement - reference| = {err:.3e}, bound {4 * SPREAD[key]:.3e}")
    assert err <= 4 * SPREAD[key]


def test_golden_is_the_seeded_identity(statement):
    """The golden's inputs are what tests/track_helpers.py generates from the seed (the model itself is not recorded)."""
    g, _ = statement
    m = th.model(12, 5)
    ident = th.identity(m, 6, 12, 1000.0)
    assert np.array_equal(ident["lms"].numpy(), g["lms"])
    st = th.perturbed_state(m, ident, [1000.0], 12, dtype=torch.float32)
    assert np.array_equal(st.pose.numpy(), g["pose0"]) and np.array_equal(st.id.numpy(), g["id0"])


def _tie_model():
    # 68 landmarks at distinct x, then 16 slots x 3 candidates.  Left slot 0: candidates 0 and 1 coincide at the smallest
    # x; right slot 0 (slot 8): candidates 1 and 2 coincide at the largest x; every other slot has a unique extreme.
    n = 68 + 48
    pts = np.zeros((n, 3))
    pts[:68, 0] = np.linspace(-0.5, 0.5, 68)
    pts[:68, 1] = np.linspace(-0.4, 0.6, 68)
    cand = np.arange(68, n).reshape(16, 3)
    for s in range(16):
        sign = -1.0 if s < 8 else 1.0
        pts[cand[s], 0] = sign * np.array([0.7, 0.8, 0.9])
        pts[cand[s], 1] = 0.1 * s
    pts[cand[0], 0] = [-0.9, -0.9, -0.7]
    pts[cand[8], 0] = [0.7, 0.9, 0.9]
    z = np.zeros((1, 3 * n))
    return track.Face3DMM(z, z, pts.reshape(-1), np.ones(1), np.ones(1), np.arange(68), cand[:8], cand[8:]), pts, cand


def test_contour_ties_take_the_first_candidate():
    m, pts, cand = _tie_model()
    z = torch.zeros(2, 1, dtype=torch.float64)
    euler = torch.zeros(2, 3, dtype=torch.float64)
    trans = torch.tensor([[0.0, 0.0, -7.0], [0.1, 0.0, -6.0]], dtype=torch.float64)
    lands, choice = track.landmarks_torch(m, z, z, euler, trans, 1000.0, 256.0, 256.0, return_choice=True)
    assert choice[:, 0].tolist() == [0, 0] and choice[:, 8].tolist() == [1, 1]
    assert choice[:, 1:8].eq(2).all() and choice[:, 9:].eq(2).all()
    assert np.array_equal(lands[0, 0].numpy(), pts[cand[0, 0]]) and np.array_equal(lands[0, 9].numpy(), pts[cand[8, 1]])
    assert np.array_equal(lands[0, 8].numpy(), pts[8]) and np.array_equal(lands[0, 17:].numpy(), pts[17:68])


def test_model_checks():
    info, keys = th.model_arrays(3, 2, 5, 3)
    m = track.Face3DMM.from_arrays(info, keys, 5, 3)
    assert (m.id_dim, m.exp_dim, m.P, m.M) == (5, 3, 2, 68 + 32)
    mu = m.mu.reshape(-1, 3)
    assert np.abs(mu.mean(axis=0)).max() < 1e-12 and 0.5 < np.abs(mu).max() < 2.0          # centred, / 1e5
    basis, basis_t, mu_d = m.device_tensors("cpu")
    assert tuple(basis.shape) == (8, 3 * m.M) and tuple(basis_t.shape) == (3 * m.M, 8) and tuple(mu_d.shape) == (3 * m.M,)
    with pytest.raises(ValueError, match="68 entries"):
        track.Face3DMM.from_arrays(info, dict(keys, keyinds=keys["keyinds"][:67]), 5, 3)


def test_face3dmm_load_reads_the_two_dictionaries(tmp_path):
    info, keys = th.model_arrays(3, 2, 5, 3)
    np.save(tmp_path / "3DMM_info.npy", info, allow_pickle=True)
    np.save(tmp_path / "keys_info.npy", keys, allow_pickle=True)
    a, b = track.Face3DMM.load(str(tmp_path), 5, 3), track.Face3DMM.from_arrays(info, keys, 5, 3)
    assert np.array_equal(a.base_id, b.base_id) and np.array_equal(a.mu, b.mu) and np.array_equal(a.points, b.points)


def _euler_np(e):
    t, p, s = e
    rx = np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rz = np.array([[np.cos(s), np.sin(s), 0], [-np.sin(s), np.cos(s), 0], [0, 0, 1]])
    return rx @ ry @ rz


def test_save_transforms_is_what_the_dataset_reader_parses(tmp_path):
    pytest.importorskip("PIL")
    root = str(tmp_path)
    a = D.make_arrays()
    D.write_identity(root, a)                                         # frames 0 .. 8, their own transforms files
    rng = np.random.default_rng(5)
    n = 9
    euler = rng.normal(0, 0.3, (n, 3)).astype(np.float32)
    trans = (rng.normal(0, 0.5, (n, 3)) + np.array([0, 0, -7.0])).astype(np.float32)
    params = dict(focal=torch.tensor([1100.0]), euler=torch.from_numpy(euler), trans=torch.from_numpy(trans))
    track.save_transforms(root, params, D.H, D.W)
    files = {s: json.load(open(os.path.join(root, f"transforms_{s}.json"))) for s in ("train", "val")}
    split = int(n * 10 / 11)
    assert [f["img_id"] for f in files["train"]["frames"]] == list(range(split)) and split == 8
    assert [f["img_id"] for f in files["val"]["frames"]] == list(range(split, n))
    for c in files.values():
        assert c["focal_len"] == 1100.0 and c["cx"] == D.W / 2.0 and c["cy"] == D.H / 2.0
        assert all(f["aud_id"] == f["img_id"] and set(f) == {"img_id", "aud_id", "transform_matrix"} for f in c["frames"])
    want = []
    for i in range(n):
        R, t = _euler_np(euler[i].astype(np.float64)), trans[i].astype(np.float64) / 10.0      # the / 10
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = R.T, -R.T @ t
        want.append(c2w)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    au = DS.read_au_csv(os.path.join(root, "au.csv"))
    lms = lambda i: a["lms"][i]
    t = DS.identity_table(files["train"], au, lms, D.T_AUDIO, "train", n_views=split + 1)
    assert t["focal_len"] == 1100.0 and t["img_id"].tolist() == list(range(split))
    assert np.abs(t["c2w"] - np.array(want[:split])).max() < 2e-6                              # fp32 writer
    rot = t["c2w"][:, :3, :3]
    assert np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    d = DS.read_identity(root, "train", extension=".png", preload_priors=False)              # N_views = -1: drops the last
    assert d["meta"]["img_id"].tolist() == list(range(split - 1)) and len(d["cameras"]) == split - 1
    assert abs(d["meta"]["FovX"] - 2 * np.arctan(D.W / 2200.0)) < 1e-12
    for i in range(split - 1):
        flipped = want[i].copy()
        flipped[:3, 1:3] *= -1
        w2c = np.linalg.inv(flipped)
        assert np.abs(d["meta"]["R"][i] - w2c[:3, :3].T).max() < 2e-6 and np.abs(d["meta"]["T"][i] - w2c[:3, 3]).max() < 2e-6


def _write_lms(directory, ids, lms):
    os.makedirs(directory, exist_ok=True)
    for i, l in zip(ids, lms):
        np.savetxt(os.path.join(directory, f"{i}.lms"), l.numpy(), fmt="%.6f")


def test_read_landmarks_orders_numerically_and_skips_missing_frames(tmp_path):
    ids = [10, 2, 0, 33, 7]
    lms = torch.arange(5 * 136, dtype=torch.float32).reshape(5, 68, 2)
    _write_lms(str(tmp_path), ids, lms)
    (tmp_path / "5.jpg").write_bytes(b"")                              # a frame without landmarks
    (tmp_path / "notes.lms").write_text("not a frame")
    got, got_ids = track.read_landmarks(str(tmp_path))
    assert got_ids == [0, 2, 7, 10, 33] and got.dtype == np.float32 and got.shape == (5, 68, 2)
    for j, i in enumerate(got_ids):
        assert np.array_equal(got[j], lms[ids.index(i)].numpy())
    with pytest.raises(FileNotFoundError):
        track.read_landmarks(str(tmp_path / "nowhere"))


def test_track_identity_writes_the_reference_files(tmp_path):
    m = th.model(4, 2, 5, 3)
    F = 12
    ident = th.identity(m, F, 4, 1000.0)
    _write_lms(str(tmp_path / "ori_imgs"), range(F), ident["lms"])
    with pytest.raises(FileNotFoundError, match="pass h and w"):
        track.track_identity(str(tmp_path), m, "cpu")
    out = track.track_identity(str(tmp_path), m, "cpu", h=th.H, w=th.W, focals=(900, 1000, 1100), every=4,
                               focal_iters=(3, 3), coarse_iters=(3, 3))
    saved = torch.load(os.path.join(str(tmp_path), "track_params.pt"))
    assert list(saved) == ["id", "exp", "euler", "trans", "focal"]
    shapes = dict(id=(1, 5), exp=(F, 3), euler=(F, 3), trans=(F, 3), focal=(1,))
    for k, s in shapes.items():
        assert tuple(saved[k].shape) == s and saved[k].dtype == torch.float32 and saved[k].device.type == "cpu"
        assert torch.equal(saved[k], out[k])
    assert float(saved["focal"]) in (900.0, 1000.0, 1100.0)
    assert len(json.load(open(tmp_path / "transforms_train.json"))["frames"]) == int(F * 10 / 11)
    assert len(json.load(open(tmp_path / "transforms_val.json"))["frames"]) == F - int(F * 10 / 11)


def test_schedules_are_the_reference_loops():
    """Each change takes effect after the step of the iteration that triggers it."""
    assert track.coarse_schedule() == ([(1001, 1.0), (499, 0.1)], [(1001, 0.1), (999, 0.020000000000000004)])
    assert track.focal_schedule() == ([(2000, 0.1)], [(1501, 0.1), (999, 0.020000000000000004)])
    assert track.coarse_schedule((60, 80)) == ([(60, 1.0)], [(80, 0.1)])
    # the reference's loops, replayed
    lr, seen = 1.0, []
    for it in range(1500):
        seen.append(lr)
        if it == 1000:
            lr = 0.1
    assert track._segments(seen) == track.coarse_schedule()[0]


def test_best_focal_is_the_first_strict_minimum():
    assert track._pick_focal([600, 700, 800], [3.0, 2.0, 2.0]) == 700
    assert track._pick_focal([600, 700], [1.0, 1.0]) == 600


def test_track_argument_errors_do_not_need_a_gpu():
    from instag_amd import _lib
    lib = _lib.lib()
    E_ARG = 1
    one = 16
    pointers = [n for n, t in _lib.TrackArgs._fields_ if t is _lib.vp]

    def args(G=1, starts=(0, 4), **kw):
        a = _lib.TrackArgs()
        for n in pointers:
            setattr(a, n, one)
        a._keep = ((_lib.i32 * len(starts))(*starts), (_lib.f32 * G)(*([1000.0] * G)))
        a.group_start, a.focal = (ctypes.addressof(k) for k in a._keep)
        a.G, a.F, a.id_dim, a.exp_dim, a.P, a.n_landmarks = G, starts[-1], 100, 79, 20, 68
        a.cx = a.cy = 256.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def calls(a, n=1):
        return (lib.instag_track_geometry(ctypes.byref(a), None), lib.instag_track_fit_pose(ctypes.byref(a), n, 0.1, None),
                lib.instag_track_fit_joint(ctypes.byref(a), n, 0.1, 0.1, None), lib.instag_track_loss_grad(ctypes.byref(a), None))

    for bad, text in ((dict(P=0), b"P"), (dict(P=65), b"P"), (dict(id_dim=0), b"id_dim"), (dict(id_dim=129), b"id_dim"),
                      (dict(exp_dim=0), b"exp_dim"), (dict(exp_dim=129), b"exp_dim"), (dict(n_landmarks=67), b"68 landmarks"),
                      (dict(basis=None), b"NULL"), (dict(lms=None), b"NULL"), (dict(pose=None), b"NULL"),
                      (dict(state=None), b"NULL"), (dict(G=0), b"groups"), (dict(G=17), b"groups")):
        for rc in calls(args(**bad)):
            assert rc == E_ARG, bad
            assert text in lib.instag_last_error(), (bad, lib.instag_last_error())
    for rc in calls(args(G=2, starts=(0, 4, 4))):
        assert rc == E_ARG and b"empty group" in lib.instag_last_error()
    for rc in calls(args(G=2, starts=(0, 2, 4), F=5)):
        assert rc == E_ARG and b"cover" in lib.instag_last_error()
    # (entries whose arguments all pass would launch on these placeholder pointers: only the rejected forms are called)
    assert lib.instag_track_fit_pose(ctypes.byref(args()), -1, 0.1, None) == E_ARG and b"n >= 0" in lib.instag_last_error()
    assert lib.instag_track_fit_joint(ctypes.byref(args()), -1, 0.1, 0.1, None) == E_ARG
    assert b"n >= 0" in lib.instag_last_error()
    assert lib.instag_track_fit_pose(ctypes.byref(args()), 0, 0.1, None) == 0           # an empty segment: nothing runs
    assert lib.instag_track_fit_joint(ctypes.byref(args(m_exp=None)), 1, 0.1, 0.1, None) == E_ARG
    assert lib.instag_track_loss_grad(ctypes.byref(args(g_exp=None)), None) == E_ARG
    assert lib.instag_track_max_groups() == 16
