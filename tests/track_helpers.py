"""A seeded synthetic 3DMM and identity for the tracking tests (instag_amd/track.py).  Nothing of it is committed: the
model is regenerated from its seed, in the layout of the reference's 3DMM_info.npy / keys_info.npy dictionaries, so the
golden generator (tests/golden/make_golden_track.py) can hand the same arrays to the reference's loader.

The "face" is a cap of ``n_points`` points with real depth relief (z spread comparable to x / y); mu is of order 1 after
the loader's / 1e5, and a unit parameter moves a point by a few percent of the face's size.  keyinds are 68 distinct
points; the contour candidates are 16 P further points, disjoint from them: the left ones scattered over a band at the
left edge of the face (x in -1.1 .. -0.7, depth -0.3 .. 0.5), the right ones mirrored, one narrow range of y per slot,
so which candidate projects outermost depends on the pose."""
import numpy as np
import torch

from instag_amd import track

H = W = 512
N_FREE = 200                      # points that are neither landmark nor candidate (the fit never touches them)


def model_arrays(seed, P, id_dim=100, exp_dim=79):
    """-> (info, keys): the two dictionaries Face3DMM.from_arrays takes."""
    rng = np.random.default_rng(seed)
    n = 68 + 16 * P + N_FREE
    pts = np.empty((n, 3))
    pts[:, 0] = rng.uniform(-1.0, 1.0, n)
    pts[:, 1] = rng.uniform(-1.2, 1.2, n)
    pts[:, 2] = 0.9 * (1.0 - 0.6 * pts[:, 0] ** 2 - 0.4 * pts[:, 1] ** 2) + rng.normal(0, 0.05, n)
    order = rng.permutation(n)
    keyinds, cand = order[:68], order[68:68 + 16 * P].reshape(2, 8, P)
    for side, sign in ((0, -1.0), (1, 1.0)):
        for s in range(8):
            idx = cand[side, s]
            pts[idx, 0] = sign * rng.uniform(0.7, 1.1, P)
            pts[idx, 1] = -1.0 + 0.25 * s + rng.uniform(-0.05, 0.05, P)
            pts[idx, 2] = rng.uniform(-0.3, 0.5, P)
    mu_shape = (pts.reshape(-1) * 1e5) * 0.7 + rng.normal(0, 10.0, 3 * n)
    mu_exp = (pts.reshape(-1) * 1e5) * 0.3
    info = dict(mu_shape=mu_shape, mu_exp=mu_exp,
                b_shape=rng.normal(0, 0.02e5, (id_dim + 3, 3 * n)), b_exp=rng.normal(0, 0.02e5, (exp_dim + 2, 3 * n)),
                sig_shape=rng.uniform(0.5, 1.5, id_dim + 3), sig_exp=rng.uniform(0.5, 1.5, exp_dim + 2))
    keys = dict(keyinds=keyinds.astype(np.int64), left_contour=cand[0].astype(np.int64),
                right_contour=cand[1].astype(np.int64))
    return info, keys


_MODELS = {}


def model(seed, P, id_dim=100, exp_dim=79):
    key = (seed, P, id_dim, exp_dim)
    if key not in _MODELS:
        info, keys = model_arrays(seed, P, id_dim, exp_dim)
        _MODELS[key] = track.Face3DMM.from_arrays(info, keys, id_dim, exp_dim)
    return _MODELS[key]


def identity(m, F, seed, focal=1000.0, noise=0.3):
    """Landmarks of a known fit: dict(lms [F,68,2] float32, id [1,I], exp [F,E], pose [F,6] (fp64), focal)."""
    rng = np.random.default_rng(seed + 1000)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    id_para = t(rng.normal(0, 0.5, (1, m.id_dim)))
    exp = t(rng.normal(0, 0.5, (F, m.exp_dim)))
    pose = t(np.concatenate([rng.normal(0, 0.15, (F, 3)), rng.normal(0, 0.3, (F, 3)) + np.array([0, 0, -7.0])], axis=1))
    lands = track.landmarks_torch(m, id_para.expand(F, -1), exp, pose[:, :3], pose[:, 3:], focal, W / 2.0, H / 2.0)
    proj = track.project_torch(lands, pose[:, :3], pose[:, 3:], focal, W / 2.0, H / 2.0)[:, :, :2]
    lms = (proj + t(rng.uniform(-noise, noise, (F, 68, 2)))).to(torch.float32)
    return dict(lms=lms, id=id_para, exp=exp, pose=pose, focal=float(focal))


def perturbed_state(m, ident, focals, seed, dtype=torch.float64, device="cpu", scale=1.0):
    """A TrackState of len(focals) groups, each holding all frames of ``ident``, started near (not at) the known fit."""
    rng = np.random.default_rng(seed + 2000)
    F, G = int(ident["lms"].shape[0]), len(focals)
    st = track.TrackState(ident["lms"].repeat(G, 1, 1), focals, [F * i for i in range(G + 1)], H, W, m.id_dim, m.exp_dim,
                          "cpu", torch.float64)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    st.id.copy_(ident["id"].expand(G, -1) + scale * t(rng.normal(0, 0.1, (G, m.id_dim))))
    st.exp.copy_(ident["exp"].repeat(G, 1) + scale * t(rng.normal(0, 0.1, (G * F, m.exp_dim))))
    st.pose.copy_(ident["pose"].repeat(G, 1) + scale * t(rng.normal(0, 0.03, (G * F, 6))))
    return st.clone(device=device, dtype=dtype)


def near_tie_frames(m, st64, px_gap=1e-3):
    """Frames of an fp64 state in which some contour slot's best and second-best projected x differ by < px_gap: the
    choice may flip in fp32 there."""
    if m.P < 2:
        return torch.zeros(st64.F, dtype=torch.bool)
    fg = st64.frame_group()
    focal = torch.as_tensor(st64.focals, dtype=torch.float64)[fg]
    geo = track.candidates_torch(m, st64.id[fg], st64.exp)[:, 68:]
    px = track.project_torch(geo, st64.pose[:, :3], st64.pose[:, 3:], focal, st64.cx, st64.cy)[:, :, 0]
    px = px.reshape(st64.F, 16, m.P)
    px = torch.cat((px[:, :8], -px[:, 8:]), dim=1).sort(dim=-1).values
    return ((px[..., 1] - px[..., 0]) < px_gap).any(dim=1)


# ---- parity of the kernels against the fp64 statement (tests/test_track_gpu.py, scripts/track_parity.py) ---------------
EPS32 = float(np.finfo(np.float32).eps)


def state_tensors(st, loss=True):
    d = dict(id=st.id, exp=st.exp, euler=st.pose[:, :3], trans=st.pose[:, 3:])
    if loss:
        d["loss"] = st.loss
    return {k: v.detach().double().cpu() for k, v in d.items()}


def parity(got, want64, stmt32, keep):
    """Per quantity: (|got - fp64|, |fp32 statement - fp64|, bound, floor active), max over the kept frames.  The bound is 4 x the fp32
    statement's own error against the same fp64 run, and never below 4 ulp (fp32) of the quantity's largest magnitude:
    one sample of a rounding error (a scalar loss, a single frame) can be zero by luck, the format's precision cannot.
    ``floor active``: the ulp term, not the statement's error, set the bound."""
    out = {}
    for k, w in want64.items():
        g, s = got[k].double().cpu(), stmt32[k].double().cpu()
        if w.dim() >= 1 and w.shape[0] == keep.shape[0] and k not in ("id", "loss", "g_id"):
            g, s, w = g[keep], s[keep], w[keep]
        if w.numel() == 0:
            continue
        e32 = float((s - w).abs().max())
        floor = EPS32 * float(w.abs().max())
        out[k] = (float((g - w).abs().max()), e32, 4.0 * max(e32, floor), bool(floor > e32))
    return out


def run_fp64_and_fp32(m, st64, steps):
    """steps: [("pose", n, lr) | ("joint", n, lr) | ("fresh",)] run on st64 and on its fp32 copy with the plain
    statements, one iteration at a time; -> (st64, st32, frames that met a near tie at any iteration)."""
    st32 = st64.clone(dtype=torch.float32)
    near = torch.zeros(st64.F, dtype=torch.bool)
    for step in steps:
        for st in (st64, st32):
            if step[0] == "fresh":
                st.fresh_idexp_optimizer()
                continue
            for _ in range(step[1]):
                if st is st64:
                    near |= near_tie_frames(m, st64)
                if step[0] == "pose":
                    track.fit_pose_torch(m, st, 1, step[2])
                else:
                    track.fit_joint_torch(m, st, 1, step[2], step[2])
    return st64, st32, near
